"""Per-row slot presence on a real MI355X (include/codae_hip.h, "Slot presence"): the gather, every loss primitive and the slot
contrast under a presence table against the float64 statement of the definition (tests/presence_ref.py), independence of what
the data holds under an absent slot (NaN), "off means off", whole steps against the oracle, graph replay and shard invariance,
complete() on incomplete rows, and the refusals.

Fixture.  N = 120 dataset rows, B = 33 (a ragged second row block) and B = 70 (a third), presence_ref.make_table: about 30 %
absent, every row keeps at least 2 present slots (asserted below; the S = 2 kernel shape keeps at least 1 - two of two would be a
table without an absence), row 0 complete and first in the batch, one dataset row twice in the batch, at least one row whose
blanked slot is absent.  Shapes: S = 4, E = 6 (4-wide groups straddle slots), S = 2, E = 12 in bf16 (an 8-wide group straddles),
S = 3, E = 5 in fp32 (the scalar path), S = 3, E = 64 with hidden width 64 for bf16 whole steps.

Tolerances are the ones the same quantities already have: selection adds no rounding.  Element-wise kinds (test_gpu_emphasis.py,
test_gpu_recon_loss.py): fp32 dY rtol 1e-6 / atol 0, bf16 dY one bf16 ulp of the reference, column sums 1e-5 sum |g| per column,
each sum relative B io 2^-24.  slot_cosine (test_gpu_recon_loss.py): |d dY_c| <= (E + 8) 2^-23 k (|x_c| / (nx ny) + |y_c| / |y|^2)
+ 1e-6 |mse term| (+ one bf16 ulp), parts[0] within E (E + 8) 2^-24 sum W + relative B io 2^-24.  Slot contrast
(test_gpu_slot_contrast.py): its fp32 bound, and for bf16 operands 4 x its measured normalised error 1.965e-2 plus one bf16 ulp.
Whole steps: rtol 1e-3 / atol 1e-5 in fp32, 2e-3 relative L2 per gradient tensor of the first step in bf16.  In every case dY
under an absent element is exactly +0 (all bits zero).
"""
import ctypes as C
import math

import numpy as np
import pytest

import contrast_ref as CR
import emphasis_ref as ER
import presence_ref as PR
import recon_loss_ref as RR
from golden_util import close, max_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"

U = 2.0 ** -24
N = 120
STEP = 5
FILL = 7.0
ALPHA, BETA = 3.0, 0.5
NOISE_SEED = ER.SEED
NOISES = [("off", None), ("gaussian", dict(sigma=0.3)), ("masking", dict(p=0.25)), ("salt_pepper", dict(p=0.1, lo=-0.75, hi=1.5))]
KIND_ID = dict(mse=0, l1=1, smooth_l1=2, huber=3, slot_cosine=4)
BF16_CONTRAST_BOUND = 4.0 * 1.965e-2          # test_gpu_slot_contrast.py's BF16_BOUND


def _bits(t):
    return t.view({torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64, torch.uint8: torch.uint8}[t.dtype])


def _bf16_ulp(ref):
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.floor(np.log2(np.abs(ref)))
    return np.where((ref == 0) | ~np.isfinite(ref), 0.0, 2.0 ** (e - 7))


def _noise(kind, kw):
    from codae.tool import InputNoise
    return (None, None) if kw is None else (InputNoise(kind, seed=NOISE_SEED, **kw), (kind, kw, NOISE_SEED))


_PROBLEMS = {}


def _problem(io, S, B=33):
    """emphasis_ref.problem with a presence table; `data` holds NaN under every absent slot, `data0` zeros (what a dataset built
    with keep_incomplete stores); numpy arrays are never modified, device tensors are made once per session."""
    key = (io, S, B)
    if key not in _PROBLEMS:
        p = dict(ER.problem(io, S=S, N=N, B=B))
        E = io // S
        t = PR.make_table(N, S, min_keep=2 if S > 2 else 1)
        rows = p["rows"].copy()
        if 0 not in rows:
            rows[0] = 0
        else:
            i = int(np.flatnonzero(rows == 0)[0])
            rows[0], rows[i] = rows[i], rows[0]
        rows[5] = rows[4]                                          # one dataset row twice in the batch
        pm_all = np.repeat(t != 0, E, axis=1)
        p.update(S=S, E=E, rows=rows, present=t, data0=np.where(pm_all, p["data"], np.float32(0)),
                 data=np.where(pm_all, p["data"], np.float32(np.nan)), cw=np.repeat(np.float32(np.linspace(0.5, 2.0, S)), E))
        # the fixture conditions
        assert (t.sum(axis=1) >= (2 if S > 2 else 1)).all() and 0.1 < (t == 0).mean() < 0.4
        assert rows[0] == 0 and t[0].all()
        assert (t[rows, p["mask_id"]] == 0).any() and (t[rows, p["mask_id"]] != 0).any()       # a row whose blanked slot is absent
        assert (t[rows] == 0).any(axis=1).sum() >= 5
        p["dev"] = {k: torch.tensor(p[k], device=DEV) for k in ("data", "data0", "y", "table", "rows", "mask_id", "mtu", "present", "cw")}
        _PROBLEMS[key] = p
    return _PROBLEMS[key]


def _routes(p):
    """(name, batch kwargs, dataset rows, keep): mask ids direct with permuted rows; the device-side id lookup with row_idx NULL
    (the callers pass B); no mask."""
    d, B, io = p["dev"], p["B"], p["io"]
    return [("mask_id", dict(row_idx=d["rows"], mask_id=d["mask_id"], table=d["table"]), p["rows"], p["table"][p["mask_id"]]),
            ("mask_to_use", dict(table=d["table"], mask_to_use=d["mtu"], run=2), np.arange(B), p["table"][p["mtu"][:B, 2]]),
            ("no-mask", dict(row_idx=d["rows"]), p["rows"], np.ones((B, io), np.uint8))]


def _batch(data, B, row_idx=None, mask_id=None, table=None, mask_to_use=None, run=0):
    from codae import hip
    return hip.Batch(hip.ptr(data), hip.ptr(row_idx), hip.ptr(mask_id), hip.ptr(table), B, int(data.shape[1]), hip.ptr(mask_to_use),
                     0 if mask_to_use is None else int(mask_to_use.shape[1]), run)


def _B(y, B, row_idx):
    return int(row_idx.numel()) if row_idx is not None else (int(y.shape[0]) if B is None else B)


# ---- 1. the gather ---------------------------------------------------------------------------------------------------------------

def gather(data, present, S, noise, step, bf16, ld=None, B=None, **route):
    """(codae_corrupt_batch, codae_corrupt_batch_present) on the same arguments -> two [B, ld] tensors prefilled with FILL."""
    from codae import hip
    lib = hip.lib()
    io = int(data.shape[1])
    B = int(route["row_idx"].numel()) if route.get("row_idx") is not None else B
    ld = io if ld is None else ld
    batch = _batch(data, B, **route)
    st = None if noise is None else noise.as_struct()
    outs = []
    for pres in (None, present):
        out = torch.full((B, ld), FILL, dtype=torch.bfloat16 if bf16 else torch.float32, device=DEV)
        if pres is None:
            rc = lib.codae_corrupt_batch(C.byref(batch), None if st is None else C.byref(st), step, None, hip.ptr(out), int(bf16), ld,
                                         hip.current_stream())
        else:
            rc = lib.codae_corrupt_batch_present(C.byref(batch), None if st is None else C.byref(st), step, None, hip.ptr(out), int(bf16),
                                                 ld, hip.ptr(pres), S, hip.current_stream())
        assert rc == 0, hip.lib().codae_last_error()
        outs.append(out)
    torch.cuda.synchronize()
    return outs


GATHER_SHAPES = [(24, 4, False, None, 33), (24, 4, True, 64, 70), (24, 2, True, None, 33), (15, 3, False, None, 33), (24, 4, False, 28, 33)]


@pytest.mark.parametrize("kind,kw", NOISES, ids=[k for k, _ in NOISES])
@pytest.mark.parametrize("io,S,bf16,ld,B", GATHER_SHAPES, ids=["s4e6-f32", "s4e6-bf16-ld64-b70", "s2e12-bf16x8", "s3e5-scalar", "s4e6-f32-ld28"])
def test_gather_writes_zero_in_absent_slots_and_todays_bits_elsewhere(io, S, bf16, ld, B, kind, kw):
    """Data with NaN under every absent slot.  Absent columns: exactly +0, noise or not; every other column and the pad columns:
    the bits of codae_corrupt_batch.  Without Gaussian noise the values are also the reference's, exactly."""
    p = _problem(io, S, B)
    d = p["dev"]
    noise, noise_ref = _noise(kind, kw)
    for name, route, rows, keep in _routes(p):
        today, got = gather(d["data"], d["present"], S, noise, STEP, bf16, ld, B=B, **route)
        pm = torch.tensor(PR.pmask(p["present"], rows, p["E"]), device=DEV)
        assert (_bits(got[:, :io])[~pm] == 0).all(), name                        # exactly +0
        assert torch.equal(_bits(got[:, :io])[pm], _bits(today[:, :io])[pm]), name
        assert torch.equal(_bits(got[:, io:]), _bits(today[:, io:])) and (got[:, io:].float() == FILL).all()
        assert not torch.isnan(got[:, :io].float()).any() and torch.isnan(today[:, :io].float()).any()
        if kind != "gaussian":
            ref = PR.gather(p["data"][rows], rows, None if name == "no-mask" else keep, p["present"], STEP, noise_ref)
            want = torch.tensor(ref, device=DEV)
            assert torch.equal(_bits(got[:, :io]), _bits(want.to(got.dtype))), name
    # all ones: the bits of the gather without a table
    ones = torch.ones_like(d["present"])
    today, got = gather(d["data0"], ones, S, noise, STEP, bf16, ld, row_idx=d["rows"], mask_id=d["mask_id"], table=d["table"])
    assert torch.equal(_bits(today), _bits(got))


# ---- 2. the loss primitives --------------------------------------------------------------------------------------------------------

def loss_call(which, data, y, present, S, B=None, noise=None, step=STEP, emph=None, loss=None, dy_bf16=False, dy_ld=None, inv_n=None,
              want_dy=True, **route):
    """which: "mse" (codae_mse_loss_present, parts [blocks, 2]), "emph" or "recon" (parts [blocks, 3]) -> (rc, dy, colsum, parts)."""
    from codae import hip
    lib = hip.lib()
    io = int(data.shape[1])
    B = _B(y, B, route.get("row_idx"))
    ld = io if dy_ld is None else dy_ld
    blocks = (B + 31) // 32
    dy = torch.full((B, ld), FILL, dtype=torch.bfloat16 if dy_bf16 else torch.float32, device=DEV)
    colsum = torch.full((blocks, io), FILL, dtype=torch.float32, device=DEV)
    parts = torch.full((blocks, 2 if which == "mse" else 3), FILL, dtype=torch.float64, device=DEV)
    batch = _batch(data, B, **route)
    st = None if noise is None else noise.as_struct()
    inv = (1.0 / (B * io)) if inv_n is None else inv_n
    pp, s = hip.ptr(present), hip.current_stream()
    if which == "mse":
        rc = lib.codae_mse_loss_present(C.byref(batch), hip.ptr(y), hip.ptr(dy) if want_dy else None, int(dy_bf16), ld, inv, hip.ptr(colsum),
                                        hip.ptr(parts), pp, S, s)
    elif which == "emph":
        em = hip.Emphasis(emph[0], emph[1], hip.ptr(emph[2]))
        rc = lib.codae_emph_loss_present(C.byref(batch), None if st is None else C.byref(st), step, C.byref(em), hip.ptr(y), hip.ptr(dy),
                                         int(dy_bf16), ld, inv, hip.ptr(colsum), hip.ptr(parts), pp, S, s)
    else:
        em = None if emph is None else hip.Emphasis(emph[0], emph[1], hip.ptr(emph[2]))
        rc = lib.codae_recon_loss_fwd_bwd_present(C.byref(batch), None if st is None else C.byref(st), step, None if em is None else C.byref(em),
                                                  C.byref(loss), hip.ptr(y), hip.ptr(dy), int(dy_bf16), ld, inv, hip.ptr(colsum),
                                                  hip.ptr(parts), pp, S, s)
    torch.cuda.synchronize()
    return rc, dy, colsum, parts


def _check_elementwise(out, ref, p, B, dy_bf16, masked, n_sums=3, bound=None):
    """test_gpu_emphasis.py's checks, plus +0 under absent elements.  bound [B, io]: an absolute fp32 bound instead of rtol 1e-6."""
    rc, dy, colsum, parts = out
    io = p["io"]
    assert rc == 0
    pm = ref["pm"]
    assert (_bits(dy[:, :io]).cpu().numpy()[~pm] == 0).all()                     # exactly +0, not -0
    got = dy[:, :io].float().cpu().numpy().astype(np.float64)
    err = np.abs(got - ref["dy"])
    if bound is not None:
        tol = bound + (_bf16_ulp(ref["dy"]) if dy_bf16 else 0.0)
        assert (err <= tol).all(), float((err / np.maximum(tol, 1e-300)).max())
    elif dy_bf16:
        assert (err <= _bf16_ulp(ref["dy"])).all(), float((err / np.maximum(_bf16_ulp(ref["dy"]), 1e-300)).max())
    else:
        np.testing.assert_allclose(got, ref["dy"], rtol=1e-6, atol=0)
    assert (dy[:, io:].float() == FILL).all()                                    # pad columns stay as found
    cs = colsum.cpu().numpy().astype(np.float64).sum(axis=0)
    cs_tol = 1e-5 * ref["colsum_abs"] + (0.0 if bound is None else bound.sum(axis=0))
    assert (np.abs(cs - ref["colsum"]) <= cs_tol).all(), float(np.abs(cs - ref["colsum"]).max())
    sums = parts.cpu().numpy().sum(axis=0)
    want = ((ref["crit"],) if n_sums == 3 else ()) + (ref["sq"], ref["sqp"] if masked else 0.0)
    print("sums", sums, want)
    return sums, want


LOSS_SHAPES = [(24, 4, False, None, 33), (24, 4, True, 64, 70), (24, 2, True, None, 33), (15, 3, False, None, 33)]
LOSS_IDS = ["s4e6-f32", "s4e6-bf16-ld64-b70", "s2e12-bf16", "s3e5-scalar"]


def _poisoned_and_clean(call):
    """call(data tensor) twice - NaN and zeros under the absent slots: the same bits, and the NaN run's outputs returned."""
    def run(p, **kw):
        a = call(p["dev"]["data"], **kw)
        b = call(p["dev"]["data0"], **kw)
        assert a[0] == 0 and b[0] == 0
        for u, v in zip(a[1:], b[1:]):
            assert torch.equal(_bits(u), _bits(v))
        return a
    return run


@pytest.mark.parametrize("io,S,bf16,ld,B", LOSS_SHAPES, ids=LOSS_IDS)
def test_mse_and_emphasised_loss_match_the_definition(io, S, bf16, ld, B):
    """codae_mse_loss_present (the evaluation sums' kernel) and codae_emph_loss_present with alpha 3, beta 0.5, slot weights and
    MASKING noise, through the three mask routes; rule 5 for the sums: present only, present and blanked only."""
    p = _problem(io, S, B)
    d = p["dev"]
    noise, noise_ref = _noise("masking", dict(p=0.25))
    for name, route, rows, keep in _routes(p):
        x = p["data"][rows]
        ref = PR.loss_terms("mse", x, p["y"], keep, None, np.float32(1.0 / (B * io)), p["present"], rows)
        run = _poisoned_and_clean(lambda data, **kw: loss_call("mse", data, d["y"], d["present"], S, B=B, dy_bf16=bf16, dy_ld=ld, **kw))
        sums, want = _check_elementwise(run(p, **route), ref, p, B, bf16, name != "no-mask", n_sums=2)
        for g, r in zip(sums, want):
            assert abs(g - r) <= B * io * U * r, (name, g, r)
        w = ER.weights(ER.corrupted(keep, rows, STEP, noise_ref), ALPHA, BETA, p["cw"])
        ref = PR.loss_terms("mse", x, p["y"], keep, w, np.float32(1.0 / (B * io)), p["present"], rows)
        run = _poisoned_and_clean(lambda data, **kw: loss_call("emph", data, d["y"], d["present"], S, B=B, noise=noise, emph=(ALPHA, BETA, d["cw"]),
                                                               dy_bf16=bf16, dy_ld=ld, **kw))
        sums, want = _check_elementwise(run(p, **route), ref, p, B, bf16, name != "no-mask")
        for g, r in zip(sums, want):
            assert abs(g - r) <= B * io * U * r, (name, g, r)
        # not vacuous: the sums without the table are larger (the absent targets are NaN there, so compare on the zero-filled data)
        full = ER.loss_terms(p["data0"][rows], p["y"], keep, w, 1.0)
        assert full["sq"] > 1.1 * ref["sq"]
    # sums only (dy NULL): the evaluation form
    rc, dy, colsum, parts = loss_call("mse", d["data"], d["y"], d["present"], S, B=B, want_dy=False, row_idx=d["rows"], mask_id=d["mask_id"],
                                      table=d["table"])
    ref = PR.loss_terms("mse", p["data"][p["rows"]], p["y"], p["table"][p["mask_id"]], None, 1.0, p["present"], p["rows"])
    assert rc == 0 and (dy == FILL).all()
    got = parts.cpu().numpy().sum(axis=0)
    assert abs(got[0] - ref["sq"]) <= B * io * U * ref["sq"] and abs(got[1] - ref["sqp"]) <= B * io * U * ref["sqp"]


ELEM = [("l1", None), ("smooth_l1", 0.5), ("huber", 0.75)]


@pytest.mark.parametrize("kind,param", ELEM, ids=[k for k, _ in ELEM])
@pytest.mark.parametrize("io,S,bf16,ld,B", LOSS_SHAPES, ids=LOSS_IDS)
def test_elementwise_criteria_match_the_definition(io, S, bf16, ld, B, kind, param):
    from codae import hip
    p = _problem(io, S, B)
    d = p["dev"]
    noise, noise_ref = _noise("masking", dict(p=0.25))
    st = hip.ReconLoss(KIND_ID[kind], 0.0 if param is None else param, 0.0, 0)
    for name, route, rows, keep in _routes(p)[:2]:
        x = p["data"][rows]
        for emph_on in (False, True):
            w = ER.weights(ER.corrupted(keep, rows, STEP, noise_ref), ALPHA, BETA, p["cw"]) if emph_on else None
            ref = PR.loss_terms(kind, x, p["y"], keep, w, np.float32(1.0 / (B * io)), p["present"], rows, param=param)
            if kind == "l1":
                dd = np.abs(p["data0"][rows].astype(np.float64) - p["y"])[ref["pm"]]
                assert dd.min() > 1e-6                                       # sign(d) is never in doubt
            run = _poisoned_and_clean(lambda data, **kw: loss_call("recon", data, d["y"], d["present"], S, B=B, noise=noise if emph_on else None,
                                                                   emph=(ALPHA, BETA, d["cw"]) if emph_on else None, loss=st, dy_bf16=bf16,
                                                                   dy_ld=ld, **kw))
            sums, want = _check_elementwise(run(p, **route), ref, p, B, bf16, True)
            for g, r in zip(sums, want):
                assert abs(g - r) <= B * io * U * r, (name, emph_on, g, r)


@pytest.mark.parametrize("mw", [0.0, 0.25], ids=["cos", "cos+mse"])
@pytest.mark.parametrize("io,S,bf16,ld,B", LOSS_SHAPES, ids=LOSS_IDS)
def test_slot_cosine_skips_absent_pairs(io, S, bf16, ld, B, mw):
    """An absent pair gives 0 to the loss and +0 to dY - not the term W of a zero present target, which the fixture also has."""
    from codae import hip
    p = _problem(io, S, B)
    d = p["dev"]
    E = p["E"]
    noise, noise_ref = _noise("masking", dict(p=0.25))
    st = hip.ReconLoss(KIND_ID["slot_cosine"], 0.0, mw, S)
    rows, keep = p["rows"], p["table"][p["mask_id"]]
    # a zero PRESENT target: slot s0 of batch row 1 (its dataset row is in no other batch row)
    s0 = int(np.flatnonzero(p["present"][rows[1]])[0])
    assert (rows == rows[1]).sum() == 1
    data = p["data"].copy()
    data[rows[1], s0 * E:(s0 + 1) * E] = 0.0
    data_t = torch.tensor(data, device=DEV)
    for emph_on in (False, True):
        w = ER.weights(ER.corrupted(keep, rows, STEP, noise_ref), ALPHA, BETA, p["cw"]) if emph_on else None
        inv = np.float32(1.0 / (B * io))
        ref = PR.loss_terms("slot_cosine", data[rows], p["y"], keep, w, inv, p["present"], rows, mse_weight=mw, S=S)
        assert ref["cos"][1, s0] == 0.0 and ref["W"][1, s0] > 0
        out = loss_call("recon", data_t, d["y"], d["present"], S, B=B, noise=noise if emph_on else None,
                        emph=(ALPHA, BETA, d["cw"]) if emph_on else None, loss=st, dy_bf16=bf16, dy_ld=ld, row_idx=d["rows"], mask_id=d["mask_id"],
                        table=d["table"])
        bound = (E + 8) * 2.0 ** -23 * ref["bound_scale"] + 1e-6 * ref["mse_part"]
        sums, want = _check_elementwise(out, ref, p, B, bf16, True, bound=bound)
        tol0 = E * (E + 8) * U * ref["W"].sum() + B * io * U * abs(want[0])
        assert abs(sums[0] - want[0]) <= tol0, (sums[0], want[0], tol0)
        for g, r in zip(sums[1:], want[1:]):
            assert abs(g - r) <= B * io * U * r, (g, r)
        # the absent pairs would have added W each: the comparison is not vacuous
        # (without the table, on zero-filled data, each absent pair is a zero target and adds its W >= 0.25)
        absent_pairs = int((p["present"][rows] == 0).sum())
        plain = RR.loss_terms("slot_cosine", np.where(ref["pm"], data[rows], np.float32(0)), p["y"], keep, w, inv, mse_weight=mw, S=S)["crit"]
        assert absent_pairs >= 5 and plain - want[0] > 0.2 * E * absent_pairs
    # a criterion whose slots disagree with the table is refused and writes nothing
    bad = hip.ReconLoss(KIND_ID["slot_cosine"], 0.0, mw, 1)
    rc, dy, colsum, parts = loss_call("recon", data_t, d["y"], d["present"], S, B=B, loss=bad, row_idx=d["rows"])
    assert rc == -1 and (dy == FILL).all() and (parts == FILL).all()


def contrast_call(p, data, K, tau, weight, seed, scale, bf16, dy_in, item_id=None, emph=None, noise=None, rows=None, sl=None, step=STEP):
    """prepare_present + fwd_bwd_present on the mask_id route (batch rows `sl`, a slice) -> (rc, dy, colsum, parts, ws)."""
    from codae import hip
    lib = hip.lib()
    d, io, S = p["dev"], p["io"], p["S"]
    sl = slice(0, p["B"]) if sl is None else sl
    row_idx, mask_id, y = d["rows"][sl].contiguous(), d["mask_id"][sl].contiguous(), d["y"][sl].contiguous()
    B = int(row_idx.numel())
    blocks = (B + 31) // 32
    dt = torch.bfloat16 if bf16 else torch.float32
    dy = torch.full((B + 32, io), FILL, dtype=dt, device=DEV)
    dy[:B] = dy_in[sl].to(dt)
    colsum = torch.full((blocks, io), FILL, dtype=torch.float32, device=DEV)
    parts = torch.full((blocks,), FILL, dtype=torch.float64, device=DEV)
    ws = torch.full((lib.codae_slot_contrast_ws_bytes(S, K, io // S, int(bf16)),), 0xFF, dtype=torch.uint8, device=DEV)
    st = hip.SlotContrast(S, K, tau, weight, seed, N, 0, int(ws.numel()), None, hip.ptr(item_id), hip.ptr(ws))
    batch = _batch(data, B, row_idx=row_idx, mask_id=mask_id, table=d["table"])
    ns = None if noise is None else noise.as_struct()
    em = None if emph is None else hip.Emphasis(emph[0], emph[1], hip.ptr(emph[2]))
    rc = lib.codae_slot_contrast_prepare_present(hip.ptr(data), io, C.byref(st), step, int(bf16), hip.ptr(d["present"]), S, hip.current_stream())
    if rc == 0:
        rc = lib.codae_slot_contrast_fwd_bwd_present(C.byref(batch), None if ns is None else C.byref(ns), step, None if em is None else C.byref(em),
                                                     C.byref(st), hip.ptr(y), hip.ptr(dy), int(bf16), io, scale, hip.ptr(colsum), hip.ptr(parts),
                                                     hip.ptr(d["present"]), S, hip.current_stream())
    torch.cuda.synchronize()
    assert (dy[B:].float() == FILL).all()
    return rc, dy[:B], colsum, parts, ws


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("io,S,K,tau,emph_on,ids_on,B", [(24, 4, 33, 0.1, True, True, 33), (24, 2, 5, 0.5, False, False, 70), (15, 3, 33, 0.1, False, True, 33)],
                         ids=["s4e6-k33-emph-ids", "s2e12-k5-b70", "s3e5-k33-ids"])
def test_slot_contrast_skips_absent_pairs_and_absent_candidates(io, S, K, tau, emph_on, ids_on, B, bf16):
    """An absent pair is a pair without a positive; a candidate whose slot is absent is left out of every pair and reaches the
    products as zeros: the NaN under it in `data` changes no bit.  The draw is the one without a table."""
    p = _problem(io, S, B)
    d = p["dev"]
    E = p["E"]
    seed = 0x5EED0000C0DA0001
    weight = 0.7
    scale = float(np.float32(weight / (B * S)))
    rows, keep = p["rows"], p["table"][p["mask_id"]]
    noise, noise_ref = _noise("masking", dict(p=0.25)) if emph_on else (None, None)
    ids = CR.item_ids(p["data0"], S).astype(np.int32) if ids_on else None
    ids_t = None if ids is None else torch.tensor(ids, device=DEV)
    dy_in = (np.random.default_rng(io + K).standard_normal((B, io)) * 1e-2).astype(np.float32)
    dy_in[~PR.pmask(p["present"], rows, E)] = 0.0                            # what the criterion's kernel leaves there
    dy_in_t = torch.tensor(dy_in, device=DEV)
    dt = torch.bfloat16 if bf16 else torch.float32
    dy_used = dy_in_t.to(dt).float().cpu().numpy()
    W = None
    if emph_on:
        w = ER.weights(ER.corrupted(keep, rows, STEP, noise_ref), ALPHA, BETA, p["cw"])
        W = np.where(PR.pmask(p["present"], rows, E), w, 0.0).reshape(B, S, E).mean(-1)
    ref = PR.contrast_terms(p["data"], p["present"], p["data"][rows], p["y"], rows, STEP, S, K, tau, scale, seed, W=W, item_id=ids, dy_in=dy_used)
    # the fixture: absent candidates, absent pairs, and the same draw as without a table
    assert ref["absent_cand"].any() and (~ref["absent_cand"]).any() and (p["present"][rows] == 0).any()
    for s in range(S):
        assert np.array_equal(ref["cand"][s], CR.candidate_rows(STEP, s, K, seed, N))
    common = dict(item_id=ids_t, emph=(ALPHA, BETA, d["cw"]) if emph_on else None, noise=noise)
    out = contrast_call(p, d["data"], K, tau, weight, seed, scale, bf16, dy_in_t, **common)
    clean = contrast_call(p, d["data0"], K, tau, weight, seed, scale, bf16, dy_in_t, **common)
    assert out[0] == 0 and clean[0] == 0
    for a, b in zip(out[1:], clean[1:]):
        assert torch.equal(_bits(a), _bits(b))                                   # the work space included
    rc, dy, colsum, parts, ws = out
    pm = PR.pmask(p["present"], rows, E)
    assert (_bits(dy).cpu().numpy()[~pm] == 0).all()
    got = dy.float().cpu().numpy().astype(np.float64)
    err = np.abs(got - ref["dy"])
    norm = np.repeat(ref["k"] / (tau * np.maximum(ref["ny"], 1e-300)), E, axis=1)
    if bf16:
        bound = BF16_CONTRAST_BOUND * norm + _bf16_ulp(ref["dy"])
        dl_tol = 2 * 2.0 ** -8 / tau
    else:
        dcos = (2 * E + 24) * U
        dl_tol = 2 * dcos / tau + 8 * (2 / tau + 9) * U
        rel = dl_tol + (K + E + 16) * U
        bound = norm * rel * (ref["bs"] + ref["yh"] * np.repeat(ref["bsn"], E, axis=1)) + 4 * U * np.abs(ref["own"]) + U * np.abs(ref["dy"])
    print("worst error / bound %.3f" % float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    assert np.abs(ref["own"]).max() > 1e-3 * np.abs(dy_in).max()                # the term moves dY
    cs = colsum.cpu().numpy().astype(np.float64)
    tol = np.stack([bound[i * 32:(i + 1) * 32].sum(axis=0) + 1e-5 * np.abs(ref["dy"][i * 32:(i + 1) * 32]).sum(axis=0) for i in range(len(cs))])
    assert (np.abs(cs - ref["colsum"]) <= tol).all()
    pt = parts.cpu().numpy()
    Wb = np.array([ref["W"][i * 32:(i + 1) * 32].sum() for i in range(len(pt))])
    assert (np.abs(pt - ref["parts"]) <= dl_tol * Wb + B * S * U * np.abs(ref["parts"])).all(), (pt, ref["parts"])
    # without the table the loss differs: the absent candidates count and the absent pairs score their zeros
    plain = CR.terms(p["data0"], p["data0"][rows], p["y"], rows, STEP, S, K, tau, scale, seed, W=W, item_id=ids, dy_in=dy_used)
    assert abs(plain["loss"] - ref["loss"]) > 1e-4 * abs(ref["loss"])
    # a sub-batch with the global scale: the bits of the same rows of the whole batch
    part = contrast_call(p, d["data"], K, tau, weight, seed, scale, bf16, dy_in_t, sl=slice(8, 21), **common)
    assert part[0] == 0 and torch.equal(_bits(part[1]), _bits(dy[8:21]))


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_a_shards_dy_rows_are_the_whole_batchs_bits_s4e6_b70(bf16):
    """Rows 8 .. 40 launched as their own batch with the global inv_n: element-wise kinds and the cosine."""
    from codae import hip
    p = _problem(24, 4, 70)
    d = p["dev"]
    noise, _ = _noise("masking", dict(p=0.25))
    inv = 1.0 / (70 * 24)
    sub = dict(row_idx=d["rows"][8:41].contiguous(), mask_id=d["mask_id"][8:41].contiguous(), table=d["table"])
    whole = dict(row_idx=d["rows"], mask_id=d["mask_id"], table=d["table"])
    cases = [("emph", None)] + [("recon", hip.ReconLoss(KIND_ID[k], 0.5, 0.25 if k == "slot_cosine" else 0.0, 4 if k == "slot_cosine" else 0))
                                for k in ("l1", "smooth_l1", "huber", "slot_cosine")]
    for which, st in cases:
        kw = dict(noise=noise, emph=(ALPHA, BETA, d["cw"]), loss=st, dy_bf16=bf16, inv_n=inv)
        full = loss_call(which, d["data"], d["y"], d["present"], 4, **kw, **whole)
        part = loss_call(which, d["data"], d["y"][8:41].contiguous(), d["present"], 4, **kw, **sub)
        assert full[0] == 0 and part[0] == 0
        assert torch.equal(_bits(part[1]), _bits(full[1][8:41])), which


# ---- engines -----------------------------------------------------------------------------------------------------------------------

def _stack(io, S, z, B, seed, poison=False):
    """io -> z -> io, S one-slot masks, one mask run; the data holds zeros (or NaN) under the absent slots."""
    from oracle import dae_oracle as O
    rng = np.random.default_rng(seed)
    E = io // S
    data = rng.random((N, io), dtype=np.float32)
    present = PR.make_table(N, S, seed=seed)
    assert (present.sum(axis=1) >= 2).all() and (present == 0).mean() > 0.1
    pm = np.repeat(present != 0, E, axis=1)
    data0 = np.where(pm, data, np.float32(0))
    sched = [(io, z, True), (z, io, False)]
    params = O.init_params(sched, rng)
    bm, nmr, _ = O.corrupter_tables([{"size": E, "position": s * E} for s in range(S)], 1)
    mtu = rng.integers(0, S, (N, 1)).astype(np.int32)
    order = [rng.permutation(N)[:B].astype(np.int32) for _ in range(4)]
    for o in order:
        o[3] = o[2]                                                   # a repeated row
        assert (present[o, mtu[o, 0]] == 0).any() and present[o].all(axis=1).any()
    return dict(io=io, S=S, E=E, data=np.where(pm, data, np.float32(np.nan)) if poison else data0, data0=data0, present=present, sched=sched,
                params=params, bm=bm, nmr=nmr, mtu=mtu, order=order, B=B)


def _trainer(p, precision, with_presence=True, **kw):
    from codae.tool import SlotPresence
    from codae.train import HipEmbeddingTrainer
    if with_presence:
        kw["presence"] = SlotPresence(p["present"])
    t = HipEmbeddingTrainer(p["sched"], torch.tensor(p["data"]), torch.tensor(p["bm"]).to(torch.uint8), torch.tensor(p["mtu"]), 1e-3,
                            1e-4, 1.0, max_batch=p["B"], precision=precision, device=DEV, n_slots=p["S"], **kw)
    t.load_params(p["params"])
    return t


def _idx(p, s):
    return torch.tensor(p["order"][s], dtype=torch.int32, device=DEV)


def _fmask(p, idx, run=0):
    from oracle import dae_oracle as O
    return O.get_masks(p["bm"], p["nmr"], p["mtu"], 1, idx, run)[1]


def _settings(name):
    """trainer kwargs of a named step setting."""
    from codae.tool import InputNoise, LossEmphasis, ReconstructionLoss, SlotContrast
    if name == "mse":
        return {}
    if name == "mse+emphasis+noise":
        return dict(input_noise=InputNoise("masking", p=0.25, seed=20260), loss_emphasis=LossEmphasis(ALPHA, BETA))
    if name == "huber":
        return dict(criterion=ReconstructionLoss("huber", delta=0.75))
    if name == "slot_cosine":
        return dict(criterion=ReconstructionLoss("slot_cosine", mse_weight=0.25))
    if name == "mse+contrast":
        return dict(contrast=SlotContrast(negatives=33, temperature=0.1, weight=0.5, seed=77, distinct=False))
    raise ValueError(name)


def _state(t):
    return t.engine.read_scalars(), t.engine.params.clone(), t.engine.grads.clone()


def _same(a, b):
    return a[0] == b[0] and torch.equal(_bits(a[1]), _bits(b[1])) and torch.equal(_bits(a[2]), _bits(b[2]))


# ---- 3. what the data holds under an absent slot ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mse", "slot_cosine", "mse+contrast"])
@pytest.mark.parametrize("precision,io,S,z,B", [("bf16", 192, 3, 64, 40), ("f32", 24, 4, 8, 33)], ids=["bf16-s3e64", "f32-s4e6"])
def test_nan_under_absent_slots_changes_no_bit_of_a_step_or_an_evaluation(precision, io, S, z, B, name):
    res = []
    for poison in (False, True):
        p = _stack(io, S, z, B, seed=31, poison=poison)
        assert bool(np.isnan(p["data"]).any()) == poison
        t = _trainer(p, precision, **_settings(name))
        losses = []
        for s in range(2):
            t.train_batch(_idx(p, s), run=0)
            losses.append(t.engine.read_scalars()[3])
        train_sums = t.epoch_sums()
        y = t.eval_batch(_idx(p, 2), run=0, want_y=True)
        eval_sums = t.epoch_sums()
        res.append((_state(t), losses, train_sums, eval_sums, y))
    (sa, la, ta, ea, ya), (sb, lb, tb, eb, yb) = res
    assert _same(sa, sb) and la == lb and ta == tb and ea == eb and torch.equal(_bits(ya), _bits(yb))
    assert all(math.isfinite(v) for v in lb + list(tb) + list(eb)) and tb[0] > 0 and tb[1] > 0 and eb[0] > 0 and eb[1] > 0
    assert torch.isfinite(sb[1]).all() and torch.isfinite(sb[2]).all()


# ---- 4. off means off ----------------------------------------------------------------------------------------------------------------

def test_no_table_is_the_step_as_it_was_and_a_table_leaves_the_chain_io192_b40():
    from codae.tool import SlotPresence
    p = _stack(192, 3, 64, 40, seed=32)
    plain = _trainer(p, "bf16", with_presence=False)
    none = _trainer(p, "bf16", with_presence=False, presence=None)
    ones = _trainer(p, "bf16", with_presence=False, presence=SlotPresence(np.ones((N, 3), np.uint8)))
    assert plain.engine.step_path(40) == none.engine.step_path(40) == ones.engine.step_path(40) == "chain"
    for s in range(3):
        for t in (plain, none, ones):
            t.train_batch(_idx(p, s), run=0)
    assert _same(_state(plain), _state(none)) and _same(_state(plain), _state(ones))
    for name in ("adam_m", "adam_v"):
        assert torch.equal(_bits(getattr(plain.engine, name)), _bits(getattr(none.engine, name)))
    # a table moves the step off the chain kernel, None brings it back - with the bits of a trainer that never had one
    t = _trainer(p, "bf16")
    fresh = _trainer(p, "bf16", with_presence=False)
    assert t.engine.step_path(40) == "layers" and t.presence is not None
    t.set_presence(None)
    assert t.engine.step_path(40) == "chain" and t.presence is None
    for tr in (t, fresh):
        tr.train_batch(_idx(p, 0), run=0)
    assert _same(_state(t), _state(fresh))


def test_an_all_ones_table_gives_the_bits_of_the_unit_weight_standalone_loss_f32_io24_b33():
    """The table forced into the engine (SlotPresence would call it default): the PRES instantiations with nothing absent against
    the emphasised kernel with a unit column-weight vector, two fp32 steps and an evaluation."""
    from codae.tool import LossEmphasis
    p = _stack(24, 4, 8, 33, seed=33)
    unit = _trainer(p, "f32", with_presence=False, loss_emphasis=LossEmphasis(column_weight=[1.0] * 24))
    ones = _trainer(p, "f32", with_presence=False)
    table = torch.ones((N, 4), dtype=torch.uint8, device=DEV)
    ones.engine._set_presence_table(table)
    assert ones.engine.step_path(33) == "layers"
    for s in range(2):
        for t in (unit, ones):
            t.train_batch(_idx(p, s), run=0)
        assert unit.engine.read_scalars() == ones.engine.read_scalars(), s
    assert _same(_state(unit), _state(ones))
    ya, yb = (t.eval_batch(_idx(p, 2), run=0, want_y=True) for t in (unit, ones))
    assert torch.equal(_bits(ya), _bits(yb)) and unit.epoch_sums() == ones.epoch_sums()


# ---- 5. whole steps ------------------------------------------------------------------------------------------------------------------

def _oracle(p, name, quant=None):
    relu = [r for _, _, r in p["sched"]]
    kw = {}
    if name == "mse+emphasis+noise":
        kw = dict(alpha=ALPHA, beta=BETA, noise=("masking", dict(p=0.25), 20260))
    elif name == "huber":
        kw = dict(kind="huber", param=0.75)
    elif name == "slot_cosine":
        kw = dict(kind="slot_cosine", mse_weight=0.25)
    elif name == "mse+contrast":
        kw = dict(contrast=dict(K=33, tau=0.1, weight=0.5, seed=77), data=p["data0"])
    return PR.PresenceOracle(p["params"], relu, 1e-3, 1e-4, p["present"], S=p["S"], quant=quant, **kw)


@pytest.mark.parametrize("name", ["mse", "mse+emphasis+noise", "huber", "slot_cosine", "mse+contrast"])
def test_f32_steps_match_the_oracle_fed_the_references_dy_io24_s4_b33(name):
    """Three steps: the loss and gradient norm of every step, every gradient tensor of the first and the parameters after the
    third at rtol 1e-3 / atol 1e-5; epoch_sums() are the present-only sums."""
    p = _stack(24, 4, 8, 33, seed=34)
    t = _trainer(p, "f32", **_settings(name))
    eng = t.engine
    assert eng.step_path(33) == "layers"
    orc = _oracle(p, name)
    sq_sum = sqp_sum = plain_sum = 0.0
    for s in range(3):
        idx = p["order"][s]
        ro = orc.step(p["data0"][idx], idx, _fmask(p, idx))
        plain_sum += float(((p["data0"][idx].astype(np.float64) - ro["y"]) ** 2).sum())
        t.train_batch(_idx(p, s), run=0)
        _, _, gsq, loss = eng.read_scalars()
        print(s, "loss", loss, ro["loss"], "gnorm", math.sqrt(gsq), ro["grad_norm"])
        assert close(loss, ro["loss"]), (s, loss, ro["loss"])
        assert close(math.sqrt(gsq), ro["grad_norm"]), (s, math.sqrt(gsq), ro["grad_norm"])
        sq_sum += ro["sq_full"]; sqp_sum += ro["sq_partial"]
        if s == 0:
            for l, (gw, gb) in enumerate(orc.last_grads):
                assert close(eng.weight_grad(l).cpu().numpy(), gw), ("dW", l, max_err(eng.weight_grad(l).cpu().numpy(), gw))
                assert close(eng.bias_grad(l).cpu().numpy(), gb), ("db", l, max_err(eng.bias_grad(l).cpu().numpy(), gb))
    for l, (w, b) in enumerate(orc.params):
        assert close(eng.weight(l).cpu().numpy(), w), ("W", l, max_err(eng.weight(l).cpu().numpy(), w))
        assert close(eng.bias(l).cpu().numpy(), b), ("b", l, max_err(eng.bias(l).cpu().numpy(), b))
    sq, sqp = t.epoch_sums()
    print("epoch sums", sq, sq_sum, sqp, sqp_sum)
    assert close(sq, sq_sum) and close(sqp, sqp_sum), (sq, sq_sum, sqp, sqp_sum)
    assert sq_sum < 0.99 * plain_sum                                  # ... and not the sums over every element of the same rows
    # evaluation: the present-only sums of the reference's forward
    idx = p["order"][3]
    want = PR.eval_sums(orc.params, [r for _, _, r in p["sched"]], p["data0"][idx], idx, _fmask(p, idx), p["present"])
    y = t.eval_batch(_idx(p, 3), run=0, want_y=True)
    got = t.epoch_sums()
    assert close(got[0], want[0]) and close(got[1], want[1]), (got, want[:2])
    assert close(y.cpu().numpy(), want[2])


def _rel_l2(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("name", ["mse", "mse+emphasis+noise", "huber"])
def test_bf16_first_step_gradients_match_the_bf16_rounded_oracle_io192_s3_b40(name):
    from oracle import dae_oracle as O
    p = _stack(192, 3, 64, 40, seed=35)
    t = _trainer(p, "bf16", **_settings(name))
    eng = t.engine
    assert eng.precision == 1 and eng.step_path(40) == "layers"
    orc = _oracle(p, name, quant=O.bf16_round)
    idx = p["order"][0]
    ro = orc.step(p["data0"][idx], idx, _fmask(p, idx))
    t.train_batch(_idx(p, 0), run=0)
    sq, sqp, gsq, loss = eng.read_scalars()
    print("loss", loss, ro["loss"], "gnorm", math.sqrt(gsq), ro["grad_norm"], "sums", sq, ro["sq_full"], sqp, ro["sq_partial"])
    for l, (gw, gb) in enumerate(orc.last_grads):
        ew, eb = _rel_l2(eng.weight_grad(l).cpu().numpy(), gw), _rel_l2(eng.bias_grad(l).cpu().numpy(), gb)
        print("layer", l, "dW", ew, "db", eb)
        assert ew <= 2e-3, ("dW", l, ew)
        assert eb <= 2e-3, ("db", l, eb)


# ---- 6. graph replay -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mse", "huber", "slot_cosine", "mse+contrast"])
def test_graph_replay_with_a_table_gives_the_bits_of_plain_steps_io192_b40(name):
    """Three replayed steps = three plain steps; swapping the table for another one re-captures (the pointer is in the graph key)."""
    from codae.tool import SlotPresence
    p = _stack(192, 3, 64, 40, seed=36)
    other = SlotPresence(PR.make_table(N, 3, seed=99))
    out = []
    for graph in (False, True):
        t = _trainer(p, "bf16", use_graph=graph, **_settings(name))
        for s in range(3):
            t.train_batch(_idx(p, s), run=0)
        mid = _state(t)
        caps = t.engine.graph_captures()
        t.set_presence(other)
        t.train_batch(_idx(p, 3), run=0)
        out.append((mid, _state(t), caps, t.engine.graph_captures()))
    assert _same(out[0][0], out[1][0]) and _same(out[0][1], out[1][1])
    assert out[1][2] == 1 and out[1][3] == 2
    assert not _same(out[0][0], out[0][1])


# ---- 7. complete() ---------------------------------------------------------------------------------------------------------------------

def test_complete_ranks_only_rows_that_have_the_slot_f32_io24_s4():
    from codae.tool import ComplementRetriever, SlotPresence
    from codae.train import _ResidentInventory
    p = _stack(24, 4, 8, 33, seed=37)
    present = p["present"].copy()
    present[:, 3] = 0                                                   # nobody has slot 3
    present[present.sum(axis=1) < 2, 0] = 1
    present[present.sum(axis=1) < 2, 1] = 1
    p = dict(p, present=present, data=np.where(np.repeat(present != 0, 6, axis=1), p["data0"], np.float32(0)))
    t = _trainer(p, "f32")
    slot, k = 1, 5
    has = np.flatnonzero(present[:, slot])
    lacks = np.flatnonzero(present[:, slot] == 0)
    q = np.concatenate([lacks[:6], has[:6]]).astype(np.int32)          # a query row that lacks the slot is the normal case
    idx, score = t.complete(q, slot, k)
    assert tuple(idx.shape) == (12, k) and (idx >= 0).all()
    assert present[idx.cpu().numpy(), slot].all()                       # only rows that have the slot
    # the same prediction through a retriever over the present rows
    S, E = 4, 6
    y = _complete_y(t, torch.tensor(q), slot)
    ret = ComplementRetriever(_ResidentInventory(t.data, S, E), t.device, candidates=[int(i) for i in has])
    want_idx, want_score = ret.topk(y, slot, k)
    assert torch.equal(idx, want_idx) and torch.equal(_bits(score), _bits(want_score))
    # a candidates= subset is intersected with the present rows
    sub = [int(i) for i in range(0, N, 2)]
    idx2, _ = t.complete(q, slot, k, candidates=sub)
    got = idx2.cpu().numpy()
    assert present[got[got >= 0], slot].all() and (got[got >= 0] % 2 == 0).all()
    # exclude_self: a row that has the slot never gets its own item back; without it, it does
    own = torch.tensor(has[:6].astype(np.int32))
    with_self, _ = t.complete(own, slot, k)
    without, _ = t.complete(own, slot, k, exclude_self=True)
    assert (without.cpu() != own.long()[:, None]).all()
    want_ex, _ = ret.topk(_complete_y(t, own, slot), slot, k, exclude=own.to(DEV))
    assert torch.equal(without, want_ex)
    assert with_self.shape == without.shape
    # a slot nobody has
    idx3, score3 = t.complete(q, 3, k)
    assert (idx3 == -1).all() and torch.isinf(score3).all() and (score3 < 0).all()


def _complete_y(t, rows, slot):
    qi = rows.to(DEV).to(torch.int32)
    mid = torch.full((int(qi.numel()),), slot, dtype=torch.int32, device=DEV)
    y = torch.empty((int(qi.numel()), int(t.data.shape[1])), dtype=torch.float32, device=DEV)
    sums = t.engine.scalars.clone()
    t.engine.eval_step(t.engine.make_batch(t.data, qi, mid, t.mask_table), y)
    t.engine.scalars.copy_(sums)
    return y


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------

def test_bad_tables_and_disagreeing_slots_are_refused_and_the_engine_stays_usable_io24_b33():
    from codae import hip
    from codae.hip import HipError
    from codae.tool import ReconstructionLoss, SlotContrast, SlotPresence
    p = _stack(24, 4, 8, 33, seed=38)
    t = _trainer(p, "f32")
    ref = _trainer(p, "f32")
    eng = t.engine
    good = eng._presence_table
    lib = hip.lib()
    for n_slots, word in ((5, "does not divide"), (0, "1 .. 128"), (129, "1 .. 128"), (-1, "1 .. 128")):
        assert lib.codae_set_slot_presence(eng._h, hip.ptr(good), N, n_slots) == -1
        assert word in lib.codae_last_error().decode(), (n_slots, lib.codae_last_error())
        with pytest.raises(HipError):
            eng._set_presence_table(good, n_slots=n_slots)
    assert lib.codae_set_slot_presence(eng._h, hip.ptr(good), 0, 4) == -1
    with pytest.raises(HipError):
        eng.set_slot_presence("table")
    with pytest.raises(HipError):
        t.set_presence(SlotPresence(PR.make_table(60, 4)))             # not the dataset's rows
    # slot_cosine / the contrast with other slots than the table: refused by whichever setter comes second
    with pytest.raises(HipError, match="presence"):
        eng.set_recon_loss(ReconstructionLoss("slot_cosine"), n_slots=2)
    with pytest.raises(HipError, match="presence"):
        eng.set_slot_contrast(SlotContrast(negatives=8), t.data, n_slots=2)
    assert eng.recon_loss is None and eng.slot_contrast is None
    u = _trainer(p, "f32", with_presence=False, criterion=ReconstructionLoss("slot_cosine"))
    u.n_slots = None
    u.engine.set_recon_loss(ReconstructionLoss("slot_cosine"), n_slots=2)
    with pytest.raises(HipError, match="slot_cosine"):
        u.engine.set_slot_presence(SlotPresence(p["present"]))
    assert u.engine.slot_presence is None and u.engine.step_path(33) == "layers"
    u.engine.set_recon_loss(None)
    u.engine.set_slot_contrast(SlotContrast(negatives=8), u.data, n_slots=2)
    with pytest.raises(HipError, match="contrast"):
        u.engine.set_slot_presence(SlotPresence(p["present"]))
    # the stand-alone launchers refuse a bad n_slots too and write nothing
    q = _problem(24, 4)
    d = q["dev"]
    rc, dy, colsum, parts = loss_call("emph", d["data"], d["y"], d["present"], 5, emph=(1.0, 1.0, None), row_idx=d["rows"])
    assert rc == -1 and (dy == FILL).all() and (parts == FILL).all()
    # the refused engine still steps, with the setting it had
    for tr in (t, ref):
        tr.train_batch(_idx(p, 0), run=0)
    assert _same(_state(t), _state(ref))
