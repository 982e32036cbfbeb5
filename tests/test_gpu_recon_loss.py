"""The training criterion on a real MI355X: the two criterion kernels (codae_recon_loss_fwd_bwd) against the float64 statement of
the definition (tests/recon_loss_ref.py), shard invariance of dY, the default left bit for bit as it was, whole steps against
the oracle fed the criterion's dY, and the step forms (graph replay, forward-only, evaluation, refusals).

Tolerances, against the float64 reference computed from the same fp32 inputs.

Element-wise kinds (as tests/test_gpu_emphasis.py derives them).  fp32 dY: rtol 1e-6, atol 0 - at most six fp32 roundings (x - y,
1 / beta, their product, the weight, weight * inv_n, the final product: 6 * 2^-24 = 3.6e-7); the two branches of SmoothL1 and Huber
meet with equal value and slope, so a |d| that falls on the other side of beta / delta in fp32 moves nothing; for L1 the test first
checks on the reference alone that no |d| is below 1e-6, so sign(d) is never in doubt.  bf16 dY: one bf16 ulp of the reference.
Column sums: 1e-5 sum |g| per column.  Each of the three sums: relative B io 2^-24, the worst case of any order of non-negative
fp32 terms.

slot_cosine.  A lane adds at most 4 ceil(E / 256) products by fma and the butterfly adds 6 levels, so every one of the three sums of
a pair carries at most E + 8 roundings relative to the sum of its terms' magnitudes; by Cauchy-Schwarz sum |x y| <= |x| |y|, so
  |d cos| <= (E + 8) 2^-24
and the two coefficients a = k / (nx ny), b = k cos / |y|^2 (k = W / (rows S)) inherit the relative error of the norms and the
absolute error of cos, which gives, with room for the divisions, the square roots and the last fma,
  |d dY_c| <= (E + 8) 2^-23 k (|x_c| / (nx ny) + |y_c| / |y|^2)  +  1e-6 |mse_weight 2 w (y_c - x_c) inv_n|
(bf16 dY: that, plus one bf16 ulp of the reference).  Column sums: the sum of the elements' bounds plus 1e-5 sum |g|.
parts[.][0] = mse_weight sum w d^2 + E sum W (1 - cos): E (E + 8) 2^-24 sum W for the cosines plus relative B io 2^-24 for the
additions (all terms are non-negative).  The bound on cos is absolute, so no tolerance here leans on 1 - cos not cancelling;
the fixture's |cos| is checked all the same (below 0.67 on problem(48) read in dataset order, the route the first case takes).

Whole steps: the project's rtol 1e-3 / atol 1e-5 in fp32, test_gpu_parity.py's 2e-3 relative L2 per gradient tensor of the first
step in bf16.
"""
import ctypes as C
import math

import numpy as np
import pytest

import emphasis_ref as ER
import recon_loss_ref as RR
from golden_util import close, max_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"

SEED = ER.SEED
NOISES = [("off", None), ("masking", dict(p=0.25)), ("salt_pepper", dict(p=0.1, lo=-0.75, hi=1.5)), ("gaussian", dict(sigma=0.3))]
ALPHA, BETA, SLOT_W = 3.0, 0.5, (0.5, 1.0, 2.0)
STEP = 5
S = 3
ELEM = [("l1", None), ("smooth_l1", 0.5), ("huber", 0.75)]
KIND_ID = dict(mse=0, l1=1, smooth_l1=2, huber=3, slot_cosine=4)


def _noise(kind, kw, seed=SEED):
    from codae.tool import InputNoise
    return None if kw is None else InputNoise(kind, seed=seed, **kw)


def _struct(kind, param=None, mse_weight=0.0, n_slots=0):
    from codae import hip
    return hip.ReconLoss(KIND_ID[kind] if isinstance(kind, str) else kind, 0.0 if param is None else param, mse_weight, n_slots)


def recon_loss(data, y, noise, step, loss, emph=None, row_idx=None, B=None, mask_id=None, table=None, mask_to_use=None, run=0,
               dy_bf16=False, dy_ld=None, inv_n=None, fill=7.0):
    """codae_recon_loss_fwd_bwd on device tensors -> (rc, dy [B, dy_ld] prefilled with `fill`, colsum_part [blocks, io], parts
    [blocks, 3]).  emph: None or (alpha, beta, col_weight tensor or None)."""
    from codae import hip
    io = int(data.shape[1])
    B = int(row_idx.numel()) if row_idx is not None else (int(y.shape[0]) if B is None else B)
    ld = io if dy_ld is None else dy_ld
    blocks = hip.lib().codae_recon_loss_blocks(B)
    assert blocks == (B + 31) // 32
    dy = torch.full((B, ld), fill, dtype=torch.bfloat16 if dy_bf16 else torch.float32, device=DEV)
    colsum = torch.full((blocks, io), fill, dtype=torch.float32, device=DEV)
    parts = torch.full((blocks, 3), fill, dtype=torch.float64, device=DEV)
    batch = hip.Batch(hip.ptr(data), hip.ptr(row_idx), hip.ptr(mask_id), hip.ptr(table), B, io, hip.ptr(mask_to_use),
                      0 if mask_to_use is None else int(mask_to_use.shape[1]), run)
    st = None if noise is None else noise.as_struct()
    em = None if emph is None else hip.Emphasis(emph[0], emph[1], hip.ptr(emph[2]))
    rc = hip.lib().codae_recon_loss_fwd_bwd(C.byref(batch), None if st is None else C.byref(st), step, None if em is None else C.byref(em),
                                            C.byref(loss), hip.ptr(y), hip.ptr(dy), int(dy_bf16), ld,
                                            (1.0 / (B * io)) if inv_n is None else inv_n, hip.ptr(colsum), hip.ptr(parts), hip.current_stream())
    torch.cuda.synchronize()
    return rc, dy, colsum, parts


def _bits(t):
    return t.view({torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}[t.dtype])


def _bf16_ulp(ref):
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.abs(ref)))
    return np.where(ref == 0, 0.0, 2.0 ** (e - 7))


_PROBLEMS = {}


def _problem(io):
    """emphasis_ref.problem(io) once per session, with its device tensors; never modified."""
    if io not in _PROBLEMS:
        p = ER.problem(io)
        p["cw"] = np.repeat(np.float32(SLOT_W), io // S)
        p["dev"] = {k: torch.tensor(p[k], device=DEV) for k in ("data", "y", "table", "rows", "mask_id", "mtu", "cw")}
        _PROBLEMS[io] = p
    return _PROBLEMS[io]


def _routes(p):
    """The mask routes of test_gpu_emphasis.py: (name, kwargs of recon_loss, x, dataset rows, keep)."""
    d, B, io = p["dev"], p["B"], p["io"]
    return [("mask_id", dict(row_idx=d["rows"], mask_id=d["mask_id"], table=d["table"]), p["data"][p["rows"]], p["rows"], p["table"][p["mask_id"]]),
            ("mask_to_use", dict(B=B, table=d["table"], mask_to_use=d["mtu"], run=2), p["data"][:B], np.arange(B), p["table"][p["mtu"][:B, 2]]),
            ("no-mask", dict(row_idx=d["rows"]), p["data"][p["rows"]], p["rows"], np.ones((B, io), np.uint8))]


def _check_sums(parts, ref, keep, B, io, crit_tol=0.0):
    sums = parts.cpu().numpy().sum(axis=0)
    masked = (np.asarray(keep) == 0).any()
    want = (ref["crit"], ref["sq"], ref["sqp"] if masked else 0.0)
    print("sums", sums, want)
    for i, (g, r) in enumerate(zip(sums, want)):
        assert abs(g - r) <= B * io * 2.0 ** -24 * r + (crit_tol if i == 0 else 0.0), (i, g, r)


# ---- 1. element-wise kinds at the kernel entry ---------------------------------------------------------------------------------

def _check_elementwise(out, ref, keep, B, io, dy_bf16, fill=7.0):
    rc, dy, colsum, parts = out
    assert rc == 0
    got = dy[:, :io].float().cpu().numpy().astype(np.float64)
    if dy_bf16:
        err = np.abs(got - ref["dy"])
        assert (err <= _bf16_ulp(ref["dy"])).all(), float((err / np.maximum(_bf16_ulp(ref["dy"]), 1e-300)).max())
    else:
        np.testing.assert_allclose(got, ref["dy"], rtol=1e-6, atol=0)
    assert (dy[:, io:].float() == fill).all()                                   # pad columns stay as found
    cs = colsum.cpu().numpy().astype(np.float64).sum(axis=0)
    assert (np.abs(cs - ref["colsum"]) <= 1e-5 * ref["colsum_abs"]).all(), float(np.abs(cs - ref["colsum"]).max())
    _check_sums(parts, ref, keep, B, io)


@pytest.mark.parametrize("emph_on", [False, True], ids=["plain", "emphasis"])
@pytest.mark.parametrize("kind,kw", NOISES, ids=[k for k, _ in NOISES])
@pytest.mark.parametrize("io,dy_bf16,pad", [(48, False, 0), (48, False, 16), (48, True, 0), (48, True, 16), (33, False, 0), (33, False, 7),
                                            (33, True, 0), (33, True, 7)],
                         ids=["io48-f32", "io48-f32-ld64", "io48-bf16", "io48-bf16-ld64", "scalar-io33-f32", "scalar-io33-f32-ld40",
                              "scalar-io33-bf16", "scalar-io33-bf16-ld40"])
def test_elementwise_kinds_match_the_definition_b33(io, dy_bf16, pad, kind, kw, emph_on):
    """L1, SmoothL1(0.5), Huber(0.75) on 33 batch rows of 120 (two blocks, the second with one live row), over the mask routes;
    emphasis (3, 0.5, slot weights 0.5 / 1 / 2) on and off.  The same call twice gives the same bits."""
    p = _problem(io)
    noise, noise_ref = _noise(kind, kw), None if kw is None else (kind, kw, SEED)
    B = p["B"]
    emph = (ALPHA, BETA, p["dev"]["cw"]) if emph_on else None
    for lk, param in ELEM:
        crits = []
        for name, route, x, rows, keep in _routes(p):
            w = ER.weights(ER.corrupted(keep, rows, STEP, noise_ref), ALPHA, BETA, p["cw"]) if emph_on else None
            ref = RR.loss_terms(lk, x, p["y"], keep, w, np.float32(1.0 / (B * io)), param=param)
            if lk == "l1":
                dmin = np.abs(x.astype(np.float64) - p["y"]).min()
                assert dmin > 1e-6, dmin                                        # sign(d) is never in doubt (reference alone)
            out = recon_loss(p["dev"]["data"], p["dev"]["y"], noise, STEP, _struct(lk, param), emph=emph, dy_bf16=dy_bf16,
                             dy_ld=io + pad if pad else None, **route)
            _check_elementwise(out, ref, keep, B, io, dy_bf16)
            crits.append(ref)
            if name == "mask_id":
                again = recon_loss(p["dev"]["data"], p["dev"]["y"], noise, STEP, _struct(lk, param), emph=emph, dy_bf16=dy_bf16,
                                   dy_ld=io + pad if pad else None, **route)
                for a, b in zip(out[1:], again[1:]):
                    assert torch.equal(_bits(a), _bits(b))
        # not vacuous: the criterion's sum is far from the squared-error sum under the same weights, and emphasis moves it
        x0, keep0 = p["data"][p["rows"]], p["table"][p["mask_id"]]
        w0 = ER.weights(ER.corrupted(keep0, p["rows"], STEP, noise_ref), ALPHA, BETA, p["cw"]) if emph_on else None
        mse = RR.loss_terms("mse", x0, p["y"], keep0, w0, 1.0)["crit"]
        assert abs(crits[0]["crit"] - mse) > 0.1 * mse
        plain = RR.loss_terms(lk, p["data"][p["rows"]], p["y"], np.ones((B, io)), None, 1.0, param=param)["crit"]
        assert (abs(crits[0]["crit"] - plain) > 0.1 * plain) == emph_on


# ---- 2. slot_cosine at the kernel entry ----------------------------------------------------------------------------------------

def _cosine_inputs(io, zero_y):
    """problem(io) with the target of dataset row rows[2] blank in slot 1 and (zero_y) the output of batch row 5 zero in slot 0."""
    p = _problem(io)
    E = io // S
    data = p["data"].copy()
    data[p["rows"][2], E:2 * E] = 0.0
    y = p["y"].copy()
    if zero_y:
        y[5, 0:E] = 0.0
    return p, data, y


def _check_cosine(out, ref, keep, B, io, E, dy_bf16, fill=7.0):
    rc, dy, colsum, parts = out
    assert rc == 0
    got = dy[:, :io].float().cpu().numpy().astype(np.float64)
    bound = (E + 8) * 2.0 ** -23 * ref["bound_scale"] + 1e-6 * ref["mse_part"]
    if dy_bf16:
        bound = bound + _bf16_ulp(ref["dy"])
    err = np.abs(got - ref["dy"])
    print("dy: worst error / bound %.3f" % float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    assert (dy[:, io:].float() == fill).all()
    cs = colsum.cpu().numpy().astype(np.float64).sum(axis=0)
    tol = ((E + 8) * 2.0 ** -23 * ref["bound_scale"] + 1e-6 * ref["mse_part"]).sum(axis=0) + 1e-5 * ref["colsum_abs"]
    assert (np.abs(cs - ref["colsum"]) <= tol).all(), float((np.abs(cs - ref["colsum"]) / tol).max())
    _check_sums(parts, ref, keep, B, io, crit_tol=E * (E + 8) * 2.0 ** -24 * float(ref["W"].sum()))


@pytest.mark.parametrize("mse_weight", [0.0, 0.25], ids=["cos", "cos+mse"])
@pytest.mark.parametrize("emph_on", [False, True], ids=["plain", "emphasis+masking"])
@pytest.mark.parametrize("io,dy_bf16,pad", [(48, False, 0), (48, True, 16), (48, False, 2), (33, False, 7), (33, True, 0), (792, False, 0),
                                            (792, True, 8)],
                         ids=["E16-f32", "E16-bf16-ld64", "E16-f32-ld50-scalar-stores", "scalar-E11-f32-ld40", "scalar-E11-bf16", "E264-f32",
                              "E264-bf16-ld800"])
def test_slot_cosine_matches_the_definition_b33(io, dy_bf16, pad, emph_on, mse_weight):
    """S = 3; E = 16 (16-B lanes), 11 (scalar, a ragged piece, slots that start inside a Philox group) and 264 (66 pieces: lanes 0
    and 1 take a second one); one target slot all zeros (gradient 0, term W) and - fp32 dY only - one output slot all zeros."""
    p, data, y = _cosine_inputs(io, zero_y=not dy_bf16)
    E, B = io // S, p["B"]
    data_t, y_t = torch.tensor(data, device=DEV), torch.tensor(y, device=DEV)
    noise, noise_ref = (_noise("masking", dict(p=0.25)), ("masking", dict(p=0.25), SEED)) if emph_on else (None, None)
    emph = (ALPHA, BETA, p["dev"]["cw"]) if emph_on else None
    loss = _struct("slot_cosine", None, mse_weight, S)
    for name, route, _, rows, keep in _routes(p):
        x = data[rows]
        w = ER.weights(ER.corrupted(keep, rows, STEP, noise_ref), ALPHA, BETA, p["cw"]) if emph_on else None
        ref = RR.loss_terms("slot_cosine", x, y, keep, w, np.float32(1.0 / (B * io)), mse_weight=mse_weight, S=S)
        if io == 48 and name == "mask_to_use":                                  # (dataset order: the issue's statement of the fixture)
            assert np.abs(ref["cos"]).max() < 0.67, np.abs(ref["cos"]).max()
        assert np.abs(ref["cos"]).max() < 0.85                                   # every route and shape: far from 1
        out = recon_loss(data_t, y_t, noise, STEP, loss, emph=emph, dy_bf16=dy_bf16, dy_ld=io + pad if pad else None, **route)
        _check_cosine(out, ref, keep, B, io, E, dy_bf16)
        got = out[1][:, :io].float().cpu().numpy()
        if name != "mask_to_use":                                               # (that route reads rows 0 .. B-1: rows[2] need not be among them)
            assert ref["cos"][2, 1] == 0.0 and (got[2, E:2 * E] == 0).all() == (mse_weight == 0.0)
            if mse_weight == 0.0:
                assert (ref["dy"][2, E:2 * E] == 0).all()
        if not dy_bf16:
            assert ref["nyr"][5, 0] == 0.0 and np.abs(ref["dy"][5, 0:E]).max() > 1e3      # the zero output slot: a = k / (nx eps)
        if name == "mask_id":
            again = recon_loss(data_t, y_t, noise, STEP, loss, emph=emph, dy_bf16=dy_bf16, dy_ld=io + pad if pad else None, **route)
            for a, b in zip(out[1:], again[1:]):
                assert torch.equal(_bits(a), _bits(b))
            if emph_on:                                                         # not vacuous: the weights move the cosine term
                plain = RR.loss_terms("slot_cosine", x, y, keep, None, np.float32(1.0 / (B * io)), mse_weight=mse_weight, S=S)
                assert abs(ref["crit"] - plain["crit"]) > 0.1 * plain["crit"]


@pytest.mark.parametrize("dy_bf16", [False, True], ids=["f32", "bf16"])
def test_slot_cosine_with_slots_that_split_a_16_byte_group_b33_io24_s4(dy_bf16):
    """S = 4, E = 6: the pairs are reduced element by element while dY is written 16 B at a time, and a group of four columns
    belongs to two slots."""
    p = ER.problem(24, S=4)
    B, io, E = p["B"], 24, 6
    dev = {k: torch.tensor(p[k], device=DEV) for k in ("data", "y", "table", "rows", "mask_id")}
    keep = p["table"][p["mask_id"]]
    noise, noise_ref = _noise("masking", dict(p=0.25)), ("masking", dict(p=0.25), SEED)
    w = ER.weights(ER.corrupted(keep, p["rows"], STEP, noise_ref), ALPHA, BETA)
    ref = RR.loss_terms("slot_cosine", p["data"][p["rows"]], p["y"], keep, w, np.float32(1.0 / (B * io)), mse_weight=0.25, S=4)
    out = recon_loss(dev["data"], dev["y"], noise, STEP, _struct("slot_cosine", None, 0.25, 4), emph=(ALPHA, BETA, None), dy_bf16=dy_bf16,
                     row_idx=dev["rows"], mask_id=dev["mask_id"], table=dev["table"])
    _check_cosine(out, ref, keep, B, io, E, dy_bf16)


def test_zero_target_slot_contributes_its_weight_b33_io48():
    """Every target zero: cos = 0 everywhere, so L = sum W / (rows S) exactly and dY = 0."""
    p = _problem(48)
    B, io = p["B"], 48
    data = torch.zeros_like(p["dev"]["data"])
    rc, dy, colsum, parts = recon_loss(data, p["dev"]["y"], None, STEP, _struct("slot_cosine", None, 0.0, S), emph=(ALPHA, BETA, p["dev"]["cw"]),
                                       row_idx=p["dev"]["rows"], mask_id=p["dev"]["mask_id"], table=p["dev"]["table"])
    assert rc == 0 and (dy == 0).all() and (colsum == 0).all()
    keep = p["table"][p["mask_id"]]
    W = ER.weights(keep == 0, ALPHA, BETA, p["cw"]).reshape(B, S, io // S).mean(-1)
    assert float(parts[:, 0].sum()) == (io // S) * float(W.sum())            # (weights 0.25 .. 6: every sum is exact in fp32)


# ---- 3. shard invariance ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("io,dy_bf16", [(48, False), (48, True), (33, False), (33, True), (792, True)],
                         ids=["io48-f32", "io48-bf16", "scalar-io33-f32", "scalar-io33-bf16", "E264-bf16"])
def test_a_shards_dy_rows_are_the_bits_of_the_full_batch_b33(io, dy_bf16):
    """Rows 0 .. 16 and 17 .. 32 as two calls with the full batch's inv_n: dY bit for bit, for every kind, with emphasis and
    MASKING noise on; the summed criterion agrees to the sum bound."""
    p = _problem(io)
    d, B, E = p["dev"], p["B"], io // S
    noise = _noise("masking", dict(p=0.25))
    emph = (ALPHA, BETA, d["cw"])
    inv_n = 1.0 / (B * io)
    for loss in [_struct(k, prm) for k, prm in ELEM] + [_struct("slot_cosine", None, 0.0, S), _struct("slot_cosine", None, 0.25, S)]:
        common = dict(emph=emph, table=d["table"], dy_bf16=dy_bf16, inv_n=inv_n)
        full = recon_loss(d["data"], d["y"], noise, STEP, loss, row_idx=d["rows"], mask_id=d["mask_id"], **common)
        crit = 0.0
        for lo, hi in ((0, 17), (17, 33)):
            part = recon_loss(d["data"], d["y"][lo:hi], noise, STEP, loss, row_idx=d["rows"][lo:hi], mask_id=d["mask_id"][lo:hi], **common)
            assert part[0] == 0 and full[0] == 0
            assert torch.equal(_bits(part[1]), _bits(full[1][lo:hi])), (loss.kind, lo)
            crit += float(part[3][:, 0].sum())
        want = float(full[3][:, 0].sum())
        tol = B * io * 2.0 ** -24 * want + (E * (E + 8) * 2.0 ** -24 * 6.0 * B * S if loss.kind == 4 else 0.0)      # (W <= alpha * 2 = 6)
        assert abs(crit - want) <= tol, (loss.kind, crit, want)
        assert crit > 0


# ---- engines ---------------------------------------------------------------------------------------------------------------

def _stack(io, z, B, seed, N=120):
    """1 + 1 layers (io -> z -> io), S = 3 one-slot masks, one mask run (test_gpu_emphasis.py's stack)."""
    from oracle import dae_oracle as O
    rng = np.random.default_rng(seed)
    E = io // 3
    data = rng.random((N, io), dtype=np.float32)
    sched = [(io, z, True), (z, io, False)]
    params = O.init_params(sched, rng)
    bm, nmr, _ = O.corrupter_tables([{"size": E, "position": s * E} for s in range(3)], 1)
    mtu = rng.integers(0, 3, (N, 1)).astype(np.int32)
    order = [rng.permutation(N)[:B].astype(np.int32) for _ in range(4)]
    return dict(io=io, data=data, sched=sched, params=params, bm=bm, nmr=nmr, mtu=mtu, order=order, B=B)


def _trainer(p, precision, **kw):
    from codae.train import HipEmbeddingTrainer
    t = HipEmbeddingTrainer(p["sched"], torch.tensor(p["data"]), torch.tensor(p["bm"]).to(torch.uint8), torch.tensor(p["mtu"]), 1e-3,
                            1e-4, 1.0, max_batch=p["B"], precision=precision, device=DEV, **kw)
    t.load_params(p["params"])
    return t


def _idx(p, s):
    return torch.tensor(p["order"][s], dtype=torch.int32, device=DEV)


def _emphasis(alpha=ALPHA):
    from codae.tool import LossEmphasis
    return LossEmphasis(alpha, BETA, slot_weight=SLOT_W)


def _masking(seed=20260):
    from codae.tool import InputNoise
    return InputNoise("masking", p=0.25, seed=seed)


def _crit(name):
    from codae.tool import ReconstructionLoss
    return {"l1": lambda: ReconstructionLoss("l1"), "smooth_l1": lambda: ReconstructionLoss("smooth_l1", beta=0.5),
            "huber": lambda: ReconstructionLoss("huber", delta=0.75), "slot_cosine": lambda: ReconstructionLoss("slot_cosine"),
            "slot_cosine+mse": lambda: ReconstructionLoss("slot_cosine", mse_weight=0.25), "mse": lambda: ReconstructionLoss()}[name]()


def _oracle(p, name, emph, noise, quant=None):
    io = p["io"]
    kind = name.split("+")[0]
    return RR.CriterionOracle(p["params"], [r for _, _, r in p["sched"]], 1e-3, 1e-4, kind, param={"smooth_l1": 0.5, "huber": 0.75}.get(kind),
                              mse_weight=0.25 if name.endswith("+mse") else 0.0, S=3, alpha=ALPHA if emph else 1.0, beta=BETA if emph else 1.0,
                              col_weight=np.repeat(np.float32(SLOT_W), io // 3) if emph else None,
                              noise=None if noise is None else ("masking", dict(p=noise.p), noise.seed), quant=quant)


def _fmask(p, idx, run=0):
    from oracle import dae_oracle as O
    return O.get_masks(p["bm"], p["nmr"], p["mtu"], 1, idx, run)[1]


def _state(t):
    return t.engine.read_scalars(), t.engine.params.clone(), t.engine.grads.clone()


def _same(a, b):
    return a[0] == b[0] and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))


# ---- 4. the default is untouched ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("emph_on", [False, True], ids=["plain", "emphasis"])
@pytest.mark.parametrize("precision,io,z,B", [("bf16", 192, 64, 40), ("f32", 24, 8, 33)], ids=["bf16-io192-b40", "f32-io24-b33"])
def test_default_criterion_leaves_the_step_as_it_was(precision, io, z, B, emph_on):
    """ReconstructionLoss(), criterion=None, and a criterion set and cleared again: the bits of a trainer built without the argument
    after three steps, on the path it took before (the chain kernel for the narrow bf16 stack without emphasis)."""
    p = _stack(io, z, B, seed=31)
    kw = dict(loss_emphasis=_emphasis()) if emph_on else {}
    plain = _trainer(p, precision, **kw)
    dflt = _trainer(p, precision, criterion=_crit("mse"), **kw)
    none = _trainer(p, precision, criterion=None, **kw)
    back = _trainer(p, precision, criterion=_crit("slot_cosine+mse"), **kw)
    path = "chain" if precision == "bf16" and not emph_on else "layers"
    assert back.engine.step_path(B) == "layers" and not back.engine.recon_loss.is_default
    back.train_batch(_idx(p, 3), run=0)                         # one step under the criterion, then back to the start
    other = _state(back)
    back.load_params(p["params"])
    back.engine.adam_m.zero_(); back.engine.adam_v.zero_(); back.engine.step_count = 0
    back.engine.zero_metric_sums()
    back.set_criterion(None)
    assert back.engine.recon_loss is None
    for t in (plain, dflt, none, back):
        assert t.engine.step_path(B) == path
        t.engine.zero_metric_sums()
        for s in range(3):
            t.train_batch(_idx(p, s), run=0)
    ref = _state(plain)
    for t in (dflt, none, back):
        assert _same(_state(t), ref)
    assert other[0][3] != ref[0][3]                             # the criterion did change the step while it was set


# ---- 5. whole steps, fp32 engine ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,emph_on", [("l1", False), ("smooth_l1", False), ("huber", False), ("slot_cosine", False),
                                          ("slot_cosine+mse", True), ("l1", True)],
                         ids=["l1", "smooth_l1", "huber", "slot_cosine", "slot_cosine+mse+emphasis", "l1+emphasis"])
def test_f32_steps_match_the_oracle_with_the_criterions_dy_io24_z8_b33(name, emph_on):
    """Three steps (MASKING(0.25) input noise with emphasis): the loss and gradient norm of every step, every gradient tensor of the
    first and the parameters after the third at rtol 1e-3 / atol 1e-5; epoch_sums() are the unweighted squared-error sums."""
    p = _stack(24, 8, 33, seed=40)
    noise = _masking() if emph_on else None
    kw = dict(input_noise=noise, loss_emphasis=_emphasis()) if emph_on else {}
    t = _trainer(p, "f32", criterion=_crit(name), **kw)
    eng = t.engine
    assert eng.step_path(33) == "layers"
    orc = _oracle(p, name, emph_on, noise)
    sq_sum = sqp_sum = 0.0
    for s in range(3):
        idx = p["order"][s]
        ro = orc.step(p["data"][idx], idx, _fmask(p, idx))
        if name.startswith("l1"):                               # the engine's y and the oracle's agree to 1e-6: sign(d) is not in doubt
            assert ro["min_abs_d"] > 1e-5, ro["min_abs_d"]
        # (oracle alone) no row's hidden units are all dead: an output slot of exact zeros has the gradient k x / (nx eps), 1e8 times
        # the others', and the step would test nothing else
        assert ro["grad_norm"] < 100.0, ro["grad_norm"]
        t.train_batch(_idx(p, s), run=0)
        _, _, gsq, loss = eng.read_scalars()
        print(s, "loss", loss, ro["loss"], "mse", ro["mse"], "gnorm", math.sqrt(gsq), ro["grad_norm"])
        assert close(loss, ro["loss"]), (s, loss, ro["loss"])
        assert abs(ro["loss"] - ro["mse"]) > 0.1 * ro["loss"]
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


# ---- 6. whole step, bf16 engine ---------------------------------------------------------------------------------------------------------

def _rel_l2(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("name", ["l1", "huber", "slot_cosine"])
def test_bf16_first_step_gradients_match_the_bf16_rounded_oracle_io192_z64_b40(name):
    """Every gradient tensor of the first step at test_fused_bf16_matches_bf16_rounded_oracle's 2e-3 relative L2."""
    from oracle import dae_oracle as O
    p = _stack(192, 64, 40, seed=24)
    t = _trainer(p, "bf16", criterion=_crit(name))
    eng = t.engine
    assert eng.precision == 1 and eng.step_path(40) == "layers"
    orc = _oracle(p, name, False, None, quant=O.bf16_round)
    idx = p["order"][0]
    ro = orc.step(p["data"][idx], idx, _fmask(p, idx))
    if name == "l1":                                            # (the two y differ by the order of 64 fp32 additions: 4e-6 |y|)
        assert ro["min_abs_d"] > 1e-5, ro["min_abs_d"]
    t.train_batch(_idx(p, 0), run=0)
    sq, sqp, gsq, loss = eng.read_scalars()
    print("loss", loss, ro["loss"], "gnorm", math.sqrt(gsq), ro["grad_norm"], "sums", sq, ro["sq_full"], sqp, ro["sq_partial"], "min |d|", ro["min_abs_d"])
    for l, (gw, gb) in enumerate(orc.last_grads):
        ew, eb = _rel_l2(eng.weight_grad(l).cpu().numpy(), gw), _rel_l2(eng.bias_grad(l).cpu().numpy(), gb)
        print("layer", l, "dW", ew, "db", eb)
        assert ew <= 2e-3, ("dW", l, ew)
        assert eb <= 2e-3, ("db", l, eb)


# ---- 7. step forms, on the io = 192 stack -----------------------------------------------------------------------------------------------

def test_graph_replay_with_a_criterion_gives_the_bits_of_plain_steps_io192_b40():
    """Three replayed steps = three plain steps (emphasis and MASKING noise on: the step index comes from device memory); a
    change of criterion between replays re-captures."""
    p = _stack(192, 64, 40, seed=26)
    out = []
    for graph in (False, True):
        t = _trainer(p, "bf16", input_noise=_masking(), loss_emphasis=_emphasis(), criterion=_crit("slot_cosine+mse"), use_graph=graph)
        for s in range(3):
            t.train_batch(_idx(p, s), run=0)
        out.append(_state(t))
    assert _same(out[0], out[1]), (out[0][0], out[1][0])
    out = []
    for graph in (False, True):
        t = _trainer(p, "bf16", use_graph=graph)
        losses = []
        for s, name in enumerate(("slot_cosine", "huber", None, "slot_cosine+mse", "l1")):
            t.set_criterion(None if name is None else _crit(name))
            t.train_batch(_idx(p, s % 4), run=0)
            losses.append(t.engine.read_scalars()[3])
        out.append((_state(t), losses))
    assert out[0][1] == out[1][1], (out[0][1], out[1][1])
    assert _same(out[0][0], out[1][0])
    assert len(set(out[0][1])) == 5


@pytest.mark.parametrize("name", ["l1", "slot_cosine+mse"])
def test_step_forward_loss_with_a_hyper_takes_the_criterion_io192_b40(name):
    """The torch.distributed data-parallel path drives codae_step_forward_loss / _backward / _update itself; the global batch's rows
    scale the loss and nothing renormalises it: with global_rows = 80 the 40 rows give half the loss."""
    p = _stack(192, 64, 40, seed=28)
    a, b = (_trainer(p, "bf16", criterion=_crit(name)) for _ in range(2))
    c = _trainer(p, "bf16")
    a.train_batch(_idx(p, 0), run=0)
    losses = []
    for tr in (b, c):
        eng = tr.engine
        eng.step_forward_loss(tr._batch(_idx(p, 0), 0), eng.hyper(1e-3, 1e-4, 1.0, global_rows=40, step=1))
        losses.append(eng.read_scalars()[3])
    assert losses[0] == a.engine.read_scalars()[3] and losses[1] != losses[0]
    dy40 = b.engine.dacts.clone()
    b.engine.step_forward_loss(b._batch(_idx(p, 0), 0), b.engine.hyper(1e-3, 1e-4, 1.0, global_rows=80, step=1))
    assert b.engine.read_scalars()[3] == losses[0] / 2
    assert not torch.equal(b.engine.dacts, dy40)


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_evaluation_and_completion_never_see_the_criterion_io192_b40(precision):
    p = _stack(192, 64, 40, seed=27)
    plain = _trainer(p, precision)
    crit = _trainer(p, precision, criterion=_crit("slot_cosine"))
    res = []
    for tr in (plain, crit):
        tr.engine.zero_metric_sums()
        y = tr.eval_batch(_idx(p, 1), run=0, want_y=True)
        _, _, _, loss = tr.engine.read_scalars()
        sums = tr.epoch_sums(reset=False)
        top = tr.complete(_idx(p, 1)[:20], 1, 5)
        res.append((y, sums, loss, top))
    assert torch.equal(res[0][0].view(torch.int32), res[1][0].view(torch.int32))
    assert res[0][1] == res[1][1] and res[0][2] == res[1][2]
    assert torch.equal(res[0][3][0], res[1][3][0]) and torch.equal(res[0][3][1], res[1][3][1])
    for tr in (plain, crit):                                    # ... while the training step of the same engine does
        tr.train_batch(_idx(p, 1), run=0)
    assert plain.engine.read_scalars()[3] != crit.engine.read_scalars()[3]


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------------

BAD = [((9, 0.0, 0.0, 0), -1, "unknown kind"), ((-1, 0.0, 0.0, 0), -1, "unknown kind"), ((2, 0.0, 0.0, 0), -1, "beta"),
       ((2, float("nan"), 0.0, 0), -1, "beta"), ((3, -1.0, 0.0, 0), -1, "delta"), ((3, float("inf"), 0.0, 0), -1, "delta"),
       ((4, 0.0, -0.5, 3), -1, "mse_weight"), ((4, 0.0, float("nan"), 3), -1, "mse_weight"), ((1, 0.0, 0.25, 0), -1, "mse_weight"),
       ((0, 0.0, 0.25, 0), -1, "mse_weight"), ((4, 0.0, 0.0, 0), -1, "n_slots"), ((4, 0.0, 0.0, 5), -1, "n_slots"),
       ((4, 0.0, 0.0, 129), -3, "128")]


@pytest.mark.parametrize("fields,code,word", BAD, ids=["kind-9", "kind-neg", "beta-0", "beta-nan", "delta-neg", "delta-inf", "mse-neg", "mse-nan",
                                                       "mse-with-l1", "mse-with-mse", "slots-0", "slots-5", "slots-129"])
def test_a_bad_criterion_is_refused_and_launches_nothing(fields, code, word):
    """io = 258 (divisible by 3 and by 129, not by 5) at the kernel entry: the prefilled outputs stay; the engine keeps its setting."""
    from codae import hip
    rng = np.random.default_rng(5)
    data = torch.tensor(rng.standard_normal((8, 258)).astype(np.float32), device=DEV)
    y = torch.tensor(rng.standard_normal((8, 258)).astype(np.float32), device=DEV)
    bad = hip.ReconLoss(*fields)
    rc, dy, colsum, parts = recon_loss(data, y, None, 1, bad)
    assert rc == code and word in hip.lib().codae_last_error().decode(), hip.lib().codae_last_error()
    assert (dy == 7.0).all() and (colsum == 7.0).all() and (parts == 7.0).all()
    if fields[0] == 0:
        return                                                  # (kind MSE with mse_weight 0 is a valid setting: off)
    p = _stack(24, 8, 33, seed=33)
    good = _crit("huber")
    t, ref = _trainer(p, "f32", criterion=good), _trainer(p, "f32", criterion=good)
    bad24 = hip.ReconLoss(*fields)
    rc = hip.lib().codae_set_recon_loss(t.engine._h, C.byref(bad24))
    if fields == (4, 0.0, 0.0, 129):
        assert rc == -1                                         # (129 does not divide 24: refused as invalid before the slot limit)
    else:
        assert rc == code and word in hip.lib().codae_last_error().decode()
    with pytest.raises(hip.HipError):
        t.engine._set_recon_struct(bad24)
    assert t.engine.recon_loss is good
    for tr in (t, ref):
        tr.train_batch(_idx(p, 0), run=0)
    assert _same(_state(t), _state(ref))


def test_python_side_refusals_io24():
    from codae import hip
    from codae.train import HipEmbeddingTrainer
    p = _stack(24, 8, 33, seed=34)
    t = _trainer(p, "f32")
    with pytest.raises(hip.HipError):
        t.engine.set_recon_loss("l1")
    with pytest.raises(hip.HipError, match="n_slots"):
        t.engine.set_recon_loss(_crit("slot_cosine"))
    bare = HipEmbeddingTrainer(p["sched"], torch.tensor(p["data"]), None, None, 1e-3, 1e-4, 1.0, max_batch=33, precision="f32", device=DEV)
    with pytest.raises(hip.HipError, match="n_slots"):
        bare.set_criterion(_crit("slot_cosine"))
    with pytest.raises(hip.HipError, match="n_slots"):
        HipEmbeddingTrainer(p["sched"], torch.tensor(p["data"]), None, None, 1e-3, 1e-4, 1.0, max_batch=33, precision="f32", device=DEV,
                            criterion=_crit("slot_cosine"))
    bare.set_criterion(_crit("l1"))                             # the element-wise kinds need no slots
    with_slots = HipEmbeddingTrainer(p["sched"], torch.tensor(p["data"]), None, None, 1e-3, 1e-4, 1.0, max_batch=33, precision="f32", device=DEV,
                                     n_slots=3, criterion=_crit("slot_cosine"))
    assert with_slots.engine.recon_loss.kind == "slot_cosine"


@pytest.mark.parametrize("alpha", [ALPHA, 0.0], ids=["alpha3", "alpha0"])
def test_a_nan_output_slot_gives_nan_there_and_in_the_loss_b33_io48(alpha):
    """One NaN in slot 1 of batch row 3 (blanked there: its weight is alpha, 0 in the second case): that slot's dY is NaN, every
    other element finite, the block's criterion sum NaN, the other block's finite."""
    p = _problem(48)
    d, E = p["dev"], 16
    mask_id = p["mask_id"].copy()
    mask_id[3] = 1
    y = p["y"].copy()
    y[3, E + 2] = np.nan
    rc, dy, colsum, parts = recon_loss(d["data"], torch.tensor(y, device=DEV), None, STEP, _struct("slot_cosine", None, 0.0, S),
                                       emph=(alpha, 1.0, None), row_idx=d["rows"], mask_id=torch.tensor(mask_id, device=DEV), table=d["table"])
    assert rc == 0
    bad = torch.isnan(dy).cpu().numpy()
    want = np.zeros_like(bad)
    want[3, E:2 * E] = True
    assert np.array_equal(bad, want)
    assert torch.isfinite(dy[~torch.tensor(want, device=DEV)]).all()
    assert math.isnan(float(parts[0, 0])) and math.isfinite(float(parts[1, 0]))
    assert torch.isnan(colsum[0, E:2 * E]).all() and torch.isfinite(colsum[0, :E]).all() and torch.isfinite(colsum[1]).all()


@pytest.mark.parametrize("name", ["l1", "slot_cosine"])
def test_a_nan_output_makes_last_loss_nan_io24_b33(name):
    """A NaN bias of the last layer makes column 9 of every output row NaN: CODAE_S_LAST_LOSS is NaN, never finite."""
    p = _stack(24, 8, 33, seed=35)
    t = _trainer(p, "f32", criterion=_crit(name))
    t.engine.bias(1)[9] = float("nan")
    eng = t.engine
    eng.step_forward_loss(t._batch(_idx(p, 0), 0), eng.hyper(1e-3, 1e-4, 1.0, global_rows=33, step=1))
    assert math.isnan(eng.read_scalars()[3])
