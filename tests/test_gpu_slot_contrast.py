"""The slot contrast on a real MI355X: the prepare + contrast launches (codae_slot_contrast_prepare / _fwd_bwd) against the float64
statement of the definition (tests/contrast_ref.py), their properties (same bits twice, shard invariance, NaN / Inf, zero target,
all candidates left out), whole steps against the oracle fed the reference's dY, and the step forms.

Fixture.  emphasis_ref.problem(io): N = 120 dataset rows, B = 33 batch rows (two 32-row blocks, the second with one live row),
S = 3, with dataset rows 100 .. 104 repeating the slot-0 and slot-2 items of the first five batch rows (so `item_id` leaves out
candidates the row rule keeps).  Before any GPU assert, on the reference alone and for every B = 33 route of every case: a pair
with a candidate left out, a pair with none left out, a row among its own candidates, no |x_s| or |y_s| below 1e-3.  The seed
of each (io, K) is the first from 0x5EED0000C0DA0001 under which this holds (tools/find_contrast_seeds.py; K = 1 draws only 3
rows).  The B = 1
sub-case has three pairs; its row is the first candidate of slot 0, so one pair has its candidate left out - the other conditions
need more than one row.

Tolerances, against the float64 reference computed from the same fp32 inputs.  u = 2^-24, k = scale W = weight W / (rows S).

fp32 form.  v_mfma_f32_16x16x4_f32 is an exact fmaf chain, so a logit's product carries E roundings of terms whose magnitudes sum
to at most |c^| |y^| = 1 (Cauchy-Schwarz), each unit vector has the relative error of its norm - (E + 8) u / 2 from the fma chain
and the butterfly, as tests/test_gpu_recon_loss.py derives - plus the division's:
  |d cos| <= dcos = (2 E + 24) u.
A softmax weight p_k = exp(z_k - lse) sees a difference of two logits, 2 dcos / tau, and the roundings of the exponent's
arithmetic (z / tau, the running maximum's rescaling, log, the subtraction, exp2's argument), each relative u of a magnitude of at
most 2 / tau + ln(4097) < 2 / tau + 9, eight of them at most:
  |d p_k| / p_k <= eta = 2 dcos / tau + 8 (2 / tau + 9) u.
g = sum_kept p_k c_k^ - (1 - p_0) x^ adds K + 1 terms by fma (K u), each c_k^ with its own (E + 8) u / 2 + u, so with
bs_e = sum_kept p_k |c_k^_e| + (1 - p_0) |x^_e| (the reference returns it):  |d g_e| <= (eta + (K + E + 16) u) bs_e.
The projection takes g . y^ = sum p_k cos_k - (1 - p_0) cos_0 from the same logits: |d (g . y^)| <= (eta + (K + E + 16) u) |bs|_2,
and multiplies by y^_e.  Carried through 1 / (tau |y|) and k:
  |d dY_e| <= k / (tau |y|) (eta + (K + E + 16) u) (bs_e + |y^_e| |bs|_2)  +  4 u |k dl_e|  +  u |dY_e|
(the last two: 1 / |y|, 1 / tau, k and the fma into dY_in; the final rounding of the stored sum).
Column sums: the sum of the element bounds plus 1e-5 sum |g|.  Parts (sum W l per block): a pair's l is a logit difference, eta,
so eta sum W over the block's pairs, plus relative B S u for the additions.

bf16-operand form.  MEASURED on an MI355X over every case of test_kernel_matches_the_definition (one run, see BF16_MEASURED
below): the largest |dY - ref| / (k / (tau |y|)), after taking off one bf16 ulp of the reference for the stored value.  The test
asserts 4 x that value per element, and every case's own largest value against the 2e-2 above which it would be a bug.  Parts: both unit vectors are rounded to bf16 (2^-9 relative
each), so |d cos| <= 2^-8 and a pair's l moves by at most 2 * 2^-8 / tau.

Whole steps: the project's rtol 1e-3 / atol 1e-5 in fp32; bf16: relative L2 per gradient tensor, 2 x the measured 6.347e-3 (the
2e-3 used elsewhere does not hold with the term on: see BF16_STEP_L2).
"""
import ctypes as C
import math

import numpy as np
import pytest

import contrast_ref as CR
import emphasis_ref as ER
import recon_loss_ref as RR
from golden_util import close, max_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"

U = 2.0 ** -24
S = 3
STEP = 5
ALPHA, BETA, SLOT_W = 3.0, 0.5, (0.5, 1.0, 2.0)
NOISE_SEED = ER.SEED
FILL = 7.0
# largest normalised error of the bf16-operand form seen over all kernel-level cases in one run on an MI355X, and the bound asserted
BF16_MEASURED = 1.965e-2      # at E = 8, K = 5, tau = 0.02 with emphasis; 1.5e-2 and below everywhere else
BF16_BOUND = 4.0 * BF16_MEASURED
BF16_CEILING = 2e-2           # a normalised error above this is a bug, not a tolerance
# bf16 engine, relative L2 of every gradient tensor of the first step against the bf16-rounded oracle.  MEASURED on an MI355X:
# 6.347e-3 at worst with the MSE underneath (layer 0's bias gradient; 4.5e-3 .. 6.0e-3 on the other tensors), 3.870e-3 with
# slot_cosine - above the 2e-3 the project uses elsewhere, because the oracle's dY carries the term in float64 while the engine forms
# it from bf16 unit vectors and bf16 p_k (the kernel-level error above), and the term is 86 % of this loss.  Asserted: 2 x the
# largest value measured.
BF16_STEP_MEASURED = 6.347e-3
BF16_STEP_L2 = 2.0 * BF16_STEP_MEASURED

# (io, K) -> (tau, emphasis, item_id given, pool given, pad columns): every pair of the E and K edge values; every tau, both
# emphasis settings, both id rules and dy_ld > io appear.  The seeds satisfy the fixture conditions (module docstring).
CASES = {
    (24, 1): (0.1, False, False, False, 0), (24, 5): (0.02, True, True, False, 8), (24, 33): (0.5, False, True, False, 0),
    (24, 130): (0.1, True, False, False, 0),
    (48, 1): (0.5, True, True, False, 16), (48, 5): (0.1, False, False, True, 0), (48, 33): (0.02, True, False, False, 0),
    (48, 130): (0.5, False, True, False, 0),
    (120, 1): (0.02, False, True, False, 0), (120, 5): (0.5, True, False, False, 0), (120, 33): (0.1, False, True, True, 8),
    (120, 130): (0.02, True, True, False, 0),
    (216, 1): (0.1, True, False, False, 0), (216, 5): (0.02, False, True, False, 0), (216, 33): (0.5, True, True, False, 0),
    (216, 130): (0.1, False, False, False, 24),
    # the kernel's other builds: E = 136 (9 column tiles: the 32-tile build), E = 520 (33 tiles: two column ranges), E = 1024 (the limit)
    (408, 33): (0.1, True, True, False, 0), (1560, 5): (0.02, False, True, False, 8), (3072, 33): (0.5, False, False, False, 0),
}
SEEDS = {}       # (io, K) -> seed; filled below


def _bits(t):
    return t.view({torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}[t.dtype])


def _bf16_ulp(ref):
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.floor(np.log2(np.abs(ref)))
    return np.where((ref == 0) | ~np.isfinite(ref), 0.0, 2.0 ** (e - 7))


_PROBLEMS = {}
_HOST = {}


def _problem_host(io):
    """emphasis_ref.problem(io) with the duplicated items, its item ids, a candidate pool and a dY_in; numpy only, never modified."""
    if io not in _HOST:
        p = dict(ER.problem(io))
        E = io // S
        data = p["data"].copy()
        for i in range(5):
            data[100 + i, 0:E] = data[p["rows"][i], 0:E]
            data[100 + i, 2 * E:3 * E] = data[p["rows"][i], 2 * E:3 * E]
        p["data"] = data
        p["cw"] = np.repeat(np.float32(SLOT_W), E)
        p["ids"] = CR.item_ids(data, S).astype(np.int32)
        p["pool"] = np.arange(3, 120, 2).astype(np.int32)
        # dy_in: what a criterion would have left, of the gradient's magnitude
        p["dy_in"] = (np.random.default_rng(io).standard_normal((p["B"], io)) * 1e-2).astype(np.float32)
        _HOST[io] = p
    return _HOST[io]


def _problem(io):
    """_problem_host(io) with its device tensors, once per session."""
    if io not in _PROBLEMS:
        p = dict(_problem_host(io))
        p["dev"] = {k: torch.tensor(p[k], device=DEV) for k in ("data", "y", "table", "rows", "mask_id", "mtu", "cw", "ids", "pool", "dy_in")}
        _PROBLEMS[io] = p
    return _PROBLEMS[io]


def _routes(p):
    """The mask routes of test_gpu_recon_loss.py: (name, batch kwargs, dataset rows, keep)."""
    d, B, io = p["dev"], p["B"], p["io"]
    return [("mask_id", dict(row_idx=d["rows"], mask_id=d["mask_id"], table=d["table"]), p["rows"], p["table"][p["mask_id"]]),
            ("mask_to_use", dict(B=B, table=d["table"], mask_to_use=d["mtu"], run=2), np.arange(B), p["table"][p["mtu"][:B, 2]]),
            ("no-mask", dict(row_idx=d["rows"]), p["rows"], np.ones((B, io), np.uint8))]


GUARD_ROWS = 32      # rows behind the batch (a whole row block), and one spare colsum row and parts entry: never written


def contrast(data, y, dy_in, K, tau, weight, seed, step, scale, n_slots=S, row_idx=None, B=None, mask_id=None, table=None, mask_to_use=None,
             run=0, emph=None, noise=None, item_id=None, pool=None, bf16=False, dy_ld=None, ws=None, prepare=True):
    """prepare + codae_slot_contrast_fwd_bwd on device tensors -> (rc, dy [B, ld] (pad columns = FILL), colsum [blocks, io], parts
    [blocks]).  dy_in [B, io] fp32 is rounded to the stored type first.  dy is allocated with GUARD_ROWS more rows than the batch and
    colsum / parts with one more entry than there are blocks, all FILL: they are checked here, on every call, to be untouched (rows
    >= B are never written).  prepare=False: the contrast launcher alone (its own refusals), whatever ws holds."""
    from codae import hip
    lib = hip.lib()
    N, io = int(data.shape[0]), int(data.shape[1])
    B = int(row_idx.numel()) if row_idx is not None else (int(y.shape[0]) if B is None else B)
    ld = io if dy_ld is None else dy_ld
    width = max(ld, io)
    blocks = lib.codae_slot_contrast_blocks(B)
    assert blocks == (B + 31) // 32
    dt = torch.bfloat16 if bf16 else torch.float32
    dy_all = torch.full((B + GUARD_ROWS, width), FILL, dtype=dt, device=DEV)
    dy_all[:B, :io] = dy_in.to(dt)
    colsum_all = torch.full((blocks + 1, io), FILL, dtype=torch.float32, device=DEV)
    parts_all = torch.full((blocks + 1,), FILL, dtype=torch.float64, device=DEV)
    if ws is None:
        ws = torch.full((lib.codae_slot_contrast_ws_bytes(n_slots, K, io // n_slots, int(bf16)),), 0xFF, dtype=torch.uint8, device=DEV)
    st = hip.SlotContrast(n_slots, K, tau, weight, seed, N, 0 if pool is None else int(pool.numel()), int(ws.numel()), hip.ptr(pool),
                          hip.ptr(item_id), hip.ptr(ws))
    batch = hip.Batch(hip.ptr(data), hip.ptr(row_idx), hip.ptr(mask_id), hip.ptr(table), B, io, hip.ptr(mask_to_use),
                      0 if mask_to_use is None else int(mask_to_use.shape[1]), run)
    ns = None if noise is None else noise.as_struct()
    em = None if emph is None else hip.Emphasis(emph[0], emph[1], hip.ptr(emph[2]))
    rc = lib.codae_slot_contrast_prepare(hip.ptr(data), io, C.byref(st), step, int(bf16), hip.current_stream()) if prepare else 0
    if rc == 0:
        rc = lib.codae_slot_contrast_fwd_bwd(C.byref(batch), None if ns is None else C.byref(ns), step, None if em is None else C.byref(em),
                                             C.byref(st), hip.ptr(y), hip.ptr(dy_all), int(bf16), ld, scale, hip.ptr(colsum_all),
                                             hip.ptr(parts_all), hip.current_stream())
    torch.cuda.synchronize()
    assert (dy_all[B:].float() == FILL).all(), "rows >= B of dy were written"
    assert (colsum_all[blocks:] == FILL).all() and (parts_all[blocks:] == FILL).all(), "a part row past the last block was written"
    return rc, dy_all[:B], colsum_all[:blocks], parts_all[:blocks]


def _noise():
    from codae.tool import InputNoise
    return InputNoise("masking", p=0.25, seed=NOISE_SEED), ("masking", dict(p=0.25), NOISE_SEED)


def _ref(p, rows, keep, K, tau, scale, seed, emph_on, ids_on, pool_on, dy_in, y=None, data=None):
    data = p["data"] if data is None else data
    W = None
    if emph_on:
        w = ER.weights(ER.corrupted(keep, rows, STEP, _noise()[1]), ALPHA, BETA, p["cw"])
        W = w.reshape(len(rows), S, -1).mean(-1)
    return CR.terms(data, data[rows], p["y"] if y is None else y, rows, STEP, S, K, tau, scale, seed, W=W,
                    item_id=p["ids"] if ids_on else None, pool=p["pool"] if pool_on else None, dy_in=dy_in)


def fixture_ok(ref, rows, x, y):
    """The fixture conditions of the module docstring, on the reference alone."""
    left = ref["left_out"]                                  # [B, S, K]
    per_pair = left.any(axis=2)
    own = (ref["cand"][None, :, :] == np.asarray(rows)[:, None, None]).any(axis=(1, 2))
    E = x.shape[1] // S
    nx = np.linalg.norm(x.astype(np.float64).reshape(len(x), S, E), axis=-1)
    ny = np.linalg.norm(y.astype(np.float64).reshape(len(y), S, E), axis=-1)
    return bool(per_pair.any() and (~per_pair).any() and own.any() and nx.min() >= 1e-3 and ny.min() >= 1e-3)


SEEDS.update({
    (24, 1): 0x5EED0000C0DA0002,
    (24, 5): 0x5EED0000C0DA0002,
    (24, 33): 0x5EED0000C0DA0001,
    (24, 130): 0x5EED0000C0DA0001,
    (48, 1): 0x5EED0000C0DA0002,
    (48, 5): 0x5EED0000C0DA0002,
    (48, 33): 0x5EED0000C0DA0001,
    (48, 130): 0x5EED0000C0DA0001,
    (120, 1): 0x5EED0000C0DA0002,
    (120, 5): 0x5EED0000C0DA0002,
    (120, 33): 0x5EED0000C0DA0001,
    (120, 130): 0x5EED0000C0DA0001,
    (216, 1): 0x5EED0000C0DA0002,
    (216, 5): 0x5EED0000C0DA0002,
    (216, 33): 0x5EED0000C0DA0001,
    (216, 130): 0x5EED0000C0DA0001,
    (408, 33): 0x5EED0000C0DA0001,
    (1560, 5): 0x5EED0000C0DA0002,
    (3072, 33): 0x5EED0000C0DA0001,
})


def _seed(io, K):
    return SEEDS[(io, K)]


def _f32_bound(ref, E, K, tau, dy_in):
    dcos = (2 * E + 24) * U
    eta = 2 * dcos / tau + 8 * (2 / tau + 9) * U
    rel = eta + (K + E + 16) * U
    kk = np.repeat(ref["k"] / (tau * np.maximum(ref["ny"], 1e-300)), E, axis=1)
    return kk * rel * (ref["bs"] + ref["yh"] * np.repeat(ref["bsn"], E, axis=1)) + 4 * U * np.abs(ref["own"]) + U * np.abs(ref["dy"]), eta


def _check(out, ref, p, K, tau, bf16, pad, dy_in_used, B):
    rc, dy, colsum, parts = out
    io = p["io"]
    E = io // S
    assert rc == 0
    got = dy[:, :io].float().cpu().numpy().astype(np.float64)
    err = np.abs(got - ref["dy"])
    norm = np.repeat(ref["k"] / (tau * np.maximum(ref["ny"], 1e-300)), E, axis=1)
    if bf16:
        ulp = _bf16_ulp(ref["dy"])
        nerr = np.maximum(err - ulp, 0.0) / np.maximum(norm, 1e-300)
        worst = float(nerr[norm > 0].max()) if (norm > 0).any() else 0.0
        print("bf16 operands: worst normalised error %.3e" % worst)
        assert worst <= BF16_CEILING, worst
        bound = BF16_BOUND * norm + ulp
        dl_tol = 2 * 2.0 ** -8 / tau
    else:
        bound, dl_tol = _f32_bound(ref, E, K, tau, dy_in_used)
        print("f32 operands: worst error / bound %.3f" % float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    if pad:
        assert (dy[:, io:].float() == FILL).all()                               # pad columns stay as found
    cs = colsum.cpu().numpy().astype(np.float64)
    tol = np.stack([bound[i * 32:(i + 1) * 32].sum(axis=0) + 1e-5 * np.abs(ref["dy"][i * 32:(i + 1) * 32]).sum(axis=0) for i in range(len(cs))])
    assert (np.abs(cs - ref["colsum"]) <= tol).all(), float((np.abs(cs - ref["colsum"]) / tol).max())
    pt = parts.cpu().numpy()
    Wb = np.array([ref["W"][i * 32:(i + 1) * 32].sum() for i in range(len(pt))])
    print("parts", pt, ref["parts"])
    assert (np.abs(pt - ref["parts"]) <= dl_tol * Wb + B * S * U * np.abs(ref["parts"])).all(), (pt, ref["parts"])


# ---- 1. the kernels against the definition -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("io,K", sorted(CASES), ids=["E%d-K%d" % (io // S, K) for io, K in sorted(CASES)])
def test_kernel_matches_the_definition(io, K, bf16):
    """E = 8, 16, 40, 72 x K = 1, 5, 33, 130, and E = 136, 520, 1024 for the kernel's other builds; B = 33 through the three mask
    routes and B = 1; the settings of CASES."""
    tau, emph_on, ids_on, pool_on, pad = CASES[(io, K)]
    seed = _seed(io, K)
    p = _problem(io)
    d, B = p["dev"], p["B"]
    weight = 0.7
    scale = float(np.float32(weight / (B * S)))
    noise = _noise()[0] if emph_on else None
    emph = (ALPHA, BETA, d["cw"]) if emph_on else None
    dt = torch.bfloat16 if bf16 else torch.float32
    dy_in = d["dy_in"].to(dt).float().cpu().numpy()
    common = dict(emph=emph, noise=noise, item_id=d["ids"] if ids_on else None, pool=d["pool"] if pool_on else None, bf16=bf16,
                  dy_ld=io + pad if pad else None)
    for name, route, rows, keep in _routes(p):
        ref = _ref(p, rows, keep, K, tau, scale, seed, emph_on, ids_on, pool_on, dy_in)
        assert fixture_ok(ref, rows, p["data"][rows], p["y"]), (name, "fixture conditions")
        out = contrast(d["data"], d["y"], d["dy_in"], K, tau, weight, seed, STEP, scale, **route, **common)
        _check(out, ref, p, K, tau, bf16, pad, dy_in, B)
        assert np.abs(ref["own"]).max() > 1e-3 * np.abs(dy_in).max()            # not vacuous: the term moves dY
    # B = 1: the first candidate of slot 0
    r1 = np.array([CR.candidate_rows(STEP, 0, K, seed, 120, p["pool"] if pool_on else None)[0]], dtype=np.int32)
    ref = _ref(p, r1, np.ones((1, io), np.uint8), K, tau, scale, seed, emph_on, ids_on, pool_on, dy_in[:1], y=p["y"][:1])
    assert ref["left_out"][0, 0].any()
    out = contrast(d["data"], d["y"][:1], d["dy_in"][:1], K, tau, weight, seed, STEP, scale, row_idx=torch.tensor(r1, device=DEV), **common)
    _check(out, ref, p, K, tau, bf16, pad, dy_in[:1], 1)


# ---- 2. properties -------------------------------------------------------------------------------------------------------------------

def _std(io=48, K=33, tau=0.1, **kw):
    p = _problem(io)
    d = p["dev"]
    base = dict(K=K, tau=tau, weight=0.7, seed=_seed(io, K), step=STEP, scale=float(np.float32(0.7 / (p["B"] * S))), item_id=d["ids"])
    base.update(kw)
    return p, d, base


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_same_inputs_same_bits_and_a_shard_is_the_full_batch_b33_io48_k33(bf16):
    """Twice the same call: dY, column sums and parts bit for bit.  Rows 8 .. 20 launched as their own batch with the global scale:
    bit for bit rows 8 .. 20 of the full launch (emphasis and MASKING noise on)."""
    p, d, base = _std(emph=None, bf16=bf16)
    base["emph"] = (ALPHA, BETA, d["cw"]); base["noise"] = _noise()[0]
    full = contrast(d["data"], d["y"], d["dy_in"], row_idx=d["rows"], mask_id=d["mask_id"], table=d["table"], **base)
    again = contrast(d["data"], d["y"], d["dy_in"], row_idx=d["rows"], mask_id=d["mask_id"], table=d["table"], **base)
    assert full[0] == 0 and again[0] == 0
    for a, b in zip(full[1:], again[1:]):
        assert torch.equal(_bits(a), _bits(b))
    part = contrast(d["data"], d["y"][8:21], d["dy_in"][8:21], row_idx=d["rows"][8:21].contiguous(), mask_id=d["mask_id"][8:21].contiguous(),
                    table=d["table"], **base)
    assert part[0] == 0
    assert torch.equal(_bits(part[1]), _bits(full[1][8:21]))
    assert not torch.equal(full[1][:, :48].float(), d["dy_in"].to(full[1].dtype).float())


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("w0", [False, True], ids=["W1", "W0"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_nonfinite_y_makes_exactly_its_pair_nan_b33_io48_k33(bad, w0, bf16):
    """One NaN / Inf in a y slot: that pair's E columns of dY, its block's column sums there and its block's part are NaN, every
    other element has the bits of the clean run.  W0: column weights of zero over slots 1 and 2, so W = 0 in the pairs that are hit -
    NaN all the same (weights multiply), while the clean run leaves those slots' dY exactly as it found them."""
    p, d, base = _std(bf16=bf16)
    if w0:
        cw = torch.cat([torch.ones(16, device=DEV), torch.zeros(32, device=DEV)])
        base["emph"] = (1.0, 1.0, cw)
    clean = contrast(d["data"], d["y"], d["dy_in"], row_idx=d["rows"], **base)
    y = d["y"].clone()
    y[4, 16 + 5] = bad                                      # row 4, slot 1
    y[32, 40] = bad                                         # the lone row of the second block, slot 2
    out = contrast(d["data"], y, d["dy_in"], row_idx=d["rows"], **base)
    assert out[0] == 0 and clean[0] == 0
    dt = torch.bfloat16 if bf16 else torch.float32
    moved = ~torch.eq(_bits(clean[1]), _bits(d["dy_in"].to(dt)))
    assert moved[:, :16].any() and moved[:, 16:].any() != w0            # W = 0: the clean run adds exactly nothing there
    hit = torch.zeros(33, 48, dtype=torch.bool, device=DEV)
    hit[4, 16:32] = True
    hit[32, 32:48] = True
    assert torch.isnan(out[1][hit].float()).all()
    assert torch.equal(_bits(out[1])[~hit], _bits(clean[1])[~hit])
    assert torch.isnan(out[3]).all()                        # both blocks hold a NaN pair
    cs, cc = out[2], clean[2]
    assert torch.isnan(cs[0, 16:32]).all() and torch.isnan(cs[1, 32:48]).all()
    assert torch.equal(_bits(cs[0, :16]), _bits(cc[0, :16])) and torch.equal(_bits(cs[0, 32:]), _bits(cc[0, 32:]))


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_zero_target_slot_and_a_lone_accidental_hit_give_no_gradient_io48(bf16):
    """A target slot of zeros: dY keeps dY_in in that pair, bit for bit, and the pair adds nothing to parts.  K = 1 with the only
    candidate the row itself: l = 0 and a zero gradient in that pair."""
    p, d, base = _std(bf16=bf16)
    data = d["data"].clone()
    data[p["rows"][2], 16:32] = 0.0
    out = contrast(data, d["y"], d["dy_in"], row_idx=d["rows"], **dict(base, item_id=None))
    dt = torch.bfloat16 if bf16 else torch.float32
    assert out[0] == 0 and torch.equal(_bits(out[1][2, 16:32]), _bits(d["dy_in"][2, 16:32].to(dt)))
    dnp = p["data"].copy(); dnp[p["rows"][2], 16:32] = 0.0
    ref = CR.terms(dnp, dnp[p["rows"]], p["y"], p["rows"], STEP, S, 33, 0.1, base["scale"], base["seed"])
    assert ref["l"][2, 1] == 0 and (ref["own"][2, 16:32] == 0).all()
    assert abs(float(out[3][0]) - ref["parts"][0]) <= (2 * 2.0 ** -8 / 0.1 if bf16 else 1e-4) * 96
    # K = 1, the batch is the candidate of slot 0 alone
    seed = base["seed"]
    r1 = np.array([CR.candidate_rows(STEP, 0, 1, seed, 120)[0]], dtype=np.int32)
    ref1 = CR.terms(p["data"], p["data"][r1], p["y"][:1], r1, STEP, S, 1, 0.1, base["scale"], seed)
    assert ref1["left_out"][0, 0, 0] and ref1["l"][0, 0] == 0
    o1 = contrast(d["data"], d["y"][:1], d["dy_in"][:1], row_idx=torch.tensor(r1, device=DEV), **dict(base, K=1, item_id=None))
    assert o1[0] == 0 and torch.equal(_bits(o1[1][0, 0:16]), _bits(d["dy_in"][0, 0:16].to(dt)))
    if not ref1["left_out"][0, 1:].any():
        assert abs(float(o1[3][0]) - ref1["parts"][0]) <= (2 * 2.0 ** -8 / 0.1 if bf16 else 1e-4) * 3


def test_launcher_refusals_write_nothing_io48():
    """Both launchers refuse a bad struct by themselves: the prepare launch leaves ws as it was, the contrast launch (called alone,
    on a ws that a good prepare filled) leaves dY, the column sums and the parts as they were.  Then the contrast launcher's own
    checks: dy_ld below io, a scale that is not finite, mask ids without a table, E = 1025 (unsupported, naming E)."""
    from codae import hip
    lib = hip.lib()
    p, d, base = _std()
    good_ws = torch.zeros(lib.codae_slot_contrast_ws_bytes(S, 33, 16, 0), dtype=torch.uint8, device=DEV)
    assert contrast(d["data"], d["y"], d["dy_in"], row_idx=d["rows"], ws=good_ws, **base)[0] == 0
    filled = good_ws.clone()
    small = torch.zeros(64, dtype=torch.uint8, device=DEV)

    def untouched(out, kw):
        rc, dy, colsum, parts = out
        assert torch.equal(dy[:, :48], d["dy_in"]) and (dy[:, 48:] == FILL).all() and (colsum == FILL).all() and (parts == FILL).all(), kw

    for kw in (dict(ws=small), dict(K=0), dict(K=4097), dict(tau=0.005), dict(tau=float("nan")), dict(weight=-1.0), dict(n_slots=5)):
        args = dict(base, **kw)
        args.setdefault("ws", good_ws)
        # the prepare launcher alone
        st = hip.SlotContrast(args.get("n_slots", S), args["K"], args["tau"], args["weight"], args["seed"], 120, 0, int(args["ws"].numel()), None,
                              hip.ptr(d["ids"]), hip.ptr(args["ws"]))
        assert lib.codae_slot_contrast_prepare(hip.ptr(d["data"]), 48, C.byref(st), STEP, 0, hip.current_stream()) == -1, kw
        torch.cuda.synchronize()
        assert torch.equal(good_ws, filled) and (small == 0).all(), kw
        # the contrast launcher alone
        out = contrast(d["data"], d["y"], d["dy_in"], row_idx=d["rows"], prepare=False, **args)
        assert out[0] == -1, kw
        untouched(out, kw)
    for kw, route in ((dict(dy_ld=40), dict(row_idx=d["rows"])), (dict(scale=float("nan")), dict(row_idx=d["rows"])),
                      (dict(scale=float("inf")), dict(row_idx=d["rows"])), (dict(), dict(row_idx=d["rows"], mask_id=d["mask_id"]))):
        out = contrast(d["data"], d["y"], d["dy_in"], prepare=False, ws=good_ws, **route, **dict(base, **kw))
        assert out[0] == -1, (kw, route)
        untouched(out, kw)
    big = torch.zeros(2, 1025, device=DEV)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    for prep in (True, False):
        rc = contrast(big, big, big, 4, 0.1, 1.0, 0, 1, 1.0, n_slots=1, ws=ws, prepare=prep)[0]
        assert rc == -3 and b"1025" in lib.codae_last_error(), prep


# ---- 3. whole steps -----------------------------------------------------------------------------------------------------------------

def _stack(B, seed, N=120, io=48, dup=True):
    """io 48: 48-32-16-32-48, S = 3 one-slot masks, one mask run; dataset rows 100 .. 104 repeat items of rows 0 .. 4."""
    from oracle import dae_oracle as O
    rng = np.random.default_rng(seed)
    E = io // 3
    data = rng.random((N, io), dtype=np.float32)
    if dup:
        data[100:105, 0:E] = data[0:5, 0:E]
    sched = [(io, 32, True), (32, 16, True), (16, 32, True), (32, io, False)]
    params = O.init_params(sched, rng)
    bm, nmr, _ = O.corrupter_tables([{"size": E, "position": s * E} for s in range(3)], 1)
    mtu = rng.integers(0, 3, (N, 1)).astype(np.int32)
    order = [rng.permutation(N)[:B].astype(np.int32) for _ in range(4)]
    return dict(io=io, data=data, sched=sched, params=params, bm=bm, nmr=nmr, mtu=mtu, order=order, B=B, ids=CR.item_ids(data, 3))


def _trainer(p, precision, **kw):
    from codae.train import HipEmbeddingTrainer
    t = HipEmbeddingTrainer(p["sched"], torch.tensor(p["data"]), torch.tensor(p["bm"]).to(torch.uint8), torch.tensor(p["mtu"]), 1e-3,
                            1e-4, 1.0, max_batch=p["B"], precision=precision, device=DEV, **kw)
    t.load_params(p["params"])
    return t


def _idx(p, s):
    return torch.tensor(p["order"][s], dtype=torch.int32, device=DEV)


def _fmask(p, idx, run=0):
    from oracle import dae_oracle as O
    return O.get_masks(p["bm"], p["nmr"], p["mtu"], 1, idx, run)[1]


def _sc(K=33, tau=0.1, weight=0.5, seed=77, **kw):
    from codae.tool import SlotContrast
    return SlotContrast(negatives=K, temperature=tau, weight=weight, seed=seed, **kw)


def _crit(name):
    from codae.tool import ReconstructionLoss
    return None if name == "mse" else ReconstructionLoss(name)


def _state(t):
    return t.engine.read_scalars(), t.engine.params.clone(), t.engine.grads.clone()


def _same(a, b):
    return a[0] == b[0] and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))


def _rel_l2(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _oracle(p, name, quant=None, K=33, tau=0.1, weight=0.5, seed=77, distinct=True):
    return CR.ContrastOracle(p["params"], [r for _, _, r in p["sched"]], 1e-3, 1e-4, p["data"], 3, K, tau, weight, seed,
                             item_id=p["ids"] if distinct else None, kind=name, quant=quant)


@pytest.mark.parametrize("name", ["mse", "slot_cosine"])
def test_f32_steps_match_the_oracle_with_the_contrast_io48_b33(name):
    """Three steps: loss (criterion + term) and gradient norm of every step, every gradient tensor of the first, the parameters
    after the third at rtol 1e-3 / atol 1e-5; epoch_sums() stay the unweighted squared-error sums."""
    p = _stack(33, seed=41)
    t = _trainer(p, "f32", criterion=_crit(name), contrast=_sc())
    eng = t.engine
    assert eng.step_path(33) == "layers"
    orc = _oracle(p, name)
    sq_sum = sqp_sum = 0.0
    for s in range(3):
        idx = p["order"][s]
        ro = orc.step(p["data"][idx], idx, _fmask(p, idx))
        t.train_batch(_idx(p, s), run=0)
        _, _, gsq, loss = eng.read_scalars()
        print(s, "loss", loss, ro["loss"], "criterion", ro["criterion"], "contrast", ro["contrast"], "gnorm", math.sqrt(gsq), ro["grad_norm"])
        assert close(loss, ro["loss"]), (s, loss, ro["loss"])
        assert ro["contrast"] > 0.1 * ro["loss"]                  # not vacuous: the term is a large share of the loss
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
    assert close(sq, sq_sum) and close(sqp, sqp_sum), (sq, sq_sum, sqp, sqp_sum)


@pytest.mark.parametrize("name", ["mse", "slot_cosine"])
def test_bf16_first_step_gradients_match_the_bf16_rounded_oracle_io48_b33(name):
    from oracle import dae_oracle as O
    p = _stack(33, seed=42)
    t = _trainer(p, "bf16", criterion=_crit(name), contrast=_sc())
    eng = t.engine
    assert eng.precision == 1 and eng.step_path(33) == "layers"
    orc = _oracle(p, name, quant=O.bf16_round)
    idx = p["order"][0]
    ro = orc.step(p["data"][idx], idx, _fmask(p, idx))
    t.train_batch(_idx(p, 0), run=0)
    _, _, gsq, loss = eng.read_scalars()
    print("loss", loss, ro["loss"], "contrast", ro["contrast"], "gnorm", math.sqrt(gsq), ro["grad_norm"])
    assert abs(loss - ro["loss"]) <= 2e-3 * abs(ro["loss"]) + 0.5 * 2 * 2.0 ** -8 / 0.1      # (weight x the bf16 logit bound)
    worst = 0.0
    for l, (gw, gb) in enumerate(orc.last_grads):
        ew, eb = _rel_l2(eng.weight_grad(l).cpu().numpy(), gw), _rel_l2(eng.bias_grad(l).cpu().numpy(), gb)
        print("layer", l, "dW", ew, "db", eb)
        worst = max(worst, ew, eb)
    print("bf16 step: worst relative L2 %.3e (bound %.3e)" % (worst, BF16_STEP_L2))
    assert worst <= BF16_STEP_L2


def test_graph_replay_is_the_plain_step_bit_for_bit_io48_b33():
    """Three replayed steps = three plain steps: the candidates change every step, so a step word frozen into the graph fails here."""
    p = _stack(33, seed=43)
    out = []
    for graph in (False, True):
        t = _trainer(p, "bf16", criterion=_crit("slot_cosine"), contrast=_sc(), use_graph=graph)
        losses = []
        for s in range(3):
            t.train_batch(_idx(p, 0), run=0)                 # the same rows every step: only the step word moves the candidates
            losses.append(t.engine.read_scalars()[3])
        out.append((_state(t), losses))
    assert out[0][1] == out[1][1], (out[0][1], out[1][1])
    assert _same(out[0][0], out[1][0])
    # a change of the setting between replays re-captures
    res = []
    for graph in (False, True):
        t = _trainer(p, "bf16", use_graph=graph)
        losses = []
        for s, c in enumerate((_sc(), None, _sc(K=5), _sc(K=5, weight=0.25))):
            t.set_contrast(c)
            t.train_batch(_idx(p, s), run=0)
            losses.append(t.engine.read_scalars()[3])
        res.append((_state(t), losses))
    assert res[0][1] == res[1][1] and _same(res[0][0], res[1][0]) and len(set(res[0][1])) == 4


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_forward_loss_backward_update_is_the_one_call_step_io48_b33(precision):
    """codae_step_forward_loss + backward + update against codae_train_step.  The loss and the metric sums are the same launches in
    both forms: bit for bit.  The two forms add the gradients and their sum of squares in different orders, whatever the loss is (the
    one-call step gathers sum g^2 in the producing epilogues, the update call in a pass of its own): the gradient tensors agree to
    1e-5 relative L2 (fp32 summation order), the norm to 1e-6, the parameters after Adam at the project's rtol 1e-3 / atol 1e-5."""
    p = _stack(33, seed=44)
    a, b = (_trainer(p, precision, criterion=_crit("slot_cosine"), contrast=_sc()) for _ in range(2))
    a.train_batch(_idx(p, 0), run=0)
    eng = b.engine
    batch = b._batch(_idx(p, 0), 0)
    hyper = eng.hyper(1e-3, 1e-4, 1.0, global_rows=33, step=1)
    eng.step_forward_loss(batch, hyper)
    eng.step_backward(33, 0, eng.L)
    eng.step_update(hyper)
    sa, sb = _state(a), _state(b)
    assert sa[0][0] == sb[0][0] and sa[0][1] == sb[0][1] and sa[0][3] == sb[0][3], (sa[0], sb[0])
    assert abs(sa[0][2] - sb[0][2]) <= 1e-6 * sa[0][2], (sa[0][2], sb[0][2])
    for l in range(eng.L):
        for ga, gb in ((a.engine.weight_grad(l), eng.weight_grad(l)), (a.engine.bias_grad(l), eng.bias_grad(l))):
            assert _rel_l2(gb.cpu().numpy(), ga.cpu().numpy()) <= 1e-5, l
        assert close(eng.weight(l).cpu().numpy(), a.engine.weight(l).cpu().numpy()) and close(eng.bias(l).cpu().numpy(), a.engine.bias(l).cpu().numpy())
    plain = _trainer(p, precision, criterion=_crit("slot_cosine"))
    plain.train_batch(_idx(p, 0), run=0)
    assert plain.engine.read_scalars()[3] != sa[0][3]          # not vacuous: the term is in both forms


def test_half_batches_with_global_rows_sum_to_the_full_batch_io48_b32():
    """fp32 engine: gradients of rows 0 .. 15 and 16 .. 31 with global_rows = 32 add up to the full batch's, within fp32 summation
    error (1e-5 relative of the largest element per tensor); the losses add up too."""
    p = _stack(32, seed=45)
    grads, losses = [], []
    for lo, hi in ((0, 32), (0, 16), (16, 32)):
        t = _trainer(p, "f32", criterion=_crit("slot_cosine"), contrast=_sc())
        eng = t.engine
        idx = _idx(p, 0)[lo:hi].contiguous()
        eng.step_forward_loss(t._batch(idx, 0), eng.hyper(1e-3, 1e-4, 1.0, global_rows=32, step=1))
        eng.step_backward(hi - lo, 0, eng.L)
        grads.append(eng.grads.clone())
        losses.append(eng.read_scalars()[3])
    full, parts = grads[0], grads[1] + grads[2]
    assert float((full - parts).abs().max()) <= 1e-5 * float(full.abs().max())
    assert abs(losses[0] - losses[1] - losses[2]) <= 1e-6 * losses[0]


@pytest.mark.parametrize("precision,B", [("bf16", 40), ("f32", 33)], ids=["bf16-chain", "f32"])
def test_off_leaves_the_step_as_it_was(precision, B):
    """contrast=None, weight = 0, and a contrast set and cleared again: the bits of a trainer built without the argument after three
    steps, on the path it took before (the chain kernel for the narrow bf16 stack)."""
    from oracle import dae_oracle as O
    rng = np.random.default_rng(5)
    io = 192 if precision == "bf16" else 48
    E = io // 3
    data = rng.random((120, io), dtype=np.float32)
    sched = [(io, 64, True), (64, io, False)]
    bm, nmr, _ = O.corrupter_tables([{"size": E, "position": s * E} for s in range(3)], 1)
    p = dict(io=io, data=data, sched=sched, params=O.init_params(sched, rng), bm=bm, nmr=nmr, mtu=rng.integers(0, 3, (120, 1)).astype(np.int32),
             order=[rng.permutation(120)[:B].astype(np.int32) for _ in range(4)], B=B)
    plain = _trainer(p, precision)
    none = _trainer(p, precision, contrast=None)
    zero = _trainer(p, precision, contrast=_sc(weight=0.0))
    back = _trainer(p, precision, contrast=_sc())
    assert back.engine.step_path(B) == "layers"
    back.train_batch(_idx(p, 3), run=0)
    other = _state(back)
    back.load_params(p["params"])
    back.engine.adam_m.zero_(); back.engine.adam_v.zero_(); back.engine.step_count = 0
    back.engine.zero_metric_sums()
    back.set_contrast(None)
    path = "chain" if precision == "bf16" else "layers"
    for t in (plain, none, zero, back):
        assert t.engine.step_path(B) == path
        t.engine.zero_metric_sums()
        for s in range(3):
            t.train_batch(_idx(p, s), run=0)
    ref = _state(plain)
    for t in (none, zero, back):
        assert _same(_state(t), ref)
    assert other[0][3] != ref[0][3]


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_evaluation_and_completion_never_see_the_term_io48_b33(precision):
    p = _stack(33, seed=46)
    a = _trainer(p, precision)
    b = _trainer(p, precision, contrast=_sc())
    ya = a.eval_batch(_idx(p, 0), run=0, want_y=True)
    yb = b.eval_batch(_idx(p, 0), run=0, want_y=True)
    assert torch.equal(ya, yb) and a.engine.read_scalars()[:2] == b.engine.read_scalars()[:2]
    ia, sa = a.complete(_idx(p, 0), 1, 5)
    ib, sb = b.complete(_idx(p, 0), 1, 5)
    assert torch.equal(ia, ib) and torch.equal(sa, sb)


def test_set_slot_contrast_refusals_leave_the_previous_setting_io48_b33():
    from codae import hip
    from codae.hip import HipError
    p = _stack(33, seed=47)
    t = _trainer(p, "f32", contrast=_sc())
    ref = _trainer(p, "f32", contrast=_sc())
    eng = t.engine
    data, pool, ids, ws = eng._contrast_pins
    good = dict(n_slots=3, n_neg=33, tau=0.1, weight=0.5, seed=77, n_rows=120, n_pool=0, ws_bytes=int(ws.numel()), pool=None, item_id=hip.ptr(ids),
                ws=hip.ptr(ws))
    empty = torch.zeros(1, dtype=torch.int32, device=DEV)
    for kw in (dict(ws_bytes=64), dict(n_neg=0), dict(n_neg=4097), dict(tau=0.005), dict(tau=float("nan")), dict(weight=-0.5),
               dict(n_slots=5), dict(pool=hip.ptr(empty), n_pool=0), dict(ws=None)):
        st = hip.SlotContrast(**dict(good, **kw))
        with pytest.raises(HipError):
            eng._set_contrast_struct(st)
    with pytest.raises(HipError):
        t.set_contrast(_sc(candidates=[0, 120]))
    for tr in (t, ref):
        tr.train_batch(_idx(p, 0), run=0)
    assert _same(_state(t), _state(ref))


@pytest.mark.parametrize("name", ["mse", "slot_cosine"])
def test_last_loss_is_the_criterions_loss_plus_the_term_io48_b33(name):
    p = _stack(33, seed=48)
    with_c = _trainer(p, "f32", criterion=_crit(name), contrast=_sc())
    without = _trainer(p, "f32", criterion=_crit(name))
    orc = _oracle(p, name)
    idx = p["order"][0]
    ro = orc.step(p["data"][idx], idx, _fmask(p, idx))
    for t in (with_c, without):
        t.train_batch(_idx(p, 0), run=0)
    la, lb = with_c.engine.read_scalars()[3], without.engine.read_scalars()[3]
    print(la, lb, ro)
    assert close(lb, ro["criterion"]) and close(la - lb, ro["contrast"]) and ro["contrast"] > 0.05
