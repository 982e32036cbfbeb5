"""Sparse code on a real MI355X (include/codae_hip.h, "Sparse code"): the two kernels on their own, bit for bit against
tests/sparse_ref.py; whole steps of both engines against the restatement evaluated under the engine's own mask; and every form the
setting reaches - skips and norms around it, dropout, tied weights, emphasis, swap noise, slot_cosine, graph replay, the backward by
ranges, rotating gradient buffers, off, the model surface, refusals, checkpoints and a NaN.

Tolerances.  Kernels: exact (values, +0 stores, mask bytes, pad bits, column-sum bits).  Steps: the engine's mask must have exactly
`keep` bits per row and be a VALID selection of the restatement's pre-selection magnitudes - no kept column's magnitude below a
dropped column's by more than 4 units in the last place of the threshold value (2^-8 relative in bf16, 2^-23 in fp32); under that
mask, fp32 steps are within rtol 1e-3 / atol 1e-5 of the float64 statement (tests/test_gpu_norm.py's bounds for the same stacks)
and the bf16 first step within 2e-3 relative L2 per gradient tensor of the rounded restatement.
"""
import ctypes as C
import math

import numpy as np
import pytest

import sparse_ref as SR
from golden_util import close, max_err
from residual_ref import colsum_parts_fixed_order
from test_gpu_norm import _fmask, _idx, _norm, _problem, _rel_l2, _res, _same, _snapshot, _square, _trainer

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
POISON = 7.0
EPS = 1e-5
ROWS = (1, 5, 70)
# the last three: fp32 widths = 4 (mod 8) on the 16-byte path, whose last lane holds half a chunk (one quad, four live mask bits)
SHAPES = [(True, 8, 8), (True, 24, 32), (True, 520, 528), (True, 1536, 1536), (False, 1, 1), (False, 21, 23), (False, 264, 268),
          (False, 1537, 1540), (False, 12, 12), (False, 20, 24), (False, 516, 516)]
SHAPE_IDS = ["bf16-w8", "bf16-w24", "bf16-w520", "bf16-w1536", "f32-w1", "f32-w21-elem", "f32-w264", "f32-w1537-elem", "f32-w12", "f32-w20",
             "f32-w516"]
TIES = (6, 7, 8, 9, 510, 511, 512, 513, 514, 515)
HALF_TIES = (10, 11, 12, 13, 514, 515, 516, 517)


def _keeps(width):
    half = {4} if width % 8 == 4 and width > 4 else set()       # keep 4 with _last_quad_row: exactly the half chunk is kept
    return sorted({1, min(2, width), max(1, width // 8), max(1, width - 1), width} | half)


def _bf16_valued(a):
    return (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def _device(a, bf16):
    """fp32 numpy (bf16: bf16-valued) -> the device tensor of the working type with exactly those bits (no converting cast: a NaN
    keeps its payload)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if bf16:
        return torch.tensor((a.view(np.uint32) >> 16).astype(np.uint16).view(np.int16), device=DEV).view(torch.bfloat16)
    return torch.tensor(a.view(np.int32), device=DEV).view(torch.float32)


def _host_bits(t):
    """the stored bits as uint32 (a bf16 in the high half, as widening puts it)"""
    if t.dtype == torch.bfloat16:
        return (t.view(torch.int16).cpu().numpy().view(np.uint16).astype(np.uint32)) << 16
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def _last_quad_row(width, rng):
    """the four largest magnitudes in the last four columns: with keep 4 and a width = 4 (mod 8), the kept set is the half chunk"""
    r = (rng.random(width).astype(np.float32) * 0.9 + 0.05) * rng.choice([-1.0, 1.0], width).astype(np.float32)
    r[width - 4:] = np.array([3.0, -2.5, 2.0, -3.5], dtype=np.float32)
    return r


def _tie_row(width, keep, rng, ties=TIES):
    """ties of magnitude 2 that straddle a lane's 8-column chunk (columns 6 .. 9) and a 64-lane tile (510 .. 515) - HALF_TIES: the
    two quads of a chunk (10 .. 13) and, at widths 12 and 516, the half chunk a width = 4 (mod 8) ends in (10, 11; 514, 515) -
    with so many larger values - in the HIGHEST other columns - that the threshold falls among the ties"""
    ties = [c for c in ties if c < width]
    r = (rng.random(width).astype(np.float32) * 0.9 + 0.05) * rng.choice([-1.0, 1.0], width).astype(np.float32)
    n_big = keep - len(ties) // 2
    others = [c for c in range(width) if c not in ties]
    if not ties or n_big < 0 or n_big > len(others):
        return None
    r[ties] = 2.0
    r[ties[1::2]] = -2.0
    if n_big:
        r[others[-n_big:]] = 3.0
    return r


def _rows(rng, B, width, keep, bf16):
    """B rows: the planted ones first (as many as fit), then random ones with 15 % exact zeros"""
    a = rng.standard_normal((B, width)).astype(np.float32)
    a[rng.random((B, width)) < 0.15] = 0.0
    planted = []
    if width >= 8:
        planted = list(SR.planted_rows(width, keep, rng))
        first = [_tie_row(width, keep, rng), _tie_row(width, keep, rng, HALF_TIES)]
        if width % 8 == 4:
            first.reverse()
            if keep == 4:
                first.insert(0, _last_quad_row(width, rng))
        planted = [t for t in first if t is not None] + planted
    for i, r in enumerate(planted[:B]):
        a[i] = r
    return _bf16_valued(a) if bf16 else a


def _padded(a, ld, pad_rows=2):
    B, width = a.shape
    full = np.full((B + pad_rows, ld), POISON, dtype=np.float32)
    full[:B, :width] = a
    return full


def _fwd(y, bf16, ld, B, width, keep, bits=None, ld_bits=0):
    from codae import hip
    rc = hip.lib().codae_sparse_code_fwd(hip.ptr(y), int(bf16), ld, B, width, keep, hip.ptr(bits), ld_bits, hip.current_stream())
    torch.cuda.synchronize()
    return rc


def _bwd(d, bf16, ld, B, width, bits, ld_bits, colsum=True):
    from codae import hip
    lib = hip.lib()
    blocks = lib.codae_sparse_code_blocks(B)
    cs = torch.full((blocks + 1, width), POISON, dtype=torch.float32, device=DEV) if colsum else None
    rc = lib.codae_sparse_code_bwd(hip.ptr(d), int(bf16), ld, B, width, hip.ptr(bits), ld_bits, hip.ptr(cs), hip.current_stream())
    torch.cuda.synchronize()
    return rc, cs


@pytest.mark.parametrize("bf16,width,ld", SHAPES, ids=SHAPE_IDS)
def test_forward_kernel_bit_for_bit(bf16, width, ld):
    from codae import hip
    rng = np.random.default_rng(width * 3 + int(bf16))
    nb = (width + 7) // 8
    for B in ROWS:
        for keep in _keeps(width):
            a = _rows(rng, B, width, keep, bf16)
            full = _padded(a, ld)
            want_mask = SR.select(a, keep, bf16)
            want = _padded(SR.apply_bits(a, want_mask), ld)
            y = _device(full, bf16)
            bits = torch.full((B + 1, nb + 1), 0xAA, dtype=torch.uint8, device=DEV)
            assert _fwd(y, bf16, ld, B, width, keep, bits, nb + 1) == 0, hip.lib().codae_last_error()
            got = _host_bits(y)
            assert np.array_equal(got, want.view(np.uint32)), (B, keep, np.argwhere(got != want.view(np.uint32))[:8])     # values, +0, pads
            gb = bits.cpu().numpy()
            assert np.array_equal(gb[:B, :nb], SR.packed(want_mask)), (B, keep, "mask bytes and pad bits")
            assert (gb[:B, nb] == 0xAA).all() and (gb[B] == 0xAA).all()
            # the evaluation form (no mask buffer): the same values
            y2 = _device(full, bf16)
            assert _fwd(y2, bf16, ld, B, width, keep) == 0
            assert np.array_equal(_host_bits(y2), got), (B, keep, "bits = NULL")


@pytest.mark.parametrize("bf16,width,ld", SHAPES, ids=SHAPE_IDS)
def test_backward_kernel_bit_for_bit_and_column_sums(bf16, width, ld):
    from codae import hip
    rng = np.random.default_rng(width * 5 + int(bf16))
    nb = (width + 7) // 8
    for B in ROWS:
        for keep in _keeps(width):
            mask = SR.select(_rows(rng, B, width, keep, bf16), keep, bf16)
            g = rng.standard_normal((B, width)).astype(np.float32)
            g[rng.random((B, width)) < 0.1] = -0.0
            dropped = np.argwhere(~mask)
            if len(dropped) >= 2:                                   # a NaN and an Inf gradient under dropped columns: +0 afterwards
                g[tuple(dropped[0])] = np.nan
                g[tuple(dropped[-1])] = -np.inf
            if bf16:
                g = _bf16_valued(g)
            full = _padded(g, ld)
            want = _padded(SR.apply_bits(g, mask), ld)
            bits_np = np.full((B + 1, nb + 1), 0x55, dtype=np.uint8)
            bits_np[:B, :nb] = SR.packed(mask)
            bits = torch.tensor(bits_np, device=DEV)
            d = _device(full, bf16)
            rc, cs = _bwd(d, bf16, ld, B, width, bits, nb + 1)
            assert rc == 0, hip.lib().codae_last_error()
            got = _host_bits(d)
            assert np.array_equal(got, want.view(np.uint32)), (B, keep, np.argwhere(got != want.view(np.uint32))[:8])
            blocks = (B + 63) // 64
            csn = cs.cpu().numpy()
            assert (csn[blocks] == POISON).all()
            stored = want[:B, :width]
            assert np.array_equal(csn[:blocks].view(np.uint32), colsum_parts_fixed_order(stored, B).view(np.uint32)), (B, keep, "column-sum bits")
            assert np.array_equal(bits.cpu().numpy(), bits_np)
            d2 = _device(full, bf16)
            rc, _ = _bwd(d2, bf16, ld, B, width, bits, nb + 1, colsum=False)
            assert rc == 0 and np.array_equal(_host_bits(d2), got), (B, keep, "colsum_part = NULL")


@pytest.mark.parametrize("bf16,width,ld", [(True, 24, 32), (True, 520, 528), (False, 21, 23), (False, 264, 268)],
                         ids=["bf16-w24", "bf16-w520", "f32-w21-elem", "f32-w264"])
def test_a_rows_results_do_not_depend_on_the_other_rows_of_the_call(bf16, width, ld):
    """rows 64 .. 129 of a 130-row call have the bits of the same rows in a 66-row call, forward and backward"""
    rng = np.random.default_rng(width + 17)
    nb = (width + 7) // 8
    keep = max(1, width // 8)
    a = _padded(_rows(rng, 130, width, keep, bf16), ld, 0)
    g = _padded(_bf16_valued(rng.standard_normal((130, width))) if bf16 else rng.standard_normal((130, width)).astype(np.float32), ld, 0)
    out = []
    for lo in (0, 64):
        B = 130 - lo
        y = _device(a[lo:], bf16)
        bits = torch.zeros((B, nb), dtype=torch.uint8, device=DEV)
        assert _fwd(y, bf16, ld, B, width, keep, bits, nb) == 0
        d = _device(g[lo:], bf16)
        rc, _ = _bwd(d, bf16, ld, B, width, bits, nb)
        assert rc == 0
        out.append((_host_bits(y)[64 - lo:], bits.cpu().numpy()[64 - lo:], _host_bits(d)[64 - lo:]))
    for whole, part, name in zip(out[0], out[1], ("values", "mask", "d")):
        assert np.array_equal(whole, part), name


# ---- engines ---------------------------------------------------------------------------------------------------------------

def _sparse(keep, layer=None):
    from codae.tool import SparseCode
    return SparseCode(keep, layer=layer)


def _engine_params(t):
    return [(w.cpu().numpy(), b.cpu().numpy()) for w, b in t.params()]


def _mask_of(t, p, Z, keep):
    mask = SR.unpacked(t.engine.sparse_bits(p["B"]).cpu().numpy(), Z)
    assert (mask.sum(axis=1) == keep).all(), "every row has exactly `keep` bits set"
    return mask


def _check_f32_step(t, ref, p, s, Z, c=None, dy_of=None, factors=None):
    """One step: the engine's mask is a valid selection; under it the loss, every gradient tensor and the parameters after the
    update are within rtol 1e-3 / atol 1e-5 of the float64 statement."""
    eng = t.engine
    idx = p["order"][s]
    x = p["data"][idx]
    c = x * _fmask(p, idx) if c is None else c
    t.train_batch(torch.tensor(idx, dtype=torch.int32, device=DEV), run=0)
    mask = _mask_of(t, p, Z, ref.keep)
    ro = ref.step(c, SR.mse(x) if dy_of is None else dy_of, factors, mask=mask)
    ok, worst = SR.selection_is_valid(ref.last_pre, mask, ref.keep, False)
    same = bool((SR.select(ref.last_pre.astype(np.float32), ref.keep) == mask).all())
    print("MEASURE f32 step %d: selection worst gap / allowance %.3g, equals the float64 ranking: %s" % (s, worst, same))
    assert ok, worst
    _, _, gsq, loss = eng.read_scalars()
    print("loss", loss, ro["loss"], "gnorm", math.sqrt(gsq), ro["grad_norm"])
    assert close(loss, ro["loss"]), (loss, ro["loss"])
    assert close(math.sqrt(gsq), ro["grad_norm"]), (math.sqrt(gsq), ro["grad_norm"])
    worst_g = 0.0
    for l, (gw, gb) in enumerate(ref.last_grads):
        ew, eb = max_err(eng.weight_grad(l).cpu().numpy(), gw), max_err(eng.bias_grad(l).cpu().numpy(), gb)
        worst_g = max(worst_g, ew, eb)
        assert ew <= 1.0, ("dW", l, ew)
        assert eb <= 1.0, ("db", l, eb)
    print("MEASURE f32 step %d: worst gradient error / tolerance %.3g" % (s, worst_g))
    for l, (w_, b_) in enumerate(ref.params):
        assert close(eng.weight(l).cpu().numpy(), w_), ("W", l, max_err(eng.weight(l).cpu().numpy(), w_))
        assert close(eng.bias(l).cpu().numpy(), b_), ("b", l, max_err(eng.bias(l).cpu().numpy(), b_))
    return mask


@pytest.mark.parametrize("act", ["relu", "leaky"])
@pytest.mark.parametrize("L", [4, 5])
def test_f32_engine_steps_match_the_float64_statement_under_the_engines_mask_w24_b70(L, act):
    p = _square(L, 24, 70, act, seed=10 * L + len(act))
    layer, keep = L // 2, 6
    t = _trainer(p, "f32", sparse_code=_sparse(keep, layer))
    assert t.engine.sparse_resolved == (layer - 1, 24) and t.engine.step_path(70) == "layers"
    ref = SR.StepRef(p["params"], p["names"], [0] * L, [0] * L, "layer", EPS, 1e-3, 1e-4, layer - 1, keep)
    for s in range(2):
        _check_f32_step(t, ref, p, s, 24)
    # ... and not the dense network
    idx = p["order"][0]
    x = p["data"][idx]
    import norm_ref as NR
    off = NR.gradients(p["params"], p["names"], [0] * L, [0] * L, "layer", EPS, x * _fmask(p, idx), SR.mse(x))[1]
    on = SR.gradients(p["params"], p["names"], [0] * L, [0] * L, "layer", EPS, x * _fmask(p, idx), SR.mse(x), layer - 1, keep)[1]
    assert abs(on - off) > 1e-3 * off


def _bf16_steps(p, layer, keep, Z, steps=2):
    """the first `steps` steps of the bf16 engine: every step's mask is a valid selection of the rounded restatement's stored
    pre-selection values; -> the first step's worst relative L2 error of a gradient tensor against the restatement under that mask"""
    L = p["L"]
    t = _trainer(p, "bf16", sparse_code=_sparse(keep, layer))
    assert t.engine.step_path(p["B"]) == "layers"
    first = None
    for s in range(steps):
        params = _engine_params(t)
        idx = p["order"][s]
        x = p["data"][idx]
        t.train_batch(_idx(p, s), run=0)
        mask = _mask_of(t, p, Z, keep)
        grads, loss, _, pre, _ = SR.gradients(params, p["names"], [0] * L, [0] * L, "layer", EPS, x * _fmask(p, idx), SR.mse(x), layer - 1, keep,
                                              mask=mask, bf16=True)
        ok, worst_sel = SR.selection_is_valid(pre, mask, keep, True)
        same = float((SR.select(pre.astype(np.float32), keep, True) == mask).all(axis=1).mean())
        eng = t.engine
        got_loss = eng.read_scalars()[3]
        worst = 0.0
        for l, (gw, gb) in enumerate(grads):
            worst = max(worst, _rel_l2(eng.weight_grad(l).cpu().numpy(), gw), _rel_l2(eng.bias_grad(l).cpu().numpy(), gb))
        print("MEASURE bf16 step %d, widths %s, B %d, keep %d at layer %d: selection worst gap / allowance %.3g, rows equal to the restatement's "
              "ranking %.3f, loss %.6f (restatement %.6f), worst gradient error %.3e" % (s, p["widths"], p["B"], keep, layer, worst_sel, same,
                                                                                           got_loss, loss, worst))
        assert ok, worst_sel
        if s == 0:
            assert abs(got_loss - loss) <= 1e-3 * abs(loss)
            first = worst
    return first


@pytest.mark.parametrize("act", ["relu", "leaky"])
@pytest.mark.parametrize("L", [4, 5])
def test_bf16_first_step_gradients_match_the_rounded_restatement_under_the_engines_mask_w192_b40(L, act):
    """Measured on MI355X: DESIGN.md section 6, "Sparse code"."""
    p = _square(L, 192, 40, act, seed=7 * L + len(act))
    worst = _bf16_steps(p, L // 2, 48, 192)
    assert worst <= 2e-3, worst


def test_bf16_first_step_on_the_pipelined_256x192_tiles_w264_b264(monkeypatch):
    from codae import hip
    monkeypatch.setenv("CODAE_GEMM_TILE", "x")
    hip.check(hip.lib().codae_reload_env())
    try:
        p = _square(4, 264, 264, "relu", seed=44)
        worst = _bf16_steps(p, 2, 66, 264)
        assert worst <= 2e-3, worst
    finally:
        monkeypatch.delenv("CODAE_GEMM_TILE")
        hip.check(hip.lib().codae_reload_env())


# ---- composition ------------------------------------------------------------------------------------------------------------------

CODE = ["relu", "relu", None, "relu", None]          # the code layer m = 2 has no activation: Linear 3 reads the code


def test_skips_on_every_other_hidden_layer_f32_w24_b70():
    """a skip around layer 1 and around Linear 3, which READS the sparse code: the residual backward kernel sits in front of the
    sparse one at that site"""
    p = _problem([24] * 6, CODE, 70, seed=31)
    t = _trainer(p, "f32", residual=_res([1, 3]), sparse_code=_sparse(6))
    assert t.engine.sparse_resolved == (2, 24) and t.engine.residual_layers == [1, 3]
    ref = SR.StepRef(p["params"], p["names"], [0, 1, 0, 1, 0], [0] * 5, "layer", EPS, 1e-3, 1e-4, 2, 6)
    for s in range(2):
        _check_f32_step(t, ref, p, s, 24)


def test_norms_elsewhere_dropout_on_the_sparse_layer_tied_weights_and_emphasis_f32_w24_b70():
    import emphasis_ref as ER
    from codae.tool import HiddenDropout, LossEmphasis
    p = _square(5, 24, 70, "leaky", seed=61)
    drop = HiddenDropout([0.0, 0.0, 0.5, 0.0], seed=77)
    t = _trainer(p, "f32", norm=_norm("layer", layers=[0, 1, 3]), hidden_dropout=drop, tied_weights=True, loss_emphasis=LossEmphasis(3.0, 1.0),
                 sparse_code=_sparse(6, layer=3))
    ref = SR.StepRef(p["params"], p["names"], [0] * 5, [1, 1, 0, 1, 0], "layer", EPS, 1e-3, 1e-4, 2, 6, tied=True)
    for s in range(2):
        idx = p["order"][s]
        fm = _fmask(p, idx)
        factors = [None, None, drop.factor(idx, 2, 24, s + 1, n_layers=5), None]
        w = ER.weights(ER.corrupted(fm, idx, s + 1, None), 3.0, 1.0)
        _check_f32_step(t, ref, p, s, 24, dy_of=SR.mse(p["data"][idx], w), factors=factors)


def test_skips_norms_and_dropout_around_a_half_chunk_wide_code_f32_w20_b70():
    """width 20 = 4 (mod 8): every row-wise kernel of the step - residual, norm, dropout, sparse - ends its rows in half a chunk"""
    from codae.tool import HiddenDropout
    p = _square(5, 20, 70, "leaky", S=4, seed=63)
    drop = HiddenDropout([0.0, 0.0, 0.5, 0.0], seed=77)
    t = _trainer(p, "f32", residual=_res([1, 3]), norm=_norm("layer", layers=[0, 3]), hidden_dropout=drop, sparse_code=_sparse(5, layer=3))
    assert t.engine.sparse_resolved == (2, 20) and t.engine.residual_layers == [1, 3] and t.engine.norm_layers == [0, 3]
    ref = SR.StepRef(p["params"], p["names"], [0, 1, 0, 1, 0], [1, 0, 0, 1, 0], "layer", EPS, 1e-3, 1e-4, 2, 5)
    for s in range(2):
        idx = p["order"][s]
        factors = [None, None, drop.factor(idx, 2, 20, s + 1, n_layers=5), None]
        _check_f32_step(t, ref, p, s, 20, factors=factors)


def test_swap_noise_and_slot_cosine_f32_w24_b70():
    import recon_loss_ref as CR
    import swap_ref as SWR
    from codae.tool import InputNoise, ReconstructionLoss
    p = _square(4, 24, 70, "relu", seed=62)
    t = _trainer(p, "f32", norm=_norm("rms", layers=[0, 2]), input_noise=InputNoise("swap", p=0.4, seed=9),
                 criterion=ReconstructionLoss("slot_cosine", mse_weight=0.1), sparse_code=_sparse(6, layer=2))
    ref = SR.StepRef(p["params"], p["names"], [0] * 4, [1, 0, 1, 0], "rms", EPS, 1e-3, 1e-4, 1, 6)
    for s in range(2):
        idx = p["order"][s]
        x = p["data"][idx]
        fm = _fmask(p, idx)
        c, cls = SWR.corrupt(x, p["data"], idx, s + 1, p["S"], 0.4, 9, keep=fm)
        assert (cls == 3).sum() > 0

        def dy_of(y, x=x, fm=fm):
            tt = CR.loss_terms("slot_cosine", x, y.astype(np.float32), fm, None, 1.0 / x.size, mse_weight=0.1, S=p["S"])
            return tt["dy"], tt["loss"]
        _check_f32_step(t, ref, p, s, 24, c=c, dy_of=dy_of)


# ---- the same bits on every form ------------------------------------------------------------------------------------------------

def _bits_snapshot(t, B):
    return t.engine.sparse_bits(B).clone()


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_two_runs_and_graph_replay_give_the_same_bits_w24_b70(precision):
    from codae.tool import HiddenDropout
    p = _problem([24] * 6, CODE, 70, seed=51)
    runs = []
    for kw in (dict(), dict(), dict(use_graph=True)):
        t = _trainer(p, precision, residual=_res([1, 3]), hidden_dropout=HiddenDropout([0.0, 0.0, 0.5, 0.0], seed=5), sparse_code=_sparse(6), **kw)
        for s in range(4):
            t.train_batch(_idx(p, s), run=0)
        runs.append((_snapshot(t), _bits_snapshot(t, 70)))
    assert float(runs[0][0]["grads"].abs().max()) > 0
    for other in runs[1:]:
        _same(other[0], runs[0][0])
        assert torch.equal(other[1], runs[0][1])


def test_bucketed_backward_keeps_the_mask_between_the_range_calls_w24_b70():
    """forward + loss, the backward layer by layer without joins, the update: the bits of the fused step"""
    p = _problem([24] * 6, CODE, 70, seed=52)
    mk = lambda: _trainer(p, "f32", residual=_res([1, 3]), sparse_code=_sparse(6))
    a, b = mk(), mk()
    a.train_batch(_idx(p, 0), run=0)
    eng = b.engine
    batch = b._batch(_idx(p, 0), 0)
    hyper = eng.hyper(b.lr, b.weight_decay, b.clip, global_rows=70)
    eng.step_forward_loss(batch, hyper)
    for l in range(4, -1, -1):
        eng.step_backward(70, l, l + 1, join=False)
    eng.step_update(hyper)
    sa, sb = _snapshot(a), _snapshot(b)
    for k in ("grads", "params", "m", "v"):
        assert torch.equal(sa[k].view(torch.int32), sb[k].view(torch.int32)), k
    assert torch.equal(_bits_snapshot(a, 70), _bits_snapshot(b, 70))


def test_eighteen_layers_rotate_the_gradient_buffers_f32_w16_b70():
    p = _square(18, 16, 70, "leaky", S=2, seed=53)
    t = _trainer(p, "f32", residual=_res([l for l in range(1, 17) if l != 8]), sparse_code=_sparse(4, layer=9))
    skips = [1 if (1 <= l <= 16 and l != 8) else 0 for l in range(18)]
    ref = SR.StepRef(p["params"], p["names"], skips, [0] * 18, "layer", EPS, 1e-3, 1e-4, 8, 4)
    _check_f32_step(t, ref, p, 0, 16)
    u = _trainer(p, "f32", residual=_res([l for l in range(1, 17) if l != 8]), sparse_code=_sparse(4, layer=9))
    u.train_batch(_idx(p, 0), run=0)
    _same(_snapshot(t), _snapshot(u))


def test_off_is_off_192_b40():
    """no argument, None and keep == Z: the bits, the digest and the chain path of today's trainer"""
    p = _square(3, 192, 40, "relu", seed=54)
    plain = _trainer(p, "bf16")
    none = _trainer(p, "bf16", sparse_code=None)
    full = _trainer(p, "bf16", sparse_code=_sparse(192, layer=2))
    cleared = _trainer(p, "bf16", sparse_code=_sparse(48, layer=2))
    assert cleared.engine.step_path(40) == "layers" and cleared.engine.sparse_resolved == (1, 192)
    cleared.set_sparse_code(None)
    assert cleared.engine.sparse_resolved is None
    trainers = (plain, none, full, cleared)
    for t in trainers:
        assert t.engine.step_path(40) == "chain"
        for s in range(3):
            t.train_batch(_idx(p, s), run=0)
    ref, dig = _snapshot(plain), plain.state_digest()
    for t in trainers[1:]:
        _same(_snapshot(t), ref)
        assert t.state_digest() == dig
    q = _square(4, 24, 70, "relu", seed=55)                       # the per-layer path
    a, b = _trainer(q, "f32"), _trainer(q, "f32", sparse_code=_sparse(24, layer=2))
    for t in (a, b):
        assert t.engine.step_path(70) == "layers"
        for s in range(3):
            t.train_batch(_idx(q, s), run=0)
    _same(_snapshot(a), _snapshot(b))
    assert a.state_digest() == b.state_digest()


# ---- the model surface ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_encode_decode_and_the_code_consumers_run_through_it_w24_b70(precision):
    from codae.tool import OutfitCodes, WeightAverage
    c = 1
    p = _problem([24] * 6, CODE, 70, seed=105)
    p["mtu"][:] = c                                                # every row's mask of run 0 is the one-slot mask {c}
    keep, bf16 = 6, precision == "bf16"
    t = _trainer(p, precision, residual=_res([1, 3]), sparse_code=_sparse(keep), weight_average=WeightAverage("ema", decay=0.5))
    dense_t = _trainer(p, precision, residual=_res([1, 3]))
    for s in range(2):
        t.train_batch(_idx(p, s), run=0)
    dense_t.load_params([(w.cpu(), b.cpu()) for w, b in t.params()])
    rows = _idx(p, 0)
    code = t.encode(rows)
    assert tuple(code.shape) == (70, 24) and int((code != 0).sum(dim=1).max()) <= keep
    # ... and is the selection of the dense stack's code: bit for bit of the engine's own dense code, and a valid selection of
    # forward_to's (whole-tensor torch ops, float64)
    dense = dense_t.encode(rows, layer=3)
    stored = dense.to(torch.bfloat16) if bf16 else dense
    from codae.tool.sparse import select
    want = torch.where(select(stored, keep), dense, torch.zeros((), device=DEV))
    assert torch.equal(code.view(torch.int32), want.view(torch.int32))
    ws, bs = [w.double().cpu() for w, _ in t.params()], [b.double().cpu() for _, b in t.params()]
    if bf16:
        ws = [w.float().to(torch.bfloat16).double() for w in ws]
    x = torch.tensor(p["data"][p["order"][0]]).double()
    if bf16:
        x = x.float().to(torch.bfloat16).double()
    acts = t.engine.layer_activations()
    ref_dense = OutfitCodes.forward_to(x, ws, bs, acts, 3, residual=_res([1, 3])).numpy()
    ok, worst = SR.selection_is_valid(ref_dense, (code != 0).cpu().numpy(), keep, bf16)
    print("MEASURE %s encode: selection worst gap / allowance against forward_to %.3g" % (precision, worst))
    assert ok, worst
    # decode(encode(rows, blank=c)) has the bits of eval_batch under the mask {c}
    y = t.eval_batch(rows, run=0, want_y=True)
    for k in range(1, 5):
        z = t.encode(rows, blank=c, layer=k)
        back = t.decode(z, layer=k)
        assert torch.equal(back.view(torch.int32), y.view(torch.int32)), (k, float((back - y).abs().max()))
    assert not torch.equal(dense_t.eval_batch(rows, run=0, want_y=True).view(torch.int32), y.view(torch.int32))
    # the evaluation under the engine's own code is the restatement's (fp32: rtol 1e-3 / atol 1e-5)
    if not bf16:
        mask = (t.encode(rows, blank=c) != 0).cpu().numpy()
        cin = p["data"][p["order"][0]] * _fmask(p, p["order"][0])
        y_ref = SR.forward(_engine_params(t), p["names"], [0, 1, 0, 1, 0], [0] * 5, "layer", EPS, cin, 2, keep, mask=mask)[0]
        assert close(y.cpu().numpy(), y_ref), max_err(y.cpu().numpy(), y_ref)
    # the averaged weights, completion, outfit scores, the index and the clusters run through it
    ya = t.eval_batch(rows, run=0, want_y=True, weights="average")
    assert torch.isfinite(ya).all() and not torch.equal(ya, y)
    za = t.encode(rows, weights="average")
    assert int((za != 0).sum(dim=1).max()) <= keep
    got_idx, got_score = t.complete(torch.tensor(p["order"][2][:9]), 1, 3, distinct=False)
    plain_score = dense_t.complete(torch.tensor(p["order"][2][:9]), 1, 3, distinct=False)[1]
    assert torch.isfinite(got_score).all() and not torch.equal(got_score, plain_score)
    items = torch.tensor(np.stack([p["order"][3][:12], p["order"][3][12:24], p["order"][3][24:36]], axis=1))
    sc = t.score_outfits(items)
    assert torch.isfinite(sc["score"]).all() and not torch.equal(sc["cos"], dense_t.score_outfits(items)["cos"])
    index = t.code_index()
    assert int((index.bank != 0).sum(dim=1).max()) <= keep
    idx, score = index.similar(code[:5], 3, exclude=rows[:5])
    assert tuple(idx.shape) == (5, 3) and torch.isfinite(score).all()
    cl = index.cluster(4)
    assert cl is not None


# ---- refusals -----------------------------------------------------------------------------------------------------------------------

def test_refusals_on_the_device_path_leave_the_trainer_unchanged():
    from codae.hip import HipError
    p = _problem([24] * 6, CODE, 70, seed=81)
    a, b = _trainer(p, "f32", sparse_code=_sparse(6)), _trainer(p, "f32", sparse_code=_sparse(6))
    dig = b.state_digest()
    for bad, words in ((_sparse(25), "keep 25"), (_sparse(6, layer=5), "last layer"), (_sparse(6, layer=9), "layer")):
        with pytest.raises(HipError, match=words):
            b.set_sparse_code(bad)
        assert b.engine.sparse_resolved == (2, 24) and b.engine.sparse_code.keep == 6
    with pytest.raises(HipError, match=r"layer 2.*name the layers and leave out layer 2"):
        b.set_residual(_res("hidden"))
    with pytest.raises(HipError, match=r"layer 2.*name the layers and leave out layer 2"):
        b.set_norm(_norm("layer"))
    assert b.engine.residual_layers == [] and b.engine.norm_layers == []
    with pytest.raises(HipError, match=r"takes no skip.*name the layers and leave out layer 2"):
        _trainer(p, "f32", residual=_res("hidden"), sparse_code=_sparse(6))
    with pytest.raises(HipError, match=r"takes no norm.*name the layers and leave out layer 2"):
        _trainer(p, "f32", norm=_norm("rms"), sparse_code=_sparse(6))
    dy = torch.zeros((70, 24), device=DEV)
    b.engine.forward(torch.tensor(p["data"][:70], device=DEV))          # the whole stack: allowed, and it sparsifies
    with pytest.raises(HipError, match="a sparse code is on"):
        b.engine.backward(dy)
    with pytest.raises(HipError, match="a sparse code is on"):
        b.engine.forward(torch.tensor(p["data"][:70], device=DEV), 0, 2)
    assert b.state_digest() == dig
    for t in (a, b):
        t.train_batch(_idx(p, 0), run=0)
    _same(_snapshot(a), _snapshot(b))
    q = _square(4, 24, 70, "relu", seed=82)
    with pytest.raises(HipError, match=r"layer 1.*none, ReLU or LeakyReLU"):
        _trainer(q, "f32", activation=lambda inplace: torch.nn.ELU(), sparse_code=_sparse(6, layer=2))


# ---- checkpoint -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_checkpoint_resume_is_bit_exact_and_inference_reproduces_encode_w24_b70(tmp_path, precision):
    from codae.hip import HipError
    from codae.tool.checkpoint import read_checkpoint
    from codae.train import HipEmbeddingTrainer
    p = _problem([24] * 6, CODE, 70, seed=91)
    mk = lambda **kw: _trainer(p, precision, residual=_res([1, 3]), **kw)
    whole = mk(sparse_code=_sparse(6))
    for s in range(4):
        whole.train_batch(_idx(p, s), run=0)
    first = mk(sparse_code=_sparse(6))
    for s in range(2):
        first.train_batch(_idx(p, s), run=0)
    path = str(tmp_path / "ck.codae")
    first.save(path)
    second = mk(sparse_code=_sparse(6))
    meta = second.load(path)
    assert meta["sparse_code"] == {"keep": 6, "layer": 3}
    for s in range(2, 4):
        second.train_batch(_idx(p, s), run=0)
    a, b = _snapshot(whole), _snapshot(second)
    for k in ("params", "m", "v", "grads"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    other = mk(sparse_code=_sparse(5))
    before = _snapshot(other)
    with pytest.raises(HipError, match="sparse code: keep 6 at layer 3, this trainer has sparse code: keep 5 at layer 3"):
        other.load(path)
    _same(_snapshot(other), before)
    plain = mk()
    with pytest.raises(HipError, match="sparse code"):
        plain.load(path)
    plain_path = str(tmp_path / "plain.codae")
    plain.save(plain_path)
    assert "sparse_code" not in read_checkpoint(plain_path, verify=False)[1]          # a file of a run without it has no key
    with pytest.raises(HipError, match="sparse code"):
        mk(sparse_code=_sparse(6)).load(plain_path)
    inf = HipEmbeddingTrainer.load_for_inference(path, torch.tensor(p["data"]), torch.tensor(p["bm"]).to(torch.uint8), torch.tensor(p["mtu"]),
                                                 n_slots=p["S"], max_batch=70, device=DEV)
    assert inf.engine.sparse_resolved == (2, 24) and inf.engine.sparse_code.keep == 6
    z0, z1 = first.encode(_idx(p, 3)), inf.encode(_idx(p, 3))
    assert torch.equal(z0.view(torch.int32), z1.view(torch.int32)) and int((z1 != 0).sum(dim=1).max()) <= 6


# ---- non-finite -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_a_nan_in_one_row_makes_that_rows_outputs_and_the_loss_nan_w24_b70(precision):
    """NaN ranks first, so it is always kept: the row's outputs and the loss are NaN, and no other row's"""
    p = _problem([24] * 6, CODE, 70, seed=95)
    idx = p["order"][0]
    fm = _fmask(p, idx)
    col = int(np.flatnonzero(fm[3] == 1)[0])                    # a column the mask keeps, in batch row 3
    data = p["data"].copy()
    data[idx[3], col] = np.nan
    q = dict(p, data=data)
    t = _trainer(q, precision, sparse_code=_sparse(6))
    y = t.eval_batch(_idx(p, 0), run=0, want_y=True).cpu().numpy()
    assert np.isnan(y[3]).all() and np.isfinite(np.delete(y, 3, axis=0)).all()
    t.train_batch(_idx(p, 0), run=0)
    assert math.isnan(t.engine.read_scalars()[3])
    mask = _mask_of(t, p, 24, 6)
    assert mask.shape == (70, 24)
