"""Residual connections on a real MI355X (include/codae_hip.h, "Residual connections"): the two kernels on their own, bit for bit
against the definition; whole steps of both engines against tests/residual_ref.py; and every form the setting reaches - graph replay,
rotating activation-gradient buffers, off, composition with dropout / tied weights / emphasis / swap noise / slot_cosine, evaluation,
completion, outfit scores, the weight average, refusals, checkpoints and a NaN.

Tolerances.  Kernel values: exact bits (one fp32 add, one fp32 product, one rounding to the working type).  Column sums:
64 * 2^-24 * sum |D| per 64-row block, the bound of 64 fp32 additions.  fp32 steps: the project's rtol 1e-3 / atol 1e-5 against the
float64 statement.  bf16 first step: 2e-3 relative L2 per gradient tensor against the restatement with the engine's roundings
(tests/test_gpu_parity.py's bound at fixture size).
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import residual_ref as RR
from golden_util import close, max_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
POISON = 7.0
ROWS = (1, 63, 64, 65, 130)
# (bf16, width, ld): 16-byte paths of both types, the fp32 element path, a bf16 element path, and one width per type that
# crosses a backward column tile (512 bf16 / 256 fp32 columns); fp32 widths = 4 (mod 8) on the 16-byte path, whose last lane holds
# half a chunk (one quad, four live mask bits): in the first tile, with a wider ld, and in the first lane of the second 512 columns
SHAPES = [(True, 8, 16), (True, 24, 32), (False, 8, 12), (False, 24, 28), (False, 21, 23), (False, 11, 13), (True, 520, 528),
          (False, 264, 268), (True, 24, 27), (False, 12, 12), (False, 20, 24), (False, 516, 516)]
SHAPE_IDS = ["bf16-w8", "bf16-w24", "f32-w8", "f32-w24", "f32-w21-elem", "f32-w11-elem", "bf16-w520", "f32-w264", "bf16-w24-elem", "f32-w12",
             "f32-w20", "f32-w516"]


def _work(a, bf16):
    """fp32 numpy -> a device tensor of the working type, and its values widened back to fp32 numpy"""
    t = torch.tensor(np.asarray(a, dtype=np.float32), device=DEV)
    if bf16:
        t = t.to(torch.bfloat16)
    return t, t.float().cpu().numpy()


def _bits32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _round(a, bf16):
    return RR.bf16_round(a) if bf16 else np.asarray(a, dtype=np.float32)


def _matrix(rng, B, width, ld, bf16, pad_rows=2, special=True):
    a = np.full((B + pad_rows, ld), POISON, dtype=np.float32)
    a[:B, :width] = rng.standard_normal((B, width)).astype(np.float32)
    if special:
        a[:B, :width][rng.random((B, width)) < 0.15] = 0.0
        a[0, 0] = -0.0
    return _work(a, bf16)


@pytest.mark.parametrize("bf16,width,ld", SHAPES, ids=SHAPE_IDS)
def test_forward_kernel_bits_and_mask(bf16, width, ld):
    from codae import hip
    lib = hip.lib()
    rng = np.random.default_rng(width * 3 + int(bf16))
    nb = (width + 7) // 8
    for B in ROWS:
        y, a = _matrix(rng, B, width, ld, bf16)
        x, h = _matrix(rng, B, width, ld, bf16)
        if B > 1:                                                # a NaN of either sign in the activation: the mask reads the sign bit
            # (written as bit patterns on the device: a conversion may canonicalise a NaN's sign)
            raw = y.view(torch.int16 if bf16 else torch.int32)
            raw[1, 0], raw[1, 1] = (0x7FC0, 0xFFC0 - (1 << 16)) if bf16 else (0x7FC00000, 0xFFC00000 - (1 << 32))
            a = a.copy()
            a[1, 0], a[1, 1] = np.uint32(0x7FC00000).view(np.float32), np.uint32(0xFFC00000).view(np.float32)
        bits = torch.full((B + 1, nb + 1), 0xAA, dtype=torch.uint8, device=DEV)
        assert lib.codae_residual_fwd(hip.ptr(y), hip.ptr(x), int(bf16), ld, ld, B, width, hip.ptr(bits), nb + 1, hip.current_stream()) == 0
        torch.cuda.synchronize()
        want = a.copy()
        with np.errstate(invalid="ignore"):
            want[:B, :width] = _round(a[:B, :width] + h[:B, :width], bf16)
        got = y.float().cpu().numpy()
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(_bits32(got)[~nan], _bits32(want)[~nan]), (B, "values")
        assert (got[:, width:] == POISON).all() and (got[B:] == POISON).all()                     # pad columns and pad rows survive
        assert np.array_equal(x.float().cpu().numpy(), h)                                         # the input is read only
        gb = bits.cpu().numpy()
        wb = RR.packed_mask(a[:B, :width])
        assert np.array_equal(gb[:B, :nb], wb), (B, "mask")
        if B > 1:
            assert wb[1, 0] & 3 == 1                             # +NaN counts as positive, -NaN does not
        assert (gb[:B, nb] == 0xAA).all() and (gb[B] == 0xAA).all()
        # without a mask buffer: the same values
        y2, _ = _work(a, bf16)
        assert lib.codae_residual_fwd(hip.ptr(y2), hip.ptr(x), int(bf16), ld, ld, B, width, None, 0, hip.current_stream()) == 0
        torch.cuda.synchronize()
        assert np.array_equal(_bits32(y2.float().cpu().numpy())[~nan], _bits32(want)[~nan])


def _bwd(d, bf16, ld, B, width, g_in=None, g_out=None, ld_g=0, bits=None, ld_bits=0, src=None, ld_src=0, kind=0, slope=0.0, colsum=True):
    from codae import hip
    lib = hip.lib()
    blocks = lib.codae_residual_blocks(B)
    cs = torch.full((blocks + 1, width), POISON, dtype=torch.float32, device=DEV) if colsum else None
    p = (C.c_float * 3)(slope, 0.0, 0.0)
    rc = lib.codae_residual_bwd(hip.ptr(d), int(bf16), ld, B, width, hip.ptr(g_in), hip.ptr(g_out), ld_g, hip.ptr(bits), ld_bits, hip.ptr(src),
                                ld_src, kind, p, hip.ptr(cs), hip.current_stream())
    torch.cuda.synchronize()
    return rc, cs


@pytest.mark.parametrize("source", ["bits-relu", "bits-leaky", "saved-relu", "saved-leaky", "none"])
@pytest.mark.parametrize("bf16,width,ld", SHAPES, ids=SHAPE_IDS)
def test_backward_kernel_bits_and_column_sums(bf16, width, ld, source):
    from codae import hip
    rng = np.random.default_rng(width * 5 + int(bf16))
    slope = np.float32(0.1)
    nb = (width + 7) // 8
    ld_g = ld + 4 if ld % 4 == 0 else ld + 1
    for B in ROWS:
        d, u = _matrix(rng, B, width, ld, bf16, special=False)
        gi = np.full((B + 2, ld_g), POISON, dtype=np.float32)
        gi[:B, :width] = rng.standard_normal((B, width)).astype(np.float32)
        act, a = _matrix(rng, B, width, ld, bf16)                # the activation the derivative comes from
        pos = RR.positive(a[:B, :width])
        kw = {}
        if source.startswith("bits"):
            packed = np.full((B + 1, nb + 1), 0x55, dtype=np.uint8)
            packed[:B, :nb] = RR.packed_mask(a[:B, :width])
            kw = dict(bits=torch.tensor(packed, device=DEV), ld_bits=nb + 1)
        elif source.startswith("saved"):
            kw = dict(src=act, ld_src=ld)
        kind = {"relu": 1, "leaky": 2, "none": 0}[source.split("-")[-1]]
        G = (u[:B, :width] + gi[:B, :width]).astype(np.float32)  # one fp32 add
        if kind == 1:
            D = np.where(pos, G, np.float32(0))
        elif kind == 2:
            D = np.where(pos, G, (G * slope).astype(np.float32))
        else:
            D = G
        D = _round(D, bf16)
        g_in = torch.tensor(gi, device=DEV)
        g_out = torch.full_like(g_in, POISON)
        rc, cs = _bwd(d, bf16, ld, B, width, g_in=g_in, g_out=g_out, ld_g=ld_g, kind=kind, slope=float(slope), **kw)
        assert rc == 0, hip.lib().codae_last_error()
        got = d.float().cpu().numpy()
        assert np.array_equal(_bits32(got[:B, :width]), _bits32(D)), (B, "D")
        assert (got[:, width:] == POISON).all() and (got[B:] == POISON).all()
        go = g_out.cpu().numpy()
        assert np.array_equal(_bits32(go[:B, :width]), _bits32(G)), (B, "G")
        assert (go[:, width:] == POISON).all() and (go[B:] == POISON).all()
        assert np.array_equal(g_in.cpu().numpy(), gi)
        csn = cs.cpu().numpy().astype(np.float64)
        blocks = (B + 63) // 64
        assert (csn[blocks] == POISON).all()
        D64 = D.astype(np.float64)
        for k in range(blocks):
            blk = D64[64 * k:64 * k + 64]
            err = np.abs(csn[k] - blk.sum(axis=0))
            bound = 64 * 2.0 ** -24 * np.abs(blk).sum(axis=0)
            assert (err <= bound).all(), (B, k, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.array_equal(_bits32(cs.cpu().numpy()[:blocks]), _bits32(RR.colsum_parts_fixed_order(D, B))), (B, "column-sum bits")
        # G updated in place, no G at all, no column sums: the same D; the same call again: the same bits (no atomics)
        d2, _ = _work(u, bf16)
        g2 = torch.tensor(gi, device=DEV)
        rc, cs2 = _bwd(d2, bf16, ld, B, width, g_in=g2, g_out=g2, ld_g=ld_g, kind=kind, slope=float(slope), **kw)
        assert rc == 0 and torch.equal(d2.view(torch.int16 if bf16 else torch.int32), d.view(torch.int16 if bf16 else torch.int32))
        assert np.array_equal(_bits32(g2.cpu().numpy()[:B, :width]), _bits32(G)) and torch.equal(cs2.view(torch.int32), cs.view(torch.int32))
        d3, _ = _work(u, bf16)
        rc, _ = _bwd(d3, bf16, ld, B, width, g_in=g_in, ld_g=ld_g, kind=kind, slope=float(slope), colsum=False, **kw)
        assert rc == 0 and torch.equal(d3.view(torch.int16 if bf16 else torch.int32), d.view(torch.int16 if bf16 else torch.int32))
        if B == 65:
            d4, _ = _work(u, bf16)
            rc, _ = _bwd(d4, bf16, ld, B, width, kind=kind, slope=float(slope), **kw)        # no G: D from U alone
            U = u[:B, :width]
            D0 = _round(np.where(pos, U, 0 if kind == 1 else (U * slope).astype(np.float32)) if kind else U, bf16)
            assert rc == 0 and np.array_equal(_bits32(d4.float().cpu().numpy()[:B, :width]), _bits32(D0))


def test_launchers_refuse_bad_arguments():
    from codae import hip
    lib = hip.lib()
    t = torch.zeros((4, 8), device=DEV)
    b = torch.zeros((4, 1), dtype=torch.uint8, device=DEV)
    s = hip.current_stream()
    assert lib.codae_residual_fwd(hip.ptr(t), hip.ptr(t), 0, 8, 8, 4, 8, None, 0, s) != 0                      # aliased
    assert lib.codae_residual_fwd(hip.ptr(t), hip.ptr(t.clone()), 0, 4, 8, 4, 8, None, 0, s) != 0              # ld < width
    p = (C.c_float * 3)(0.1, 0, 0)
    assert lib.codae_residual_bwd(hip.ptr(t), 0, 8, 4, 8, None, None, 0, hip.ptr(b), 1, hip.ptr(t), 8, 1, p, None, s) != 0   # bits and src
    assert lib.codae_residual_bwd(hip.ptr(t), 0, 8, 4, 8, None, None, 0, hip.ptr(b), 1, None, 0, 4, p, None, s) != 0         # bits of an ELU
    assert lib.codae_residual_bwd(hip.ptr(t), 0, 8, 4, 8, hip.ptr(t), None, 4, None, 0, None, 0, 0, p, None, s) != 0          # ld_g < width


# ---- engines ---------------------------------------------------------------------------------------------------------------

LEAKY = 0.1


def _problem(L, w, B, act, S=3, seed=0, extra_rows=50, gain=1.0):
    """L square layers of width w, `act` ("relu" / "leaky") behind every layer but the last; S one-slot masks, one mask run."""
    from oracle import dae_oracle as O
    rng = np.random.default_rng(seed)
    N = B + extra_rows
    E = w // S
    assert E * S == w
    data = rng.random((N, w), dtype=np.float32)
    sched = [(w, w, True)] * (L - 1) + [(w, w, False)]
    params = [((W * np.float32(gain)).astype(np.float32), (rng.standard_normal(W.shape[0]) * 0.05).astype(np.float32))
              for W, _ in O.init_params(sched, rng)]
    bm, nmr, _ = O.corrupter_tables([{"size": E, "position": s * E} for s in range(S)], 1)
    mtu = rng.integers(0, S, (N, 1)).astype(np.int32)
    order = [rng.permutation(N)[:B].astype(np.int32) for _ in range(4)]
    names = [("leaky", LEAKY) if act == "leaky" else "relu"] * (L - 1) + [None]
    return dict(L=L, w=w, B=B, S=S, N=N, data=data, sched=sched, params=params, bm=bm, nmr=nmr, mtu=mtu, order=order, names=names, act=act)


def _trainer(p, precision, **kw):
    from codae.train import HipEmbeddingTrainer
    kw.setdefault("max_batch", p["B"])
    if p["act"] == "leaky":
        kw.setdefault("activation", lambda inplace: torch.nn.LeakyReLU(LEAKY, inplace))
    t = HipEmbeddingTrainer(p["sched"], torch.tensor(p["data"]), torch.tensor(p["bm"]).to(torch.uint8), torch.tensor(p["mtu"]), 1e-3,
                            1e-4, 1.0, precision=precision, device=DEV, n_slots=p["S"], **kw)
    t.load_params(p["params"])
    return t


def _res(layers="hidden"):
    from codae.tool import Residual
    return Residual(layers)


def _skips(p, layers):
    L = p["L"]
    return [1 if (1 <= l <= L - 2 if layers == "hidden" else l in layers) else 0 for l in range(L)]


def _idx(p, s):
    return torch.tensor(p["order"][s], dtype=torch.int32, device=DEV)


def _fmask(p, idx, run=0):
    from oracle import dae_oracle as O
    return O.get_masks(p["bm"], p["nmr"], p["mtu"], 1, idx, run)[1]


def _snapshot(t):
    eng = t.engine
    torch.cuda.synchronize()
    return dict(scalars=eng.read_scalars(), sums=t.epoch_sums(reset=False), grads=eng.grads.clone(), params=eng.params.clone(),
                m=eng.adam_m.clone(), v=eng.adam_v.clone())


def _same(a, b):
    assert a["scalars"] == b["scalars"], (a["scalars"], b["scalars"])
    assert a["sums"] == b["sums"]
    for k in ("grads", "params", "m", "v"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def _check_f32_step(p, t, ref, idx, c, dy_of, factors=None):
    """One step: the loss, every gradient tensor, the parameters after the update - rtol 1e-3 / atol 1e-5."""
    eng = t.engine
    ro = ref.step(c, dy_of, factors)
    t.train_batch(torch.tensor(idx, dtype=torch.int32, device=DEV), run=0)
    _, _, gsq, loss = eng.read_scalars()
    print("loss", loss, ro["loss"], "gnorm", math.sqrt(gsq), ro["grad_norm"])
    assert close(loss, ro["loss"]), (loss, ro["loss"])
    assert close(math.sqrt(gsq), ro["grad_norm"]), (math.sqrt(gsq), ro["grad_norm"])
    for l, (gw, gb) in enumerate(ref.last_grads):
        ew, eb = max_err(eng.weight_grad(l).cpu().numpy(), gw), max_err(eng.bias_grad(l).cpu().numpy(), gb)
        print("layer", l, "dW", ew, "db", eb)
        assert ew <= 1.0, ("dW", l, ew)
        assert eb <= 1.0, ("db", l, eb)
    for l, (w_, b_) in enumerate(ref.params):
        assert close(eng.weight(l).cpu().numpy(), w_), ("W", l, max_err(eng.weight(l).cpu().numpy(), w_))
        assert close(eng.bias(l).cpu().numpy(), b_), ("b", l, max_err(eng.bias(l).cpu().numpy(), b_))


@pytest.mark.parametrize("layers", ["hidden", [1], [0, 1]], ids=["hidden", "layer1", "layers01"])
@pytest.mark.parametrize("act", ["relu", "leaky"])
@pytest.mark.parametrize("L", [4, 5])
def test_f32_engine_step_matches_the_float64_statement_w24_b70(L, act, layers):
    p = _problem(L, 24, 70, act, seed=10 * L + len(act))
    t = _trainer(p, "f32", residual=_res(layers))
    skips = _skips(p, layers)
    assert t.engine.residual_layers == [l for l, s in enumerate(skips) if s] and t.engine.step_path(70) == "layers"
    ref = RR.StepRef(p["params"], p["names"], skips, 1e-3, 1e-4)
    for s in range(2):
        idx = p["order"][s]
        x = p["data"][idx]
        _check_f32_step(p, t, ref, idx, x * _fmask(p, idx), RR.mse(x))
    # ... and not the network without the skips
    x = p["data"][p["order"][0]]
    off = RR.gradients(p["params"], p["names"], [0] * L, x * _fmask(p, p["order"][0]), RR.mse(x))[1]
    on = RR.gradients(p["params"], p["names"], skips, x * _fmask(p, p["order"][0]), RR.mse(x))[1]
    assert abs(on - off) > 1e-3 * off


def _rel_l2(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _bf16_first_step_errors(p, layers):
    """max relative L2 error of a first-step gradient tensor against the bf16-rounded restatement; also checks the loss"""
    t = _trainer(p, "bf16", residual=_res(layers))
    skips = _skips(p, layers)
    idx = p["order"][0]
    x = p["data"][idx]
    grads, loss, _ = RR.gradients(p["params"], p["names"], skips, x * _fmask(p, idx), RR.mse(x), bf16=True)
    t.train_batch(_idx(p, 0), run=0)
    eng = t.engine
    got_loss = eng.read_scalars()[3]
    worst = 0.0
    for l, (gw, gb) in enumerate(grads):
        ew, eb = _rel_l2(eng.weight_grad(l).cpu().numpy(), gw), _rel_l2(eng.bias_grad(l).cpu().numpy(), gb)
        print("skips", layers, "layer", l, "dW", ew, "db", eb)
        worst = max(worst, ew, eb)
    print("skips", layers, "loss", got_loss, loss, "worst gradient error", worst)
    assert abs(got_loss - loss) <= 1e-3 * abs(loss)
    return worst


@pytest.mark.parametrize("L,w,B,act,layers", [(4, 24, 70, "relu", "hidden"), (5, 24, 70, "leaky", "hidden"), (4, 24, 70, "relu", [1]),
                                              (5, 24, 70, "leaky", [1]), (4, 24, 70, "relu", [0, 1])],
                         ids=["L4-relu", "L5-leaky", "L4-relu-layer1", "L5-leaky-layer1", "L4-relu-layers01"])
def test_bf16_first_step_gradients_match_the_rounded_restatement(L, w, B, act, layers):
    """Measured on MI355X: the table under "Accuracy" in DESIGN.md section 6, "Residual connections".  The last case puts a skip around
    layer 0: what is added there is act[0], which the bf16 engine gathers from the dataset's bf16 image."""
    p = _problem(L, w, B, act, seed=7 * L + len(act))
    on = _bf16_first_step_errors(p, layers)
    off = _bf16_first_step_errors(p, [])
    print("MEASURE bf16 first-step gradient error: skips on %.3e, skips off %.3e" % (on, off))
    assert on <= max(2e-3, 2 * off), (on, off)


def test_bf16_first_step_on_the_pipelined_256x192_tiles_w264_b264(monkeypatch):
    """The forced 256 x 192 tile (tests/test_gpu_gemm_plan.py's smallest route to it) with ragged edges both ways: 264 columns =
    one tile and 72 columns, 264 rows (320 padded) = one row tile and 64 rows."""
    from codae import hip
    monkeypatch.setenv("CODAE_GEMM_TILE", "x")
    monkeypatch.setenv("CODAE_NO_CHAIN", "1")                   # (the stack with skips off: per-layer launches on the same tiles)
    hip.check(hip.lib().codae_reload_env())
    try:
        p = _problem(4, 264, 264, "relu", seed=44)
        on = _bf16_first_step_errors(p, "hidden")
        off = _bf16_first_step_errors(p, [])
        print("MEASURE bf16 first-step gradient error on 256 x 192 tiles: skips on %.3e, skips off %.3e" % (on, off))
        assert on <= max(2e-3, 2 * off), (on, off)
    finally:
        monkeypatch.delenv("CODAE_GEMM_TILE")
        monkeypatch.delenv("CODAE_NO_CHAIN")
        hip.check(hip.lib().codae_reload_env())


# ---- the same bits on every form ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_two_runs_and_graph_replay_give_the_same_bits_w24_b70(precision):
    from codae.tool import HiddenDropout
    p = _problem(5, 24, 70, "relu", seed=51)
    runs = []
    for kw in (dict(), dict(), dict(use_graph=True)):
        t = _trainer(p, precision, residual=_res(), hidden_dropout=HiddenDropout([0.0, 0.5, 0.0, 0.0], seed=5), **kw)
        for s in range(4):
            t.train_batch(_idx(p, s), run=0)
        runs.append(_snapshot(t))
    assert float(runs[0]["grads"].abs().max()) > 0
    _same(runs[1], runs[0])
    _same(runs[2], runs[0])


def test_bucketed_backward_keeps_g_between_the_range_calls_w24_b70():
    """forward + loss, the backward layer by layer without joins, the update: the bits of the fused step"""
    p = _problem(5, 24, 70, "leaky", seed=52)
    a, b = _trainer(p, "f32", residual=_res()), _trainer(p, "f32", residual=_res())
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


def test_eighteen_layers_rotate_the_gradient_buffers_f32_w16_b70():
    p = _problem(18, 16, 70, "leaky", S=2, seed=53, gain=0.5)          # (sixteen skips in a row: keep the sum's magnitude near 1)
    t = _trainer(p, "f32", residual=_res())
    skips = _skips(p, "hidden")
    assert sum(skips) == 16
    ref = RR.StepRef(p["params"], p["names"], skips, 1e-3, 1e-4)
    idx = p["order"][0]
    x = p["data"][idx]
    _check_f32_step(p, t, ref, idx, x * _fmask(p, idx), RR.mse(x))


def test_off_is_off_192_b40():
    """residual=None, Residual([]), no argument and set-then-cleared: the bits and the chain path of today's trainer"""
    p = _problem(3, 192, 40, "relu", seed=54)
    plain = _trainer(p, "bf16")
    none = _trainer(p, "bf16", residual=None)
    empty = _trainer(p, "bf16", residual=_res([]))
    cleared = _trainer(p, "bf16", residual=_res([1]))
    assert cleared.engine.step_path(40) == "layers" and cleared.engine.residual_layers == [1]
    cleared.set_residual(None)
    assert cleared.engine.residual_layers == []
    trainers = (plain, none, empty, cleared)
    for t in trainers:
        assert t.engine.step_path(40) == "chain"
        for s in range(3):
            t.train_batch(_idx(p, s), run=0)
    ref = _snapshot(plain)
    for t in trainers[1:]:
        _same(_snapshot(t), ref)
    q = _problem(4, 24, 70, "relu", seed=55)
    a, b = _trainer(q, "f32"), _trainer(q, "f32", residual=_res())
    b.set_residual(_res([]))
    for t in (a, b):
        for s in range(3):
            t.train_batch(_idx(q, s), run=0)
    _same(_snapshot(a), _snapshot(b))


# ---- composition ------------------------------------------------------------------------------------------------------------------

def test_skips_with_dropout_tied_weights_and_emphasis_f32_w24_b70():
    import emphasis_ref as ER
    from codae.tool import HiddenDropout, LossEmphasis
    p = _problem(5, 24, 70, "leaky", seed=61)
    drop = HiddenDropout([0.0, 0.5, 0.5, 0.5], seed=77)
    t = _trainer(p, "f32", residual=_res(), hidden_dropout=drop, tied_weights=True, loss_emphasis=LossEmphasis(3.0, 1.0))
    ref = RR.StepRef(p["params"], p["names"], _skips(p, "hidden"), 1e-3, 1e-4, tied=True)
    for s in range(2):
        idx = p["order"][s]
        x = p["data"][idx]
        fm = _fmask(p, idx)
        factors = [None] + [drop.factor(idx, l, 24, s + 1, n_layers=5) for l in (1, 2, 3)]
        w = ER.weights(ER.corrupted(fm, idx, s + 1, None), 3.0, 1.0)
        _check_f32_step(p, t, ref, idx, x * fm, RR.mse(x, w), factors)


def test_skips_with_swap_noise_and_slot_cosine_f32_w24_b70():
    import recon_loss_ref as CR
    import swap_ref as SR
    from codae.tool import InputNoise, ReconstructionLoss
    p = _problem(4, 24, 70, "relu", seed=62)
    t = _trainer(p, "f32", residual=_res(), input_noise=InputNoise("swap", p=0.4, seed=9), criterion=ReconstructionLoss("slot_cosine", mse_weight=0.1))
    ref = RR.StepRef(p["params"], p["names"], _skips(p, "hidden"), 1e-3, 1e-4)
    for s in range(2):
        idx = p["order"][s]
        x = p["data"][idx]
        fm = _fmask(p, idx)
        c, cls = SR.corrupt(x, p["data"], idx, s + 1, p["S"], 0.4, 9, keep=fm)
        assert (cls == 3).sum() > 0

        def dy_of(y, x=x, fm=fm):
            tt = CR.loss_terms("slot_cosine", x, y.astype(np.float32), fm, None, 1.0 / x.size, mse_weight=0.1, S=p["S"])
            return tt["dy"], tt["loss"]
        _check_f32_step(p, t, ref, idx, c, dy_of)


# ---- evaluation ---------------------------------------------------------------------------------------------------------------------

def test_evaluation_completion_scores_and_the_average_run_through_the_skips_f32_w24_b70():
    from codae.tool import Residual, WeightAverage
    p = _problem(5, 24, 70, "relu", seed=71)
    t = _trainer(p, "f32", residual=_res(), weight_average=WeightAverage("ema", decay=0.5))
    for s in range(2):
        t.train_batch(_idx(p, s), run=0)
    idx = p["order"][2]
    acts = [True] * 4 + [False]

    def torch_forward(params):
        x = torch.tensor(p["data"][idx] * _fmask(p, idx), dtype=torch.float64)
        return Residual("hidden").forward(x, [w.double().cpu() for w, _ in params], [b.double().cpu() for _, b in params], acts).numpy()
    y = t.eval_batch(_idx(p, 2), run=0, want_y=True).cpu().numpy()
    want = torch_forward(t.params())
    assert close(y, want), max_err(y, want)
    plain = RR.forward([(w.cpu().numpy(), b.cpu().numpy()) for w, b in t.params()], p["names"], [0] * 5, p["data"][idx] * _fmask(p, idx))[0]
    assert not close(y, plain)
    ya = t.eval_batch(_idx(p, 2), run=0, want_y=True, weights="average").cpu().numpy()
    want_a = torch_forward(t.params(average=True))
    assert close(ya, want_a), max_err(ya, want_a)
    assert not close(ya, y)
    # complete(): the top-k of that output's blanked slot against the resident items
    k, slot, E = 3, 1, 8
    rows = _idx(p, 2)[:9]
    got_idx, got_score = t.complete(rows, slot, k)
    mid = torch.full((9,), slot, dtype=torch.int32, device=DEV)
    yq = torch.empty((9, 24), dtype=torch.float32, device=DEV)
    t.engine.eval_step(t.engine.make_batch(t.data, rows, mid, t.mask_table), yq)
    q = torch.nn.functional.normalize(yq[:, slot * E:(slot + 1) * E].double(), dim=1)
    inv = torch.nn.functional.normalize(t.data[:, slot * E:(slot + 1) * E].double(), dim=1)
    cos = q @ inv.T
    top = cos.topk(k, dim=1)
    assert torch.allclose(got_score.double(), top.values, atol=1e-5)
    assert torch.equal(torch.gather(cos, 1, got_idx), torch.gather(cos, 1, top.indices)) or torch.allclose(
        torch.gather(cos, 1, got_idx), top.values, atol=1e-6)
    # score_outfits: an outfit alone and inside a chunk give the same bits
    items = torch.tensor(np.stack([p["order"][3][:12], p["order"][3][12:24], p["order"][3][24:36]], axis=1), dtype=torch.int32)
    whole = t.score_outfits(items)
    for qi in (0, 5, 11):
        one = t.score_outfits(items[qi:qi + 1])
        for key in ("score", "cos", "sq"):
            assert torch.equal(one[key].view(torch.int32), whole[key][qi:qi + 1].view(torch.int32)), (qi, key)
    # ... and they are those of the network with the skips
    no_skip = _trainer(p, "f32")
    no_skip.load_params([(w.cpu(), b.cpu()) for w, b in t.params()])
    assert not torch.equal(no_skip.score_outfits(items)["cos"], whole["cos"])


# ---- refusals -----------------------------------------------------------------------------------------------------------------------

def test_refusals_on_the_device_path_leave_the_trainer_unchanged():
    from codae.hip import HipError
    from oracle import dae_oracle as O
    p = _problem(4, 24, 70, "relu", seed=81)
    a, b = _trainer(p, "f32", residual=_res([1])), _trainer(p, "f32", residual=_res([1]))
    with pytest.raises(HipError, match="layer 3.*last layer"):
        b.set_residual(_res([3]))
    assert b.engine.residual_layers == [1]
    dy = torch.zeros((70, 24), device=DEV)
    b.engine.forward(torch.tensor(p["data"][:70], device=DEV))          # the whole stack: allowed, and it adds the skip
    with pytest.raises(HipError, match="residual connections are on"):
        b.engine.backward(dy)
    with pytest.raises(HipError, match="residual connections are on"):
        b.engine.forward(torch.tensor(p["data"][:70], device=DEV), 0, 2)
    for t in (a, b):
        t.train_batch(_idx(p, 0), run=0)
    _same(_snapshot(a), _snapshot(b))
    # a taper: unequal widths, on the library's own check (the message names the layer and the widths)
    rng = np.random.default_rng(82)
    sched = [(24, 24, True), (24, 12, True), (12, 24, True), (24, 24, False)]
    q = dict(p, sched=sched, params=O.init_params(sched, rng))
    with pytest.raises(HipError, match=r"layer 1.*equal widths"):
        _trainer(q, "f32", residual=_res([1]))
    t = _trainer(q, "f32")
    flags = (C.c_uint8 * 4)(0, 1, 0, 0)
    from codae import hip
    st = hip.ResidualFlags(4, flags)
    assert hip.lib().codae_set_residual(t.engine._h, C.byref(st), None, 0) == -3 and b"layer 1" in hip.lib().codae_last_error()
    # a Softplus layer
    with pytest.raises(HipError, match=r"layer 1.*none, ReLU or LeakyReLU"):
        _trainer(dict(p, act="softplus"), "f32", activation=lambda inplace: torch.nn.Softplus(), residual=_res([1]))
    st = hip.ResidualFlags(4, flags)
    sp = _trainer(dict(p, act="softplus"), "f32", activation=lambda inplace: torch.nn.Softplus())
    assert hip.lib().codae_set_residual(sp.engine._h, C.byref(st), None, 0) == -3 and b"layer 1" in hip.lib().codae_last_error()
    assert hip.lib().codae_residual_ws_bytes(sp.engine._h, C.byref(st)) == -1


# ---- checkpoint -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_checkpoint_resume_is_bit_exact_with_skips_and_dropout_w24_b70(tmp_path, precision):
    from codae.hip import HipError
    from codae.tool import HiddenDropout
    from codae.train import HipEmbeddingTrainer
    p = _problem(5, 24, 70, "relu", seed=91)
    mk = lambda **kw: _trainer(p, precision, hidden_dropout=HiddenDropout(0.25, seed=3), **kw)
    whole = mk(residual=_res())
    for s in range(4):
        whole.train_batch(_idx(p, s), run=0)
    first = mk(residual=_res())
    for s in range(2):
        first.train_batch(_idx(p, s), run=0)
    path = str(tmp_path / "ck.codae")
    first.save(path)
    second = mk(residual=_res())
    meta = second.load(path)
    assert meta["residual"] == [1, 2, 3]
    for s in range(2, 4):
        second.train_batch(_idx(p, s), run=0)
    a, b = _snapshot(whole), _snapshot(second)
    for k in ("params", "m", "v", "grads"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert a["scalars"][2:] == b["scalars"][2:]
    before = _snapshot(mk())
    other = mk()
    with pytest.raises(HipError, match="residual"):
        other.load(path)
    _same(_snapshot(other), before)
    with pytest.raises(HipError, match="residual"):
        mk(residual=_res([1])).load(path)
    inf = HipEmbeddingTrainer.load_for_inference(path, torch.tensor(p["data"]), torch.tensor(p["bm"]).to(torch.uint8), torch.tensor(p["mtu"]),
                                                 n_slots=p["S"], max_batch=70, device=DEV)
    assert inf.engine.residual_layers == [1, 2, 3]
    y0 = first.eval_batch(_idx(p, 3), run=0, want_y=True)
    y1 = inf.eval_batch(_idx(p, 3), run=0, want_y=True)
    assert torch.equal(y0.view(torch.int32), y1.view(torch.int32))


# ---- non-finite -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_a_nan_in_a_skipped_layers_activation_reaches_the_loss_w24_b70(precision):
    p = _problem(5, 24, 70, "relu", seed=95)
    params = [(W.copy(), b.copy()) for W, b in p["params"]]
    params[2][1][5] = np.nan                                    # one NaN column in a_2, a skipped layer's activation
    q = dict(p, params=params)
    idx = p["order"][0]
    x = p["data"][idx]
    ref_loss = RR.gradients(params, p["names"], _skips(p, "hidden"), x * _fmask(p, idx), RR.mse(x), bf16=precision == "bf16")[1]
    assert not math.isfinite(ref_loss)
    t = _trainer(q, precision, residual=_res())
    t.train_batch(_idx(p, 0), run=0)
    loss = t.engine.read_scalars()[3]
    assert not math.isfinite(loss), loss
    y = t.eval_batch(_idx(p, 0), run=0, want_y=True)
    assert bool(torch.isnan(y).any())
