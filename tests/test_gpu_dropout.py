"""Hidden dropout on a real MI355X: the two kernels (codae_dropout_fwd / codae_dropout_bwd) against the independent statement
of the definition in tests/dropout_ref.py bit for bit, whole steps of both engines against its step references, and the step
forms (off, evaluation, graph replay, the driver path, launch counts, history, refusals).

Tolerances.  Kernel values: exact bits (one fp32 product, round-to-nearest-even to bf16).  Column sums: 1e-5 sum |d| per column
(the emphasis kernel's bound: 70 fp32 additions in a fixed order cost at most 70 * 2^-24 = 4.2e-6 of sum |d|).  fp32 steps: the
project's rtol 1e-3 / atol 1e-5 against float64 autograd.  bf16 first step: test_gpu_parity.py's 2e-3 relative L2 per gradient
tensor against the restatement with the engine's roundings.
"""
import ctypes as C
import math
import re

import numpy as np
import pytest

import dropout_ref as DR
from golden_util import close, max_err
from residual_ref import colsum_parts_fixed_order

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"

SEED = 0x0123456789ABCDEF
FILL = 7.0
# (bf16, width, ld): fp32 element path, fp32 16-B path, bf16 16-B path with pad columns, bf16 element path
SHAPES = [(False, 21, 21), (False, 24, 24), (True, 72, 128), (True, 20, 20)]
SHAPE_IDS = ["f32-w21", "f32-w24", "bf16-w72-ld128", "bf16-w20"]


def _bits(t):
    return t.view({torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}[t.dtype])


def _matrix(rng, bf16, rows_alloc, width, ld, B):
    """[rows_alloc, ld] prefilled with FILL, random values in rows < B and columns < width; -> (device tensor, fp32 numpy of it)."""
    a = np.full((rows_alloc, ld), FILL, dtype=np.float32)
    a[:B, :width] = rng.standard_normal((B, width)).astype(np.float32)
    t = torch.tensor(a, device=DEV)
    if bf16:
        t = t.to(torch.bfloat16)
    return t, t.float().cpu().numpy()


def drop_fwd(t, bf16, ld, B, width, rows_t, layer, step, p, seed=SEED):
    from codae import hip
    rc = hip.lib().codae_dropout_fwd(hip.ptr(t), int(bf16), ld, B, width, hip.ptr(rows_t), layer, step, p, seed, hip.current_stream())
    torch.cuda.synchronize()
    return rc


def drop_bwd(t, bf16, ld, B, width, rows_t, layer, step, p, seed=SEED):
    """-> (rc, colsum_part [blocks, width] prefilled with FILL)"""
    from codae import hip
    blocks = hip.lib().codae_dropout_blocks(B)
    assert blocks == (B + 63) // 64
    colsum = torch.full((blocks + 1, width), FILL, dtype=torch.float32, device=DEV)
    rc = hip.lib().codae_dropout_bwd(hip.ptr(t), int(bf16), ld, B, width, hip.ptr(rows_t), layer, step, p, seed, hip.ptr(colsum),
                                     hip.current_stream())
    torch.cuda.synchronize()
    return rc, colsum


def _same_bits(got_t, want_np):
    got = got_t.float().cpu().numpy()
    return np.array_equal(got.view(np.uint32), np.asarray(want_np, dtype=np.float32).view(np.uint32))


@pytest.mark.parametrize("permuted", [True, False], ids=["row_idx", "null-rows"])
@pytest.mark.parametrize("bf16,width,ld", SHAPES, ids=SHAPE_IDS)
def test_forward_kernel_bits_equal_the_definition_b33(bf16, width, ld, permuted):
    B, layer, step, p = 33, 1, 5, 0.25
    rng = np.random.default_rng(100 + width)
    rows = rng.permutation(120)[:B].astype(np.int32) if permuted else np.arange(B, dtype=np.int32)
    rows_t = torch.tensor(rows, device=DEV) if permuted else None
    t, a = _matrix(rng, bf16, B + 2, width, ld, B)
    f = DR.factor(rows, layer, width, step, SEED, p)
    assert 0.1 < float((f == 0).mean()) < 0.4
    assert drop_fwd(t, bf16, ld, B, width, rows_t, layer, step, p) == 0
    want = a.copy()
    want[:B, :width] = DR.apply(a[:B, :width], f, bf16)
    assert _same_bits(t, want)                                  # values exact; pad columns and the rows past B keep their prefill
    assert (t[:, width:].float() == FILL).all() and (t[B:].float() == FILL).all()
    # the same rows in another batch order: the same value per dataset row
    order = rng.permutation(B)
    t2 = torch.tensor(a, device=DEV)[torch.tensor(np.concatenate([order, [B, B + 1]]), device=DEV)].contiguous()
    if bf16:
        t2 = t2.to(torch.bfloat16)
    assert drop_fwd(t2, bf16, ld, B, width, torch.tensor(rows[order], device=DEV), layer, step, p) == 0
    assert _same_bits(t2[:B], want[:B][order])
    # another layer, step or seed: other values
    for kw in (dict(layer=2), dict(step=6), dict(seed=SEED + 1)):
        args = dict(layer=layer, step=step, seed=SEED)
        args.update(kw)
        t3 = torch.tensor(a, device=DEV).to(torch.bfloat16) if bf16 else torch.tensor(a, device=DEV)
        assert drop_fwd(t3, bf16, ld, B, width, rows_t, args["layer"], args["step"], p, args["seed"]) == 0
        assert not _same_bits(t3, want), kw


def _check_backward_kernel(bf16, width, ld, B):
    """Values, pad columns and pad rows, the column sums (bound and bits), run-to-run bits, the call without column sums."""
    layer, step, p = 0, 3, 0.5
    rng = np.random.default_rng(200 + width)
    rows = rng.permutation(max(120, B + 50))[:B].astype(np.int32)
    rows_t = torch.tensor(rows, device=DEV)
    t, a = _matrix(rng, bf16, B + 2, width, ld, B)
    f = DR.factor(rows, layer, width, step, SEED, p)
    rc, colsum = drop_bwd(t, bf16, ld, B, width, rows_t, layer, step, p)
    assert rc == 0
    want = a.copy()
    want[:B, :width] = DR.apply(a[:B, :width], f, bf16)
    assert _same_bits(t, want)
    assert (t[:, width:].float() == FILL).all() and (t[B:].float() == FILL).all()
    d64 = want[:B, :width].astype(np.float64)
    cs = colsum.cpu().numpy().astype(np.float64)
    blocks = (B + 63) // 64
    assert (cs[blocks] == FILL).all()                           # one part row per 64 batch rows, none after them
    bound = 1e-5 * np.abs(d64).sum(axis=0)
    for part in range(blocks):
        err = np.abs(cs[part] - d64[64 * part:64 * part + 64].sum(axis=0))
        print("part", part, "max err / bound", float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), part
    assert (np.abs(cs[:blocks].sum(axis=0) - d64.sum(axis=0)) <= bound).all()
    # the sweep's fixed order of fp32 additions, restated: the same bits
    got_cs = np.ascontiguousarray(colsum.cpu().numpy()[:blocks]).view(np.uint32)
    assert np.array_equal(got_cs, colsum_parts_fixed_order(want[:B, :width], B).view(np.uint32))
    # the same call on the same input: the same bits (no atomics)
    t2 = torch.tensor(a, device=DEV).to(torch.bfloat16) if bf16 else torch.tensor(a, device=DEV)
    rc2, colsum2 = drop_bwd(t2, bf16, ld, B, width, rows_t, layer, step, p)
    assert rc2 == 0 and torch.equal(_bits(t), _bits(t2)) and torch.equal(_bits(colsum), _bits(colsum2))
    # without a column-sum buffer the values are the same
    from codae import hip
    t3 = torch.tensor(a, device=DEV).to(torch.bfloat16) if bf16 else torch.tensor(a, device=DEV)
    assert hip.lib().codae_dropout_bwd(hip.ptr(t3), int(bf16), ld, B, width, hip.ptr(rows_t), layer, step, p, SEED, None, hip.current_stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(t), _bits(t3))


@pytest.mark.parametrize("bf16,width,ld", SHAPES, ids=SHAPE_IDS)
def test_backward_kernel_bits_and_column_sums_b70(bf16, width, ld):
    """Two part rows, the second with six live rows."""
    _check_backward_kernel(bf16, width, ld, 70)


# the backward sweep is the residual and norm kernels' too: their widths past one column tile (512 bf16 / 256 fp32 columns, the
# bf16 one with a partial second tile), a bf16 element path with an odd ld, and their row counts around the 64-row block
@pytest.mark.parametrize("bf16,width,ld", [(True, 520, 528), (False, 264, 268), (True, 24, 27)], ids=["bf16-w520", "f32-w264", "bf16-w24-elem"])
def test_backward_kernel_past_one_column_tile_and_around_one_row_block(bf16, width, ld):
    for B in (1, 63, 64, 65, 130):
        _check_backward_kernel(bf16, width, ld, B)


@pytest.mark.parametrize("bf16,width,ld", [(False, 24, 24), (True, 72, 128)], ids=["f32-w24", "bf16-w72-ld128"])
def test_nan_and_inf_under_dropped_elements_become_nan_b70(bf16, width, ld):
    """The factor multiplies: NaN * 0 and Inf * 0 are NaN, as torch.nn.functional.dropout gives; only their own column sums see it."""
    B, layer, step, p = 70, 1, 2, 0.5
    rng = np.random.default_rng(300 + width)
    rows = rng.permutation(120)[:B].astype(np.int32)
    rows_t = torch.tensor(rows, device=DEV)
    drop = DR.dropped(rows, layer, width, step, SEED, p)
    _, a = _matrix(rng, bf16, B, width, ld, B)
    (b0, c0), (b1, c1) = [tuple(x) for x in np.argwhere(drop[:60])[[3, 40]]]        # two dropped elements of the first part row
    assert c0 != c1
    a[b0, c0], a[b1, c1] = np.nan, np.inf
    want_nan = np.zeros((B, width), dtype=bool)
    want_nan[b0, c0] = want_nan[b1, c1] = True
    mk = lambda: torch.tensor(a, device=DEV).to(torch.bfloat16) if bf16 else torch.tensor(a, device=DEV)
    t = mk()
    assert drop_fwd(t, bf16, ld, B, width, rows_t, layer, step, p) == 0
    assert np.array_equal(torch.isnan(t[:, :width]).cpu().numpy(), want_nan)
    t = mk()
    rc, colsum = drop_bwd(t, bf16, ld, B, width, rows_t, layer, step, p)
    assert rc == 0 and np.array_equal(torch.isnan(t[:, :width]).cpu().numpy(), want_nan)
    nan_cs = torch.isnan(colsum[:2]).cpu().numpy()
    want_cs = np.zeros((2, width), dtype=bool)
    want_cs[0, c0] = want_cs[0, c1] = True
    assert np.array_equal(nan_cs, want_cs)


# ---- engines ---------------------------------------------------------------------------------------------------------------

def _stack(widths, relu, B, seed, N=120):
    """Linear stack widths[0] -> ... -> widths[-1] (= widths[0]), S = 3 one-slot masks, one mask run."""
    from oracle import dae_oracle as O
    rng = np.random.default_rng(seed)
    io = widths[0]
    E = io // 3
    data = rng.random((N, io), dtype=np.float32)
    sched = [(widths[i], widths[i + 1], bool(relu[i])) for i in range(len(widths) - 1)]
    params = O.init_params(sched, rng)
    bm, nmr, _ = O.corrupter_tables([{"size": E, "position": s * E} for s in range(3)], 1)
    mtu = rng.integers(0, 3, (N, 1)).astype(np.int32)
    order = [rng.permutation(N)[:B].astype(np.int32) for _ in range(4)]
    return dict(io=io, data=data, sched=sched, params=params, bm=bm, nmr=nmr, mtu=mtu, order=order, B=B, N=N)


F32_STACK = dict(widths=(24, 40, 8, 24), relu=(True, False, False), B=33)          # ReLU, a linear code layer, the output
BF16_STACK = dict(widths=(192, 72, 64, 192), relu=(True, False, False), B=40)
NARROW = dict(widths=(192, 64, 192), relu=(True, False), B=40)                     # takes the chain kernel when nothing is on
P2 = (0.5, 0.25)


def _trainer(p, precision, **kw):
    from codae.train import HipEmbeddingTrainer
    kw.setdefault("max_batch", p["B"])
    t = HipEmbeddingTrainer(p["sched"], torch.tensor(p["data"]), torch.tensor(p["bm"]).to(torch.uint8), torch.tensor(p["mtu"]), 1e-3,
                            1e-4, 1.0, precision=precision, device=DEV, **kw)
    t.load_params(p["params"])
    return t


def _idx(p, s):
    return torch.tensor(p["order"][s], dtype=torch.int32, device=DEV)


def _drop(p=P2, seed=SEED):
    from codae.tool import HiddenDropout
    return HiddenDropout(p, seed=seed)


def _fmask(p, idx, run=0):
    from oracle import dae_oracle as O
    return O.get_masks(p["bm"], p["nmr"], p["mtu"], 1, idx, run)[1]


def _snapshot(t):
    eng = t.engine
    torch.cuda.synchronize()
    return dict(scalars=eng.read_scalars(), grads=eng.grads.clone(), params=eng.params.clone(), m=eng.adam_m.clone(), v=eng.adam_v.clone())


def _same(a, b, keys=("grads", "params", "m", "v")):
    assert a["scalars"] == b["scalars"], (a["scalars"], b["scalars"])
    for k in keys:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def _check_steps_f32(p, t, ref, inputs_of):
    """Three steps: the loss of every step, every gradient tensor of the first, the parameters after the third."""
    eng = t.engine
    for s in range(3):
        idx = p["order"][s]
        c, w = inputs_of(idx, s + 1)
        ro = ref.step(c, p["data"][idx], idx, w)
        t.train_batch(_idx(p, s), run=0)
        _, _, gsq, loss = eng.read_scalars()
        print(s, "loss", loss, ro["loss"], "gnorm", math.sqrt(gsq), ro["grad_norm"])
        assert close(loss, ro["loss"]), (s, loss, ro["loss"])
        assert close(math.sqrt(gsq), ro["grad_norm"]), (s, math.sqrt(gsq), ro["grad_norm"])
        if s == 0:
            for l, (gw, gb) in enumerate(ref.last_grads):
                print("layer", l, "dW", max_err(eng.weight_grad(l).cpu().numpy(), gw), "db", max_err(eng.bias_grad(l).cpu().numpy(), gb))
                assert close(eng.weight_grad(l).cpu().numpy(), gw), ("dW", l, max_err(eng.weight_grad(l).cpu().numpy(), gw))
                assert close(eng.bias_grad(l).cpu().numpy(), gb), ("db", l, max_err(eng.bias_grad(l).cpu().numpy(), gb))
    for l, (w_, b_) in enumerate(ref.params):
        assert close(eng.weight(l).cpu().numpy(), w_), ("W", l, max_err(eng.weight(l).cpu().numpy(), w_))
        assert close(eng.bias(l).cpu().numpy(), b_), ("b", l, max_err(eng.bias(l).cpu().numpy(), b_))


def test_f32_engine_three_steps_match_float64_autograd_24_40_8_24_b33():
    p = _stack(seed=31, **F32_STACK)
    t = _trainer(p, "f32", hidden_dropout=_drop())
    assert t.engine.step_path(33) == "layers"
    ref = DR.StepRef(p["params"], ["relu", None, None], P2, SEED, 1e-3, 1e-4)
    # the loss differs from the no-dropout loss (the comparison below is not vacuous)
    idx = p["order"][0]
    plain = DR.StepRef(p["params"], ["relu", None, None], P2, SEED, 1e-3, 1e-4).step(p["data"][idx] * _fmask(p, idx), p["data"][idx], idx, drop=False)
    plain_t = _trainer(p, "f32")
    plain_t.train_batch(_idx(p, 0), run=0)
    assert close(plain_t.engine.read_scalars()[3], plain["loss"])
    _check_steps_f32(p, t, ref, lambda idx, step: (p["data"][idx] * _fmask(p, idx), None))
    t2 = _trainer(p, "f32", hidden_dropout=_drop())
    t2.train_batch(_idx(p, 0), run=0)
    dropped_loss = t2.engine.read_scalars()[3]
    print("first loss dropped", dropped_loss, "plain", plain["loss"])
    assert abs(dropped_loss - plain["loss"]) > 0.02 * plain["loss"]


def test_f32_engine_leaky_relu_with_masking_noise_and_emphasis_24_40_8_24_b33():
    import emphasis_ref as ER
    import noise_ref as NR
    from codae.tool import InputNoise, LossEmphasis
    p = _stack(seed=32, **F32_STACK)
    nseed, alpha, beta, slot_w = 20260, 3.0, 0.5, (0.5, 1.0, 2.0)
    t = _trainer(p, "f32", activation=lambda inplace: torch.nn.LeakyReLU(0.1, inplace), input_noise=InputNoise("masking", p=0.25, seed=nseed),
                 loss_emphasis=LossEmphasis(alpha, beta, slot_weight=slot_w), hidden_dropout=_drop())
    ref = DR.StepRef(p["params"], [("leaky", 0.1), None, None], P2, SEED, 1e-3, 1e-4)
    noise = ("masking", dict(p=0.25), nseed)
    cw = np.repeat(np.float32(slot_w), p["io"] // 3)

    def inputs_of(idx, step):
        fm = _fmask(p, idx)
        c = NR.corrupt(p["data"][idx], idx, step, "masking", seed=nseed, p=0.25, keep=fm)
        return np.asarray(c, dtype=np.float32), ER.weights(ER.corrupted(fm, idx, step, noise), alpha, beta, cw)
    _check_steps_f32(p, t, ref, inputs_of)


def _rel_l2(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def test_bf16_first_step_gradients_match_the_bf16_restatement_192_72_64_192_b40():
    p = _stack(seed=33, **BF16_STACK)
    t = _trainer(p, "bf16", hidden_dropout=_drop())
    eng = t.engine
    assert eng.precision == 1 and eng.step_path(40) == "layers"
    ref = DR.StepRefBf16(p["params"], ["relu", None, None], P2, SEED, 1e-3, 1e-4)
    idx = p["order"][0]
    ro = ref.step(p["data"][idx] * _fmask(p, idx), p["data"][idx], idx)
    t.train_batch(_idx(p, 0), run=0)
    sq, _, gsq, loss = eng.read_scalars()
    print("loss", loss, ro["loss"], "gnorm", math.sqrt(gsq), ro["grad_norm"], "sq", sq, ro["sq_full"])
    for l, (gw, gb) in enumerate(ref.last_grads):
        ew, eb = _rel_l2(eng.weight_grad(l).cpu().numpy(), gw), _rel_l2(eng.bias_grad(l).cpu().numpy(), gb)
        print("layer", l, "dW", ew, "db", eb)
        assert ew <= 2e-3, ("dW", l, ew)
        assert eb <= 2e-3, ("db", l, eb)
    # ... and not those of the network without dropout
    plain = DR.StepRefBf16(p["params"], ["relu", None, None], P2, SEED, 1e-3, 1e-4)
    plain.step(p["data"][idx] * _fmask(p, idx), p["data"][idx], idx, drop=False)
    assert _rel_l2(eng.weight_grad(0).cpu().numpy(), plain.last_grads[0][0]) > 0.1


# ---- step forms ---------------------------------------------------------------------------------------------------------------

def test_off_leaves_everything_as_it_was_192_64_192_b40():
    """None, all-zero p and set-then-unset: the bits and the chain path of a plain trainer."""
    p = _stack(seed=34, **NARROW)
    plain = _trainer(p, "bf16")
    none = _trainer(p, "bf16", hidden_dropout=None)
    zero = _trainer(p, "bf16", hidden_dropout=_drop([0.0]))
    unset = _trainer(p, "bf16", hidden_dropout=_drop([0.5]))
    assert unset.engine.step_path(40) == "layers"
    unset.set_hidden_dropout(None)
    assert unset.engine.hidden_dropout is None
    trainers = (plain, none, zero, unset)
    for tr in trainers:
        assert tr.engine.step_path(40) == "chain"
        for s in range(2):
            tr.train_batch(_idx(p, s), run=0)
    ref = _snapshot(plain)
    for tr in trainers[1:]:
        _same(_snapshot(tr), ref)
    # the same on the per-layer path of the fp32 engine
    q = _stack(seed=35, **F32_STACK)
    a, b = _trainer(q, "f32"), _trainer(q, "f32", hidden_dropout=_drop())
    b.set_hidden_dropout(_drop((0.0, 0.0)))
    for tr in (a, b):
        tr.train_batch(_idx(q, 0), run=0)
    _same(_snapshot(a), _snapshot(b))


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_evaluation_and_completion_never_drop_192_72_64_192_b40(precision):
    p = _stack(seed=36, **BF16_STACK)
    plain = _trainer(p, precision)
    drop = _trainer(p, precision, hidden_dropout=_drop())

    def probe(tr):
        tr.engine.zero_metric_sums()
        y = tr.eval_batch(_idx(p, 1), run=0, want_y=True)
        loss = tr.engine.read_scalars()[3]
        sums = tr.epoch_sums(reset=True)
        top = tr.complete(_idx(p, 1)[:20], 1, 5)
        return y, sums, loss, top

    def same(a, b):
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
        assert a[1] == b[1] and a[2] == b[2]
        assert torch.equal(a[3][0], b[3][0]) and torch.equal(a[3][1], b[3][1])
    same(probe(plain), probe(drop))
    # after a dropped training step: a plain engine holding the dropped engine's parameters
    drop.train_batch(_idx(p, 0), run=0)
    plain.train_batch(_idx(p, 0), run=0)
    assert plain.engine.read_scalars()[3] != drop.engine.read_scalars()[3]             # (the training step did drop)
    plain2 = _trainer(p, precision)
    plain2.load_params([(w.clone(), b.clone()) for w, b in drop.params()])
    same(probe(plain2), probe(drop))


def test_graph_replay_gives_the_bits_of_plain_steps_192_72_64_192_b40():
    """Under replay the step of the counter comes from device memory; a change of p re-captures."""
    p = _stack(seed=37, **BF16_STACK)
    out = []
    for graph in (False, True):
        t = _trainer(p, "bf16", hidden_dropout=_drop(), use_graph=graph)
        for s in range(3):
            t.train_batch(_idx(p, s), run=0)
        out.append(_snapshot(t))
    _same(out[0], out[1])
    # it depends on the step: the same three batches with the step's factors of another seed give other bits
    t = _trainer(p, "bf16", hidden_dropout=_drop(seed=4), use_graph=True)
    for s in range(3):
        t.train_batch(_idx(p, s), run=0)
    assert not torch.equal(_snapshot(t)["params"], out[0]["params"])
    out = []
    for graph in (False, True):
        t = _trainer(p, "bf16", use_graph=graph)
        for s, pp in enumerate(((0.5, 0.25), (0.25, 0.25), None, (0.5, 0.0))):
            t.set_hidden_dropout(None if pp is None else _drop(pp))
            t.train_batch(_idx(p, s), run=0)
        out.append(_snapshot(t))
    _same(out[0], out[1])


def test_driver_path_gives_the_bits_of_train_batch_b33_b40():
    """codae_step_forward_loss + bucketed codae_step_backward + codae_step_update, as the torch.distributed drivers call them.  fp32:
    everything bit for bit.  bf16: the fused step gathers the gradient norm inside its gradient launches, in another order, so the
    loss and every gradient bit for bit there."""
    for stack, precision, steps in ((F32_STACK, "f32", 2), (BF16_STACK, "bf16", 1)):
        p = _stack(seed=38, **stack)
        B = p["B"]
        a, b = _trainer(p, precision, hidden_dropout=_drop()), _trainer(p, precision, hidden_dropout=_drop())
        eng = b.engine
        for s in range(steps):
            a.train_batch(_idx(p, s), run=0)
            batch, hyper = b._batch(_idx(p, s), 0), eng.hyper(1e-3, 1e-4, 1.0, global_rows=B)
            eng.step_forward_loss(batch, hyper)
            for lo, hi in ((2, 3), (0, 2)):
                eng.step_backward(B, lo, hi, join=False)
            if precision == "f32":
                eng.step_update(hyper)
        if precision == "f32":
            _same(_snapshot(a), _snapshot(b))
        else:
            eng.join()
            torch.cuda.synchronize()
            assert a.engine.read_scalars()[3] == eng.read_scalars()[3]
            assert torch.equal(a.engine.grads.view(torch.int32), eng.grads.view(torch.int32))


def _launch_counts(tr, idx):
    from codae.hip import KERNEL_CLASSES
    tr.engine.profile_begin(classes=KERNEL_CLASSES, max_records=512)
    tr.train_batch(idx, run=0)
    torch.cuda.synchronize()
    rec = tr.engine.profile_end()
    return {k: len(rec.get(k, [])) for k in KERNEL_CLASSES}


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_launch_counts_two_per_dropped_layer_192_72_64_192_b40(precision):
    p = _stack(seed=39, **BF16_STACK)
    tr = _trainer(p, precision)
    base = _launch_counts(tr, _idx(p, 0))
    assert base["dropout"] == 0
    for pp, n in (((0.5, 0.25), 2), ((0.0, 0.25), 1), ((0.5, 0.0), 1), ((0.0, 0.0), 0)):
        tr.set_hidden_dropout(_drop(pp))
        got = _launch_counts(tr, _idx(p, 1))
        print(pp, got)
        assert got["dropout"] == 2 * n, (pp, got)
        # every other class as without dropout
        assert {k: v for k, v in got.items() if k != "dropout"} == {k: v for k, v in base.items() if k != "dropout"}, (pp, got, base)
    tr.set_hidden_dropout(None)
    assert _launch_counts(tr, _idx(p, 2)) == base


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_a_dropped_step_after_steps_of_another_batch_size_gives_a_fresh_engines_bits(precision):
    """Widths 72 and 64 beside 192: pad columns (bf16) and pad rows must come through the dropout kernels untouched."""
    p = _stack(seed=40, **BF16_STACK)
    used = _trainer(p, precision, hidden_dropout=_drop())
    for n in (17, 40, 5):
        used.train_batch(_idx(p, 1)[:n].contiguous(), run=0)
    used.eval_batch(_idx(p, 2)[:23].contiguous(), run=0)
    eng = used.engine
    used.load_params(p["params"])
    eng.adam_m.zero_(); eng.adam_v.zero_(); eng.scalars.zero_()
    eng.step_count = 0
    fresh = _trainer(p, precision, hidden_dropout=_drop())
    for tr in (used, fresh):
        tr.train_batch(_idx(p, 0)[:33].contiguous(), run=0)
    _same(_snapshot(used), _snapshot(fresh))


@pytest.mark.parametrize("values,code,word", [([1.0, 0.25], -1, "layer 0: p 1"), ([0.5, -0.25], -1, "layer 1: p -0.25"),
                                              ([float("nan"), 0.25], -1, "layer 0: p -?nan"), ([0.5], -1, "1 values for 2 hidden"),
                                              ([0.5, 0.25, 0.1], -1, "3 values for 2 hidden")],
                         ids=["p-one", "p-negative", "p-nan", "too-short", "too-long"])
def test_bad_dropout_is_refused_and_the_previous_setting_stays_192_72_64_192_b40(values, code, word):
    from codae import hip
    p = _stack(seed=41, **BF16_STACK)
    good = _drop()
    t, ref = _trainer(p, "bf16", hidden_dropout=good), _trainer(p, "bf16", hidden_dropout=good)
    arr = (C.c_float * len(values))(*values)
    st = hip.Dropout(arr, len(values), 5)
    rc = hip.lib().codae_set_hidden_dropout(t.engine._h, C.byref(st))
    assert rc == code and re.search(word, hip.lib().codae_last_error().decode()), hip.lib().codae_last_error().decode()
    with pytest.raises(hip.HipError, match=word):
        t.engine._set_dropout_values(values, 5)
    assert t.engine.hidden_dropout is good and t.engine.step_path(40) == "layers"
    for tr in (t, ref):
        tr.train_batch(_idx(p, 0), run=0)
    _same(_snapshot(t), _snapshot(ref))
    with pytest.raises(hip.HipError):
        t.engine.set_hidden_dropout("dropout")
    # the stand-alone launchers refuse a bad p too and write nothing
    bad = [v for v in values if not 0.0 <= v < 1.0]
    if bad:
        a = torch.full((4, 8), FILL, dtype=torch.float32, device=DEV)
        assert drop_fwd(a, False, 8, 4, 8, None, 0, 1, bad[0]) == -1
        rc, colsum = drop_bwd(a, False, 8, 4, 8, None, 0, 1, bad[0])
        assert rc == -1 and (a == FILL).all() and (colsum == FILL).all()


def test_dropout_behind_elu_is_unsupported_and_names_the_layer_192_64_192_b40():
    from codae import hip
    p = _stack(seed=42, **NARROW)
    t, ref = (_trainer(p, "bf16", activation=torch.nn.ELU) for _ in range(2))
    st = hip.Dropout((C.c_float * 1)(0.5), 1, 0)
    rc = hip.lib().codae_set_hidden_dropout(t.engine._h, C.byref(st))
    assert rc == -3 and "layer 0" in hip.lib().codae_last_error().decode()
    with pytest.raises(hip.HipError, match="layer 0"):
        t.set_hidden_dropout(_drop([0.5]))
    assert t.engine.hidden_dropout is None
    t.set_hidden_dropout(_drop([0.0]))                          # nothing dropped: nothing to refuse
    for tr in (t, ref):
        tr.train_batch(_idx(p, 0), run=0)
    _same(_snapshot(t), _snapshot(ref))
    # the linear code layer behind an ELU stack is fine: (ELU, none, none) with p on layer 1 only
    q = _stack(seed=43, **BF16_STACK)
    u = _trainer(q, "bf16", activation=torch.nn.ELU)
    with pytest.raises(hip.HipError, match="layer 0"):
        u.set_hidden_dropout(_drop((0.5, 0.25)))
    u.set_hidden_dropout(_drop((0.0, 0.25)))
    u.train_batch(_idx(q, 0), run=0)
    assert math.isfinite(u.engine.read_scalars()[3])
