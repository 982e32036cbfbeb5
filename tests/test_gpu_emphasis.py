"""The emphasised denoising loss on a real MI355X: the loss kernel (codae_emph_loss) against the float64 statement of the
definition (tests/emphasis_ref.py), the fp32 engine with unit weights against the unweighted kernel bit for bit, whole
steps against the oracle fed the weighted dy, and the step forms (chain fall-back, graph replay, evaluation, errors).

Tolerances, against the float64 reference computed from the same fp32 inputs.  fp32 dy: rtol 1e-6, atol 0 (at most four
fp32 roundings: x - y, the weight, weight * inv_n, the product).  bf16 dy: one bf16 ulp of the reference.  Column sums:
1e-5 sum |g| per column.  Each of the three sums: relative B io 2^-24, the worst case of any order of non-negative fp32
terms.  Whole steps: the project's rtol 1e-3 / atol 1e-5 in fp32, test_gpu_parity.py's 2e-3 relative L2 per gradient
tensor of the first step in bf16.
"""
import ctypes as C
import math

import numpy as np
import pytest

import emphasis_ref as ER
from golden_util import close, max_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"

SEED = ER.SEED
NOISES = [("off", None), ("masking", dict(p=0.25)), ("salt_pepper", dict(p=0.1, lo=-0.75, hi=1.5)), ("gaussian", dict(sigma=0.3))]
ALPHA, BETA, SLOT_W = 3.0, 0.5, (0.5, 1.0, 2.0)
STEP = 5


def _noise(kind, kw, seed=SEED):
    from codae.tool import InputNoise
    return None if kw is None else InputNoise(kind, seed=seed, **kw)


def emph_loss(data, y, noise, step, alpha, beta, col_weight=None, row_idx=None, B=None, mask_id=None, table=None, mask_to_use=None,
              run=0, dy_bf16=False, dy_ld=None, inv_n=None, fill=7.0):
    """codae_emph_loss on device tensors -> (rc, dy [B, dy_ld] prefilled with `fill`, colsum_part [blocks, io], parts [blocks, 3])."""
    from codae import hip
    io = int(data.shape[1])
    B = int(row_idx.numel()) if row_idx is not None else (int(y.shape[0]) if B is None else B)
    ld = io if dy_ld is None else dy_ld
    blocks = hip.lib().codae_emph_loss_blocks(B)
    assert blocks == (B + 31) // 32
    dy = torch.full((B, ld), fill, dtype=torch.bfloat16 if dy_bf16 else torch.float32, device=DEV)
    colsum = torch.full((blocks, io), fill, dtype=torch.float32, device=DEV)
    parts = torch.full((blocks, 3), fill, dtype=torch.float64, device=DEV)
    batch = hip.Batch(hip.ptr(data), hip.ptr(row_idx), hip.ptr(mask_id), hip.ptr(table), B, io, hip.ptr(mask_to_use),
                      0 if mask_to_use is None else int(mask_to_use.shape[1]), run)
    st = None if noise is None else noise.as_struct()
    em = hip.Emphasis(alpha, beta, hip.ptr(col_weight))
    rc = hip.lib().codae_emph_loss(C.byref(batch), None if st is None else C.byref(st), step, C.byref(em), hip.ptr(y), hip.ptr(dy),
                                   int(dy_bf16), ld, (1.0 / (B * io)) if inv_n is None else inv_n, hip.ptr(colsum), hip.ptr(parts),
                                   hip.current_stream())
    torch.cuda.synchronize()
    return rc, dy, colsum, parts


def _bits(t):
    return t.view({torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}[t.dtype])


def _bf16_ulp(ref):
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.abs(ref)))
    return np.where(ref == 0, 0.0, 2.0 ** (e - 7))


def _check_against_reference(out, x, y, rows, keep, noise_ref, cw, B, io, dy_bf16, fill=7.0):
    rc, dy, colsum, parts = out
    assert rc == 0
    w = ER.weights(ER.corrupted(keep, rows, STEP, noise_ref), ALPHA, BETA, cw)
    ref = ER.loss_terms(x, y, keep, w, np.float32(1.0 / (B * io)))
    got = dy[:, :io].float().cpu().numpy().astype(np.float64)
    if dy_bf16:
        err = np.abs(got - ref["dy"])
        assert (err <= _bf16_ulp(ref["dy"])).all(), float((err / np.maximum(_bf16_ulp(ref["dy"]), 1e-300)).max())
    else:
        np.testing.assert_allclose(got, ref["dy"], rtol=1e-6, atol=0)
    assert (dy[:, io:].float() == fill).all()                                   # pad columns stay as found
    cs = colsum.cpu().numpy().astype(np.float64).sum(axis=0)
    assert (np.abs(cs - ref["colsum"]) <= 1e-5 * ref["colsum_abs"]).all(), float(np.abs(cs - ref["colsum"]).max())
    sums = parts.cpu().numpy().sum(axis=0)
    masked = (np.asarray(keep) == 0).any()
    want = (ref["wsum"], ref["sq"], ref["sqp"] if masked else 0.0)
    print("sums", sums, want)
    for g, r in zip(sums, want):
        assert abs(g - r) <= B * io * 2.0 ** -24 * r, (g, r)
    return ref


@pytest.mark.parametrize("kind,kw", NOISES, ids=[k for k, _ in NOISES])
@pytest.mark.parametrize("io,dy_bf16,dy_ld", [(24, False, None), (24, True, 64), (21, False, None)],
                         ids=["io24-f32", "io24-bf16-ld64", "scalar-io21-f32"])
def test_emph_loss_matches_the_definition_b33(io, dy_bf16, dy_ld, kind, kw):
    """120 dataset rows, 33 batch rows (two blocks, the second with one live row), 3 one-slot masks, alpha 3, beta 0.5, slot
    weights (0.5, 1, 2); the four mask routes of test_corrupt_batch_matches_the_definition.  GAUSSIAN must weight like off."""
    p = ER.problem(io)
    noise = _noise(kind, kw)
    noise_ref = None if kw is None else (kind, kw, SEED)
    B = p["B"]
    cw = np.repeat(np.float32(SLOT_W), io // 3)
    data, y = torch.tensor(p["data"], device=DEV), torch.tensor(p["y"], device=DEV)
    table, cw_t = torch.tensor(p["table"], device=DEV), torch.tensor(cw, device=DEV)
    rows_t, mid_t, mtu_t = (torch.tensor(p[k], device=DEV) for k in ("rows", "mask_id", "mtu"))
    common = dict(col_weight=cw_t, dy_bf16=dy_bf16, dy_ld=dy_ld)
    refs = []
    # (a) permuted row_idx, mask ids direct
    out = emph_loss(data, y, noise, STEP, ALPHA, BETA, row_idx=rows_t, mask_id=mid_t, table=table, **common)
    refs.append(_check_against_reference(out, p["data"][p["rows"]], p["y"], p["rows"], p["table"][p["mask_id"]], noise_ref, cw, B, io, dy_bf16))
    # (b) row_idx NULL (rows 0 .. B-1), mask ids through mask_to_use / run
    out = emph_loss(data, y, noise, STEP, ALPHA, BETA, B=B, table=table, mask_to_use=mtu_t, run=2, **common)
    _check_against_reference(out, p["data"][:B], p["y"], np.arange(B), p["table"][p["mtu"][:B, 2]], noise_ref, cw, B, io, dy_bf16)
    # (c) permuted rows and the device-side id lookup; (d) no mask at all
    out = emph_loss(data, y, noise, STEP, ALPHA, BETA, row_idx=rows_t, table=table, mask_to_use=mtu_t, run=1, **common)
    _check_against_reference(out, p["data"][p["rows"]], p["y"], p["rows"], p["table"][p["mtu"][p["rows"], 1]], noise_ref, cw, B, io, dy_bf16)
    out = emph_loss(data, y, noise, STEP, ALPHA, BETA, row_idx=rows_t, **common)
    refs.append(_check_against_reference(out, p["data"][p["rows"]], p["y"], p["rows"], np.ones((B, io), np.uint8), noise_ref, cw, B, io, dy_bf16))
    # the comparison is not vacuous: the weighted sum is far from the unweighted one, and a replacing noise moves it
    assert abs(refs[0]["wsum"] - refs[0]["sq"]) > 0.1 * refs[0]["sq"]
    off = ER.loss_terms(p["data"][p["rows"]], p["y"], np.ones((B, io)), ER.weights(np.zeros((B, io), bool), ALPHA, BETA, cw), 1.0)["wsum"]
    assert (abs(refs[1]["wsum"] - off) > 0.05 * off) == (kind in ("masking", "salt_pepper"))
    # the same call twice: the same bits (no atomics)
    one = emph_loss(data, y, noise, STEP, ALPHA, BETA, row_idx=rows_t, mask_id=mid_t, table=table, **common)
    two = emph_loss(data, y, noise, STEP, ALPHA, BETA, row_idx=rows_t, mask_id=mid_t, table=table, **common)
    for a, b in zip(one[1:], two[1:]):
        assert torch.equal(_bits(a), _bits(b))


def test_a_nan_under_weight_zero_stays_nan_b33_io24():
    """Weights multiply: alpha = 0 on a blanked element whose prediction is NaN gives NaN in dy there and in the weighted sum."""
    p = ER.problem(24)
    keep = p["table"][p["mask_id"]]
    b0 = 3
    c0 = int(np.flatnonzero(keep[b0] == 0)[2])
    y = p["y"].copy()
    y[b0, c0] = np.nan
    rc, dy, colsum, parts = emph_loss(torch.tensor(p["data"], device=DEV), torch.tensor(y, device=DEV), None, STEP, 0.0, 1.0,
                                      row_idx=torch.tensor(p["rows"], device=DEV), mask_id=torch.tensor(p["mask_id"], device=DEV),
                                      table=torch.tensor(p["table"], device=DEV))
    assert rc == 0
    bad = torch.isnan(dy).cpu().numpy()
    want = np.zeros_like(bad)
    want[b0, c0] = True
    assert np.array_equal(bad, want)
    assert (dy.cpu().numpy()[keep == 0][~want[keep == 0]] == 0).all()          # the other blanked elements: weight 0, gradient 0
    assert math.isnan(float(parts[0, 0])) and not math.isnan(float(parts[1, 0]))
    assert math.isnan(float(colsum[0, c0]))


# ---- engines ---------------------------------------------------------------------------------------------------------------

def _stack(io, z, B, seed, N=120):
    """1 + 1 layers (io -> z -> io), S = 3 one-slot masks, one mask run."""
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


def _emphasis(alpha=ALPHA, **kw):
    from codae.tool import LossEmphasis
    return LossEmphasis(alpha, BETA, slot_weight=SLOT_W, **kw)


def _masking(seed=20260):
    from codae.tool import InputNoise
    return InputNoise("masking", p=0.25, seed=seed)


def test_f32_engine_with_unit_weights_gives_the_bits_of_the_unweighted_kernel_io24_b33():
    """A weight vector of ones forces the new kernel (alpha = beta = 1 with weights counts as on); multiplying by 1.0f is exact
    and the block order is mse_loss_kernel's: the same loss, gradients, parameters and Adam state, bit for bit, after 2 steps."""
    from codae.tool import LossEmphasis
    p = _stack(24, 8, 33, seed=21)
    plain = _trainer(p, "f32")
    ones = _trainer(p, "f32", loss_emphasis=LossEmphasis(column_weight=[1.0] * 24))
    assert ones.engine.loss_emphasis is not None and not ones.engine.loss_emphasis.is_identity
    for s in range(2):
        for t in (plain, ones):
            t.train_batch(_idx(p, s), run=0)
        assert plain.engine.read_scalars() == ones.engine.read_scalars(), s
        assert torch.equal(plain.engine.grads.view(torch.int32), ones.engine.grads.view(torch.int32)), s
    for name in ("params", "adam_m", "adam_v"):
        assert torch.equal(getattr(plain.engine, name).view(torch.int32), getattr(ones.engine, name).view(torch.int32)), name


def test_default_emphasis_leaves_the_bf16_step_as_it_was_io192_b40():
    from codae.tool import LossEmphasis
    p = _stack(192, 64, 40, seed=22)
    plain = _trainer(p, "bf16")
    dflt = _trainer(p, "bf16", loss_emphasis=LossEmphasis())
    assert plain.engine.step_path(40) == dflt.engine.step_path(40) == "chain"
    for s in range(2):
        for t in (plain, dflt):
            t.train_batch(_idx(p, s), run=0)
    assert plain.engine.read_scalars() == dflt.engine.read_scalars()
    assert torch.equal(plain.engine.params.view(torch.int32), dflt.engine.params.view(torch.int32))


def _oracle(p, noise, quant=None, alpha=ALPHA):
    io = p["io"]
    return ER.EmphasisOracle(p["params"], [r for _, _, r in p["sched"]], 1e-3, 1e-4, alpha, BETA, np.repeat(np.float32(SLOT_W), io // 3),
                             noise=None if noise is None else ("masking", dict(p=noise.p), noise.seed), quant=quant)


def _fmask(p, idx, run=0):
    from oracle import dae_oracle as O
    return O.get_masks(p["bm"], p["nmr"], p["mtu"], 1, idx, run)[1]


def test_f32_steps_match_the_oracle_with_the_weighted_dy_io24_z8_b33():
    """Three steps, alpha 3, beta 0.5, slot weights (0.5, 1, 2), MASKING(0.25): the loss of every step, every gradient tensor of
    the first and the parameters after the third at rtol 1e-3 / atol 1e-5; epoch_sums() are the UNWEIGHTED sums."""
    p = _stack(24, 8, 33, seed=23)
    noise = _masking()
    t = _trainer(p, "f32", input_noise=noise, loss_emphasis=_emphasis())
    eng = t.engine
    assert eng.step_path(33) == "layers"
    orc = _oracle(p, noise)
    sq_sum = sqp_sum = 0.0
    for s in range(3):
        idx = p["order"][s]
        ro = orc.step(p["data"][idx], idx, _fmask(p, idx))
        t.train_batch(_idx(p, s), run=0)
        _, _, gsq, loss = eng.read_scalars()
        print(s, "loss", loss, ro["loss"], "unweighted", ro["unweighted_loss"], "gnorm", math.sqrt(gsq), ro["grad_norm"])
        assert close(loss, ro["loss"]), (s, loss, ro["loss"])
        assert abs(ro["loss"] - ro["unweighted_loss"]) > 0.1 * ro["loss"]
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


def _rel_l2(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def test_bf16_first_step_gradients_match_the_bf16_rounded_oracle_io192_z64_b40():
    """Every gradient tensor of the first step at test_fused_bf16_matches_bf16_rounded_oracle's 2e-3 relative L2."""
    from oracle import dae_oracle as O
    p = _stack(192, 64, 40, seed=24)
    noise = _masking()
    t = _trainer(p, "bf16", input_noise=noise, loss_emphasis=_emphasis())
    eng = t.engine
    assert eng.precision == 1 and eng.step_path(40) == "layers"
    orc = _oracle(p, noise, quant=O.bf16_round)
    idx = p["order"][0]
    ro = orc.step(p["data"][idx], idx, _fmask(p, idx))
    t.train_batch(_idx(p, 0), run=0)
    sq, sqp, gsq, loss = eng.read_scalars()
    print("loss", loss, ro["loss"], "gnorm", math.sqrt(gsq), ro["grad_norm"], "sums", sq, ro["sq_full"], sqp, ro["sq_partial"])
    for l, (gw, gb) in enumerate(orc.last_grads):
        ew, eb = _rel_l2(eng.weight_grad(l).cpu().numpy(), gw), _rel_l2(eng.bias_grad(l).cpu().numpy(), gb)
        print("layer", l, "dW", ew, "db", eb)
        assert ew <= 2e-3, ("dW", l, ew)
        assert eb <= 2e-3, ("db", l, eb)


# ---- step forms, on the io = 192 stack ----------------------------------------------------------------------------------------

def test_emphasis_keeps_the_stack_off_the_chain_kernel_and_off_restores_it_io192_b40():
    p = _stack(192, 64, 40, seed=25)
    fresh = _trainer(p, "bf16")
    t = _trainer(p, "bf16", loss_emphasis=_emphasis())
    assert fresh.engine.step_path(40) == "chain"
    assert t.engine.step_path(40) == "layers"
    t.set_loss_emphasis(None)
    assert t.engine.step_path(40) == "chain" and t.engine.loss_emphasis is None
    for tr in (fresh, t):
        tr.train_batch(_idx(p, 0), run=0)
    assert fresh.engine.read_scalars() == t.engine.read_scalars()
    assert torch.equal(fresh.engine.params.view(torch.int32), t.engine.params.view(torch.int32))


def test_graph_replay_with_emphasis_gives_the_bits_of_plain_steps_io192_b40():
    """Under replay the step index of the noise words comes from device memory; a change of alpha re-captures."""
    p = _stack(192, 64, 40, seed=26)
    out = []
    for graph in (False, True):
        t = _trainer(p, "bf16", input_noise=_masking(), loss_emphasis=_emphasis(), use_graph=graph)
        for s in range(3):
            t.train_batch(_idx(p, s), run=0)
        out.append((t.engine.params.clone(), t.engine.read_scalars()))
    assert out[0][1] == out[1][1], (out[0][1], out[1][1])
    assert torch.equal(out[0][0].view(torch.int32), out[1][0].view(torch.int32))
    # it depends on the step: another noise stream does not give these bits
    t = _trainer(p, "bf16", input_noise=_masking(seed=4), loss_emphasis=_emphasis(), use_graph=True)
    for s in range(3):
        t.train_batch(_idx(p, s), run=0)
    assert not torch.equal(t.engine.params, out[0][0])
    # alpha changes between the steps: 3, 1.5, off, 3
    out = []
    for graph in (False, True):
        t = _trainer(p, "bf16", input_noise=_masking(), use_graph=graph)
        for s, a in enumerate((3.0, 1.5, None, 3.0)):
            t.set_loss_emphasis(None if a is None else _emphasis(a))
            t.train_batch(_idx(p, s), run=0)
        out.append((t.engine.params.clone(), t.engine.read_scalars()))
    assert out[0][1] == out[1][1], (out[0][1], out[1][1])
    assert torch.equal(out[0][0].view(torch.int32), out[1][0].view(torch.int32))


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_evaluation_and_completion_are_never_weighted_io192_b40(precision):
    p = _stack(192, 64, 40, seed=27)
    plain = _trainer(p, precision)
    emph = _trainer(p, precision, loss_emphasis=_emphasis())
    res = []
    for tr in (plain, emph):
        tr.engine.zero_metric_sums()
        y = tr.eval_batch(_idx(p, 1), run=0, want_y=True)
        _, _, _, loss = tr.engine.read_scalars()
        sums = tr.epoch_sums(reset=False)
        top = tr.complete(_idx(p, 1)[:20], 1, 5)
        res.append((y, sums, loss, top))
    assert torch.equal(res[0][0].view(torch.int32), res[1][0].view(torch.int32))
    assert res[0][1] == res[1][1] and res[0][2] == res[1][2]
    assert torch.equal(res[0][3][0], res[1][3][0]) and torch.equal(res[0][3][1], res[1][3][1])
    # ... while the training step of the same engine is weighted (the comparison above is not vacuous)
    for tr in (plain, emph):
        tr.train_batch(_idx(p, 1), run=0)
    assert plain.engine.read_scalars()[3] != emph.engine.read_scalars()[3]


def test_step_forward_loss_with_a_hyper_is_weighted_like_train_step_io192_b40():
    """The torch.distributed data-parallel path drives codae_step_forward_loss / _backward / _update itself."""
    p = _stack(192, 64, 40, seed=28)
    a, b = (_trainer(p, "bf16", input_noise=_masking(), loss_emphasis=_emphasis()) for _ in range(2))
    c = _trainer(p, "bf16", input_noise=_masking())
    a.train_batch(_idx(p, 0), run=0)
    losses = []
    for tr, step in ((b, 1), (b, 2), (c, 1)):
        eng = tr.engine
        eng.step_forward_loss(tr._batch(_idx(p, 0), 0), eng.hyper(1e-3, 1e-4, 1.0, global_rows=40, step=step))
        losses.append(eng.read_scalars()[3])
    assert losses[0] == a.engine.read_scalars()[3]
    assert losses[1] != losses[0] and losses[2] != losses[0]
    # the global batch's rows scale the loss and nothing renormalises it
    b.engine.step_forward_loss(b._batch(_idx(p, 0), 0), b.engine.hyper(1e-3, 1e-4, 1.0, global_rows=80, step=1))
    assert b.engine.read_scalars()[3] == losses[0] / 2


@pytest.mark.parametrize("alpha,beta,word", [(-1.0, 1.0, "alpha -1"), (float("nan"), 1.0, "alpha nan"), (1.0, float("inf"), "beta inf"),
                                             (1.0, -0.5, "beta -0.5")], ids=["neg-alpha", "nan-alpha", "inf-beta", "neg-beta"])
def test_bad_emphasis_is_refused_by_the_library_and_launches_nothing_io192_b40(alpha, beta, word):
    from codae import hip
    p = _stack(192, 64, 40, seed=29)
    good = _emphasis()
    t = _trainer(p, "bf16", loss_emphasis=good)
    ref = _trainer(p, "bf16", loss_emphasis=good)
    bad = hip.Emphasis(alpha, beta, None)
    rc = hip.lib().codae_set_loss_emphasis(t.engine._h, C.byref(bad))
    assert rc == -1 and word in hip.lib().codae_last_error().decode()
    with pytest.raises(hip.HipError, match=word):
        t.engine._set_emphasis_struct(bad)
    assert t.engine.loss_emphasis is good and t.engine.step_path(40) == "layers"            # the previous setting and path stay
    for tr in (t, ref):
        tr.train_batch(_idx(p, 0), run=0)
    assert t.engine.read_scalars() == ref.engine.read_scalars()
    assert torch.equal(t.engine.params.view(torch.int32), ref.engine.params.view(torch.int32))
    # the stand-alone launcher refuses it too and writes nothing
    q = ER.problem(24)
    rc, dy, colsum, parts = emph_loss(torch.tensor(q["data"], device=DEV), torch.tensor(q["y"], device=DEV), None, 1, alpha, beta,
                                      row_idx=torch.tensor(q["rows"], device=DEV))
    assert rc == -1 and word in hip.lib().codae_last_error().decode()
    assert (dy == 7.0).all() and (colsum == 7.0).all() and (parts == 7.0).all()
    with pytest.raises(hip.HipError):
        t.engine.set_loss_emphasis("emphasis")
