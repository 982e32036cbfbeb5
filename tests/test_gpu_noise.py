"""Input noise on a real MI355X: the noise-enabled gather kernels (codae_corrupt_batch) against the numpy statement of the
definition (tests/noise_ref.py), the fused training step with noise against the oracle fed the reference-noised input and
the clean target, and the step forms (graph replay, chain fall-back, evaluation, errors).

Tolerances.  MASKING / SALT_PEPPER: bit for bit.  GAUSSIAN, fp32 out: sigma 1e-5 (the device's unit normal is within 1e-5
of the float64 formulas: tools/noise_accuracy.py) + 2 fp32 ulps of |x| + sigma |n| (the product and
the sum); bf16 out: plus one bf16 ulp of the reference value.  Fused step: the project's rtol 1e-3 / atol 1e-5 in fp32,
the bounds of test_gpu_parity.py's bf16-rounding-oracle tests in bf16.
"""
import ctypes as C
import math

import numpy as np
import pytest

import noise_ref as R
from golden_util import Golden, close, max_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"

KINDS = [("masking", dict(p=0.25)), ("salt_pepper", dict(p=0.1, lo=-0.75, hi=1.5)), ("gaussian", dict(sigma=0.3))]
SEED = 0x0123456789ABCDEF


def _noise(kind, kw, seed=SEED):
    from codae.tool import InputNoise
    return InputNoise(kind, seed=seed, **kw)


def corrupt_batch(data, noise, step, row_idx=None, B=None, mask_id=None, table=None, mask_to_use=None, run=0, out_bf16=False,
                  out_ld=None, noise_rows=None):
    """codae_corrupt_batch on device tensors -> the [B, out_ld] output tensor (allocated zeroed)."""
    from codae import hip
    io = int(data.shape[1])
    B = int(row_idx.numel()) if row_idx is not None else (int(data.shape[0]) if B is None else B)
    ld = io if out_ld is None else out_ld
    out = torch.zeros((B, ld), dtype=torch.bfloat16 if out_bf16 else torch.float32, device=DEV)
    batch = hip.Batch(hip.ptr(data), hip.ptr(row_idx), hip.ptr(mask_id), hip.ptr(table), B, io, hip.ptr(mask_to_use),
                      0 if mask_to_use is None else int(mask_to_use.shape[1]), run)
    st = None if noise is None else noise.as_struct()
    hip.check(hip.lib().codae_corrupt_batch(C.byref(batch), None if st is None else C.byref(st), step, hip.ptr(noise_rows),
                                            hip.ptr(out), int(out_bf16), ld, hip.current_stream()))
    torch.cuda.synchronize()
    return out


_PROBLEMS = {}


def kernel_problem(io):
    """200 dataset rows, 67 batch rows (not a multiple of 64), 5 masks that blank one span each, a mask_to_use table with
    3 runs; shared by every kernel-level case of one width."""
    if io not in _PROBLEMS:
        rng = np.random.default_rng(1000 + io)
        N, B = 200, 67
        data = rng.standard_normal((N, io)).astype(np.float32)
        table = np.ones((5, io), dtype=np.uint8)
        w = max(1, io // 5)
        for m in range(5):
            table[m, m * w:(m + 1) * w] = 0
        _PROBLEMS[io] = dict(N=N, B=B, data=data, table=table, rows=rng.permutation(N)[:B].astype(np.int32),
                             mask_id=rng.integers(0, 5, B).astype(np.int32), mtu=rng.integers(0, 5, (N, 3)).astype(np.int32))
    return _PROBLEMS[io]


def _check_against_reference(got, x, rows, keep, step, kind, kw, out_bf16, seed=SEED):
    got32 = got.float().cpu().numpy()
    if kind == "gaussian":
        ref, mag = R.corrupt(x, rows, step, kind, seed=seed, keep=keep, **kw)
        tol = R.gaussian_tol(mag, kw["sigma"], bf16_ref=ref if out_bf16 else None)
        err = np.abs(got32 - ref)
        assert (err <= tol).all(), (float(err.max()), float((err / tol).max()))
        live = keep != 0
        assert (got32 != (torch.tensor(x).to(got.dtype).float().numpy()))[live].mean() > 0.95        # noise was applied
    else:
        ref = torch.tensor(R.corrupt(x, rows, step, kind, seed=seed, keep=keep, **kw)).to(got.dtype)
        bits = torch.int16 if out_bf16 else torch.int32
        assert torch.equal(got.contiguous().cpu().view(bits), ref.view(bits))
        assert not np.array_equal(got32, torch.tensor(x * keep).to(got.dtype).float().numpy())
    assert (got32[keep == 0] == 0).all()                                                          # blanked slots: exactly 0


@pytest.mark.parametrize("kind,kw", KINDS, ids=[k for k, _ in KINDS])
@pytest.mark.parametrize("io,out_bf16,out_ld", [(48, True, None), (72, True, 128), (44, False, None), (44, True, None), (11, False, None)],
                         ids=["x8-io48", "x8-io72-ld128", "x4-io44-f32", "x4-io44-bf16", "scalar-io11"])
def test_corrupt_batch_matches_the_definition(io, out_bf16, out_ld, kind, kw):
    p = kernel_problem(io)
    noise = _noise(kind, kw)
    data = torch.tensor(p["data"], device=DEV)
    table = torch.tensor(p["table"], device=DEV)
    rows_t = torch.tensor(p["rows"], device=DEV)
    mid_t = torch.tensor(p["mask_id"], device=DEV)
    mtu_t = torch.tensor(p["mtu"], device=DEV)
    B, step = p["B"], 5
    # (a) permuted row_idx, mask ids direct
    got = corrupt_batch(data, noise, step, row_idx=rows_t, mask_id=mid_t, table=table, out_bf16=out_bf16, out_ld=out_ld)
    _check_against_reference(got[:, :io], p["data"][p["rows"]], p["rows"], p["table"][p["mask_id"]], step, kind, kw, out_bf16)
    if out_ld is not None:
        assert (got[:, io:] == 0).all()                              # pad columns stay zero
    # (b) row_idx NULL (rows 0 .. B-1), mask ids through mask_to_use / run
    rows0 = np.arange(B)
    got = corrupt_batch(data, noise, step, B=B, table=table, mask_to_use=mtu_t, run=2, out_bf16=out_bf16, out_ld=out_ld)
    _check_against_reference(got[:, :io], p["data"][:B], rows0, p["table"][p["mtu"][:B, 2]], step, kind, kw, out_bf16)
    # (c) permuted row_idx and the device-side id lookup (id = mask_to_use[dataset row][run]); (d) no mask at all
    got = corrupt_batch(data, noise, step, row_idx=rows_t, table=table, mask_to_use=mtu_t, run=1, out_bf16=out_bf16, out_ld=out_ld)
    _check_against_reference(got[:, :io], p["data"][p["rows"]], p["rows"], p["table"][p["mtu"][p["rows"], 1]], step, kind, kw, out_bf16)
    got = corrupt_batch(data, noise, step, row_idx=rows_t, out_bf16=out_bf16, out_ld=out_ld)
    _check_against_reference(got[:, :io], p["data"][p["rows"]], p["rows"], np.ones((B, io), np.uint8), step, kind, kw, out_bf16)
    # noise off through the same entry: the plain gather
    plain = corrupt_batch(data, None, step, row_idx=rows_t, mask_id=mid_t, table=table, out_bf16=out_bf16, out_ld=out_ld)
    want = torch.tensor(p["data"][p["rows"]] * p["table"][p["mask_id"]]).to(plain.dtype)
    assert torch.equal(plain[:, :io].cpu(), want)


@pytest.mark.parametrize("kind,kw", KINDS, ids=[k for k, _ in KINDS])
def test_noise_is_keyed_by_the_dataset_row(kind, kw):
    p = kernel_problem(48)
    noise = _noise(kind, kw)
    data = torch.tensor(p["data"], device=DEV)
    table = torch.tensor(p["table"], device=DEV)
    mtu_t = torch.tensor(p["mtu"], device=DEV)
    rows = p["rows"]
    args = dict(table=table, mask_to_use=mtu_t, run=0)
    one = corrupt_batch(data, noise, 3, row_idx=torch.tensor(rows, device=DEV), **args)
    again = corrupt_batch(data, noise, 3, row_idx=torch.tensor(rows, device=DEV), **args)
    assert torch.equal(one.view(torch.int32), again.view(torch.int32))                          # the same call twice
    perm = np.random.default_rng(2).permutation(len(rows))
    other = corrupt_batch(data, noise, 3, row_idx=torch.tensor(rows[perm], device=DEV), **args)
    assert torch.equal(one[torch.tensor(perm, device=DEV)].view(torch.int32), other.view(torch.int32))   # another batch order
    halves = [corrupt_batch(data, noise, 3, row_idx=torch.tensor(np.ascontiguousarray(rows[r::2]), device=DEV), **args) for r in (0, 1)]
    for r in (0, 1):                                                                             # two data-parallel shards
        assert torch.equal(one[r::2].view(torch.int32), halves[r].view(torch.int32))
    # an already gathered batch + noise_rows (InputNoise.apply on a HIP tensor) is the same thing
    dense = torch.tensor(p["data"][rows], device=DEV)
    keep = torch.tensor(p["table"][p["mtu"][rows, 0]], device=DEV)
    assert torch.equal(noise.apply(dense, rows, 3, mask=keep).view(torch.int32), one.view(torch.int32))


def test_gaussian_streams_differ_between_steps_and_seeds():
    p = kernel_problem(48)
    kw = dict(sigma=0.3)
    data = torch.tensor(p["data"], device=DEV)
    rows_t = torch.tensor(p["rows"], device=DEV)
    base = corrupt_batch(data, _noise("gaussian", kw, seed=77), 4, row_idx=rows_t)
    next_step = corrupt_batch(data, _noise("gaussian", kw, seed=77), 5, row_idx=rows_t)
    next_seed = corrupt_batch(data, _noise("gaussian", kw, seed=78), 4, row_idx=rows_t)
    assert float((base != next_step).float().mean()) > 0.99
    assert float((base != next_seed).float().mean()) > 0.99
    hi_word = corrupt_batch(data, _noise("gaussian", kw, seed=77 + 2 ** 32), 4, row_idx=rows_t)     # the key's second word
    assert float((base != hi_word).float().mean()) > 0.99


# ---- the fused step against the oracle ----------------------------------------------------------------------------------

class NoisyOracle:
    """oracle.EmbeddingTrainer.step composed from the oracle's public functions, fed the reference-noised (and blanked) input
    `c` and the CLEAN target x."""

    def __init__(self, params, relu_flags, lr, weight_decay, quant=None):
        from oracle import dae_oracle as O
        self.O = O
        self.params = [(w.astype(np.float32).copy(), b.astype(np.float32).copy()) for w, b in params]
        self.relu, self.lr, self.wd, self.quant = list(relu_flags), lr, weight_decay, quant
        self.adam = O.adam_init(self.params)
        self.last_grads = None

    def step(self, x, c, fmask):
        O = self.O
        y, acts = O.forward(self.params, self.relu, c, keep=True, quant=self.quant)
        loss = O.mse_mean(x, y)
        grads = O.backward(self.params, self.relu, acts, O.mse_mean_grad_y(x, y), quant=self.quant)
        self.last_grads = grads
        clipped, gnorm = O.clip_grad_norm(grads, 1.0)
        self.params = O.adam_step(self.params, clipped, self.adam, self.lr, self.wd)
        se = ((x - y) ** 2).astype(np.float32)
        return {"loss": float(loss), "grad_norm": float(gnorm), "sq_full": float(np.sum(se)),
                "sq_partial": float(np.sum((1 - fmask) * se))}


def _reference_input(g, idx, run, step, noise):
    """(clean x, noised + blanked c as fp32, fmask) of one call of a golden run."""
    from oracle import dae_oracle as O
    _, fmask = O.get_masks(g["binary_masks"], g["nb_missing_per_run"], g["mask_to_use"], 1, idx, run)
    x = g["data"][idx]
    kw = {k: getattr(noise, k) for k in ("sigma", "p", "lo", "hi") if getattr(noise, k) is not None}
    c = R.corrupt(x, idx, step, noise.kind, seed=noise.seed, keep=fmask, **kw)
    if noise.kind == "gaussian":
        c = c[0].astype(np.float32)
    return x, c, fmask


def _golden_trainer(g, precision, noise):
    from codae.train import HipEmbeddingTrainer
    m = g.meta
    sched = [(w.shape[1], w.shape[0], r) for (w, _), r in zip(g.params("init"), g.relu_flags())]
    t = HipEmbeddingTrainer(sched, torch.tensor(g["data"]), torch.tensor(g["binary_masks"]).to(torch.uint8),
                            torch.tensor(g["mask_to_use"]).to(torch.int32), m["lr"], m["weight_decay"], clip=1.0,
                            max_batch=m["batch"], precision=precision, device=DEV, input_noise=noise)
    t.load_params(g.params("init"))
    return t


def _rel_l2(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _golden_noise(g, kind):
    from codae.tool import InputNoise
    if kind == "masking":
        return InputNoise("masking", p=0.25, seed=20260)
    if kind == "salt_pepper":
        return InputNoise("salt_pepper", p=0.1, lo=float(g["data"].min()), hi=float(g["data"].max()), seed=20260)
    return InputNoise("gaussian", sigma=0.05, seed=20260)


@pytest.mark.parametrize("name,steps,kind", [("embedding_wide_square", 3, "masking"), ("embedding_wide_square", 3, "salt_pepper"),
                                             ("embedding_wide_square", 3, "gaussian"), ("embedding_taper", 1, "masking")])
def test_fused_f32_step_with_noise_matches_the_oracle(name, steps, kind):
    """fp32 engine on a golden run's own batches: the oracle gets the reference-noised input, the loss target stays clean.
    MASKING / SALT_PEPPER inputs are bit-identical on both sides, so every bound of the un-noised parity tests holds: loss,
    gradient norm and metric sums at rtol 1e-3 / atol 1e-5, the first step's gradients at test_fused_first_step_grads_f32's
    bound.  GAUSSIAN inputs agree to the kernel tolerance: loss and gradient norm at rtol 1e-3."""
    g = Golden(name)
    noise = _golden_noise(g, kind)
    t = _golden_trainer(g, "f32", noise)
    eng = t.engine
    orc = NoisyOracle(g.params("init"), g.relu_flags(), g.meta["lr"], g.meta["weight_decay"])
    for s, (idx, run) in enumerate(g.calls()[:steps]):
        x, c, fmask = _reference_input(g, idx, run, s + 1, noise)
        assert not np.array_equal(c, x * fmask)
        ro = orc.step(x, c, fmask)
        eng.zero_metric_sums()
        t.train_batch(torch.tensor(idx, dtype=torch.int32, device=DEV), run=run)
        sq, sqp, gsq, loss = eng.read_scalars()
        print(name, kind, s, "loss", loss, ro["loss"], "gnorm", math.sqrt(gsq), ro["grad_norm"], "sums", sq, ro["sq_full"], sqp, ro["sq_partial"])
        assert close(loss, ro["loss"]), (s, loss, ro["loss"])
        assert close(math.sqrt(gsq), ro["grad_norm"]), (s, math.sqrt(gsq), ro["grad_norm"])
        if kind == "gaussian":
            continue
        assert close(sq, ro["sq_full"]) and close(sqp, ro["sq_partial"]), (s, sq, ro["sq_full"], sqp, ro["sq_partial"])
        if s == 0 and name == "embedding_wide_square":
            for l, (gw, gb) in enumerate(orc.last_grads):
                assert close(eng.weight_grad(l).cpu().numpy(), gw, atol=1e-8), ("dW", l, max_err(eng.weight_grad(l).cpu().numpy(), gw))
                assert close(eng.bias_grad(l).cpu().numpy(), gb, atol=1e-8), ("db", l)


@pytest.mark.parametrize("name", ["embedding_wide_square", "embedding_taper"])
def test_fused_bf16_first_step_with_masking_noise_matches_the_bf16_rounded_oracle(name):
    """The bounds test_fused_bf16_matches_bf16_rounded_oracle / ..._not_multiples_of_64 assert for the un-noised first step:
    loss 1e-6, gradient norm 1e-5, blanked-slot sum 1e-6 (relative), every gradient tensor 2e-3 relative L2."""
    from oracle import dae_oracle as O
    g = Golden(name)
    noise = _golden_noise(g, "masking")
    t = _golden_trainer(g, "bf16", noise)
    eng = t.engine
    assert eng.precision == 1 and eng.step_path(g.meta["batch"]) == "layers"
    orc = NoisyOracle(g.params("init"), g.relu_flags(), g.meta["lr"], g.meta["weight_decay"], quant=O.bf16_round)
    idx, run = g.calls()[0]
    x, c, fmask = _reference_input(g, idx, run, 1, noise)
    ro = orc.step(x, c, fmask)
    eng.zero_metric_sums()
    t.train_batch(torch.tensor(idx, dtype=torch.int32, device=DEV), run=run)
    sq, sqp, gsq, loss = eng.read_scalars()
    print(name, "loss", loss, ro["loss"], "gnorm", math.sqrt(gsq), ro["grad_norm"], "sq_partial", sqp, ro["sq_partial"])
    assert abs(loss - ro["loss"]) <= 1e-6 * ro["loss"], (loss, ro["loss"])
    assert abs(math.sqrt(gsq) - ro["grad_norm"]) <= 1e-5 * ro["grad_norm"], (math.sqrt(gsq), ro["grad_norm"])
    assert abs(sqp - ro["sq_partial"]) <= 1e-6 * ro["sq_partial"]
    for l, (gw, gb) in enumerate(orc.last_grads):
        assert _rel_l2(eng.weight_grad(l).cpu().numpy(), gw) <= 2e-3, ("dW", l)
        assert _rel_l2(eng.bias_grad(l).cpu().numpy(), gb) <= 2e-3, ("db", l)


# ---- step forms -------------------------------------------------------------------------------------------------------------

def _stack(io, n_in, n_out, B, seed, n_rows=None):
    from oracle import dae_oracle as O
    rng = np.random.default_rng(seed)
    N = n_rows or 3 * B
    S = 3
    E = io // S
    data = rng.random((N, io), dtype=np.float32)
    sched = O.layer_schedule(io, io, n_in, n_out, False, "embedding")
    params = O.init_params(sched, rng)
    bm, _, _ = O.corrupter_tables([{"size": E, "position": s * E} for s in range(S)], 1)
    mtu = rng.integers(0, S, (N, 1)).astype(np.int32)
    order = [torch.tensor(rng.permutation(N)[:B], dtype=torch.int32, device=DEV) for _ in range(4)]
    return dict(data=data, sched=sched, params=params, bm=bm, mtu=mtu, order=order, B=B)


def _trainer(p, precision="bf16", **kw):
    from codae.train import HipEmbeddingTrainer
    t = HipEmbeddingTrainer(p["sched"], torch.tensor(p["data"]), torch.tensor(p["bm"]).to(torch.uint8), torch.tensor(p["mtu"]), 1e-3,
                            1e-4, 1.0, max_batch=p["B"], precision=precision, device=DEV, **kw)
    t.load_params(p["params"])
    return t


def test_graph_replay_with_noise_gives_the_bits_of_plain_steps_width192_10layers_batch128():
    """Batch 128 on a 10-layer 192-wide stack: the launch-bound regime use_graph exists for.  Under replay the step index of
    the noise counter comes from device memory (kernel arguments are frozen at capture), and a change of noise re-captures."""
    from codae.tool import InputNoise
    p = _stack(192, 4, 4, 128, seed=11)
    assert len(p["sched"]) == 10 and all(k == 192 and n == 192 for k, n, _ in p["sched"])
    ga, gb = InputNoise("gaussian", sigma=0.1, seed=5), InputNoise("masking", p=0.25, seed=6)
    # three steps, GAUSSIAN on
    out = []
    for graph in (False, True):
        t = _trainer(p, input_noise=ga, use_graph=graph)
        for s in range(3):
            t.train_batch(p["order"][s], run=0)
        out.append((t.engine.params.clone(), t.engine.read_scalars()))
    assert out[0][1] == out[1][1], (out[0][1], out[1][1])
    assert torch.equal(out[0][0], out[1][0]), float((out[0][0] - out[1][0]).abs().max())
    # it depends on the step: replaying step 1's noise three times would not give these bits
    t = _trainer(p, input_noise=InputNoise("gaussian", sigma=0.1, seed=4), use_graph=True)
    for s in range(3):
        t.train_batch(p["order"][s], run=0)
    assert not torch.equal(t.engine.params, out[0][0])
    # the noise changes between steps: gaussian, masking, off, gaussian
    out = []
    for graph in (False, True):
        t = _trainer(p, use_graph=graph)
        for s, n in enumerate((ga, gb, None, ga)):
            t.engine.set_input_noise(n)
            t.train_batch(p["order"][s], run=0)
        out.append((t.engine.params.clone(), t.engine.read_scalars()))
    assert out[0][1] == out[1][1], (out[0][1], out[1][1])
    assert torch.equal(out[0][0], out[1][0]), float((out[0][0] - out[1][0]).abs().max())


def test_noise_keeps_the_stack_off_the_chain_kernel_and_off_restores_it_3x64_batch256():
    from codae.tool import InputNoise
    p = _stack(192, 2, 2, 256, seed=12)
    fresh = _trainer(p)
    t = _trainer(p, input_noise=InputNoise("gaussian", sigma=0.1, seed=1))
    assert fresh.engine.step_path(256) == "chain"
    assert t.engine.step_path(256) == "layers"
    t.engine.set_input_noise(None)
    assert t.engine.step_path(256) == fresh.engine.step_path(256)
    for tr in (fresh, t):
        tr.train_batch(p["order"][0], run=0)
    assert fresh.engine.read_scalars() == t.engine.read_scalars()
    assert torch.equal(fresh.engine.params, t.engine.params)
    assert torch.equal(fresh.engine.adam_v, t.engine.adam_v)


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_evaluation_and_completion_are_never_noised(precision):
    from codae.tool import InputNoise
    p = _stack(192, 2, 2, 256, seed=13)
    clean = _trainer(p, precision)
    noisy = _trainer(p, precision, input_noise=InputNoise("salt_pepper", p=0.3, lo=-1.0, hi=2.0, seed=9))
    idx = p["order"][1]
    res = []
    for tr in (clean, noisy):
        tr.engine.zero_metric_sums()
        y = tr.eval_batch(idx, run=0, want_y=True)
        sums = tr.epoch_sums(reset=False)
        top = tr.complete(idx[:50], 1, 5)
        res.append((y, sums, top))
    assert torch.equal(res[0][0].view(torch.int32), res[1][0].view(torch.int32))
    assert res[0][1] == res[1][1]
    assert torch.equal(res[0][2][0], res[1][2][0]) and torch.equal(res[0][2][1], res[1][2][1])
    # ... while the training step of the same engine is noised (the comparison above is not vacuous)
    for tr in (clean, noisy):
        tr.train_batch(idx, run=0)
    assert clean.engine.read_scalars()[3] != noisy.engine.read_scalars()[3]


def test_step_forward_loss_with_a_hyper_is_noised_like_train_step():
    """The torch.distributed data-parallel path drives codae_step_forward_loss / _backward / _update itself: its forward
    must see the same noised input as codae_train_step (same loss bits), keyed by hyper.step."""
    from codae.tool import InputNoise
    p = _stack(192, 2, 2, 256, seed=14)
    noise = InputNoise("gaussian", sigma=0.2, seed=3)
    a, b, c = _trainer(p, input_noise=noise), _trainer(p, input_noise=noise), _trainer(p)
    idx = p["order"][0]
    a.train_batch(idx, run=0)
    losses = []
    for tr, step in ((b, 1), (b, 2), (c, 1)):
        eng = tr.engine
        batch = tr._batch(idx, 0)
        eng.step_forward_loss(batch, eng.hyper(1e-3, 1e-4, 1.0, global_rows=256, step=step))
        losses.append(eng.read_scalars()[3])
    assert losses[0] == a.engine.read_scalars()[3]
    assert losses[1] != losses[0] and losses[2] != losses[0]


class _RawNoise:
    """What InputNoise refuses to build: hands a raw struct to the library's own validation."""

    def __init__(self, kind, p0, p1=0.0, p2=0.0):
        self.args = (kind, p0, p1, p2, 0)

    def as_struct(self):
        from codae import hip
        return hip.Noise(*self.args)


@pytest.mark.parametrize("raw,word", [(_RawNoise(9, 0.1), "unknown kind 9"), (_RawNoise(2, 1.5), ": p 1.5"), (_RawNoise(1, -1.0), "sigma -1"),
                                      (_RawNoise(1, float("nan")), "sigma nan"), (_RawNoise(3, float("nan"), 0.0, 1.0), ": p nan"),
                                      (_RawNoise(3, 0.1, float("inf"), 1.0), "lo inf"), (_RawNoise(3, 0.1, 0.0, float("nan")), "hi nan")],
                         ids=["kind", "p", "sigma", "nan-sigma", "nan-p", "inf-lo", "nan-hi"])
def test_bad_noise_is_refused_by_the_library_and_launches_nothing(raw, word):
    from codae.hip import HipError
    from codae.tool import InputNoise
    p = _stack(192, 2, 2, 256, seed=15)
    good = InputNoise("masking", p=0.25)
    t = _trainer(p, input_noise=good)
    with pytest.raises(HipError, match=word):
        t.engine.set_input_noise(raw)
    assert t.engine.input_noise is good and t.engine.step_path(256) == "layers"          # the previous setting stays
    data = torch.tensor(p["data"], device=DEV)
    out_before = torch.full((8, 192), 7.0, device=DEV)
    from codae import hip
    batch = hip.Batch(hip.ptr(data), None, None, None, 8, 192, None, 0, 0)
    st = raw.as_struct()
    rc = hip.lib().codae_corrupt_batch(C.byref(batch), C.byref(st), 1, None, hip.ptr(out_before), 0, 192, hip.current_stream())
    torch.cuda.synchronize()
    assert rc == -1 and word in hip.lib().codae_last_error().decode()
    assert (out_before == 7.0).all()
    with pytest.raises(HipError):
        t.engine.set_input_noise("gaussian")
