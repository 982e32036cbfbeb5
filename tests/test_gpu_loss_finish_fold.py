"""The fused bf16 step's loss finish inside the backward's bias-finish launch (the default) against the separate one-block launch
between the loss GEMM and the first data gradient (CODAE_NO_FOLDED_LOSS_FINISH=1).

Only a launch moves: the metric sums are added in the same order by the same reduction, the norm accumulators are cleared by the
gather's first block instead of the loss-finish kernel - before the first weight gradient either way.  So everything the step
leaves behind must be EQUAL, bit for bit: read_scalars() (both metric sums, sum g^2, loss), last_loss_and_grad_norm(), gradients
and parameters after each of 3 steps, with an eval_batch between the steps (its own, unfolded loss finish runs in between).
Then a stand-alone forward-loss -> backward -> update sequence on the same engine (the unfolded path, right after folded steps:
the `norm_scalars_zero` bookkeeping), and one case with clipping off (the update takes the norm in a pass of its own)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
# every launch of the 192-wide stack on the forced pipelined tile (as tests/test_gpu_store_policy.py)
FORCED = dict(CODAE_GEMM_TILE="x", CODAE_NO_CHAIN="1", CODAE_NO_DEFER_WGRAD="1", CODAE_SINGLE_STREAM="1", CODAE_WGRAD_SPLITK="1")
STACKS = {
    "forced-3x192-B96": (3, 64, 96, 3, FORCED),
    "default-io1536-L5-B64": (3, 512, 64, 5, {}),
}


def _problem(S, E, B, n_layers, seed):
    from oracle import dae_oracle as O
    io = S * E
    rng = np.random.default_rng(seed)
    n = B + 64
    data = rng.random((n, io), dtype=np.float32)
    sched = [(io, io, l + 1 < n_layers) for l in range(n_layers)]
    params = O.init_params(sched, rng)
    bm, _, _ = O.corrupter_tables([{"size": E, "position": s * E} for s in range(S)], 1)
    mtu = rng.integers(0, S, (n, 1)).astype(np.int32)
    idx = [torch.tensor(rng.permutation(n)[:B], dtype=torch.int32, device=DEV) for _ in range(5)]
    return sched, params, torch.tensor(data), torch.tensor(bm).to(torch.uint8), torch.tensor(mtu), idx


def _snapshot(tr):
    eng = tr.engine
    return {"scalars": eng.read_scalars(), "loss_norm": tr.last_loss_and_grad_norm(), "grads": eng.grads.clone(),
            "params": eng.params.clone(), "adam_m": eng.adam_m.clone(), "adam_v": eng.adam_v.clone()}


def _run(problem, B, clip):
    from codae.train import HipEmbeddingTrainer
    sched, params, data, bm, mtu, idx = problem
    tr = HipEmbeddingTrainer(sched, data, bm, mtu, 1e-3, 1e-4, clip, max_batch=B, precision="bf16", device=DEV)
    tr.load_params(params)
    assert tr.engine.step_path(B) == "layers"
    out = []
    for s in range(3):
        tr.train_batch(idx[s], run=0)
        out.append(_snapshot(tr))
        tr.eval_batch(idx[s + 1], run=0)
        out.append({"scalars": tr.engine.read_scalars()})
    # stand-alone sequence: the loss finish is a launch of its own here under both settings
    eng = tr.engine
    batch = tr._batch(idx[4], 0)
    hyper = eng.hyper(tr.lr, tr.weight_decay, tr.clip, global_rows=batch.B)
    eng.step_forward_loss(batch, hyper)
    eng.step_backward(batch.B, 0, eng.L)
    eng.step_update(hyper)
    out.append(_snapshot(tr))
    tr.train_batch(idx[0], run=0)           # and a folded step again behind it
    out.append(_snapshot(tr))
    torch.cuda.synchronize()
    del tr
    return out


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return torch.equal(a, b)
    return a == b


@pytest.mark.parametrize("stack,clip", [("forced-3x192-B96", 1.0), ("default-io1536-L5-B64", 1.0), ("forced-3x192-B96", 0.0)],
                         ids=["forced-3x192-B96", "default-io1536-L5-B64", "forced-3x192-B96-no-clipping"])
def test_folded_loss_finish_leaves_the_bits_of_the_separate_launch(monkeypatch, stack, clip):
    from codae import hip as H
    S, E, B, n_layers, forced = STACKS[stack]
    problem = _problem(S, E, B, n_layers, 11)
    for k, v in forced.items():
        monkeypatch.setenv(k, v)
    runs = {}
    try:
        for fold in (False, True):
            if fold:
                monkeypatch.delenv("CODAE_NO_FOLDED_LOSS_FINISH", raising=False)
            else:
                monkeypatch.setenv("CODAE_NO_FOLDED_LOSS_FINISH", "1")
            runs[fold] = _run(problem, B, clip)
    finally:
        for k in list(forced) + ["CODAE_NO_FOLDED_LOSS_FINISH"]:
            monkeypatch.delenv(k, raising=False)
        H.check(H.lib().codae_reload_env())
    first, last = runs[True][0], runs[True][-1]
    assert first["scalars"][3] > 0 and float(first["grads"].abs().max()) > 0 and not torch.equal(first["params"], last["params"])
    if clip > 0:
        assert first["scalars"][2] > 0, "the step left no sum g^2"
    for i, (got, ref) in enumerate(zip(runs[True], runs[False])):
        for name in ref:
            assert _same(got[name], ref[name]), "record %d: %s differs between the folded and the separate loss finish: %r / %r" % (
                i, name, got[name] if not isinstance(got[name], torch.Tensor) else "tensor", ref[name] if not isinstance(ref[name], torch.Tensor) else "tensor")
