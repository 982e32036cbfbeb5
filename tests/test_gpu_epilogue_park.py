"""The pipelined bf16 GEMM parks what its epilogue needs beside the accumulators - the tile's bias slice and, for the data
gradient, the tile of the 1-bit ReLU mask - in LDS by LDS-DMA issued at kernel entry (gemm_bf16_pipe.hip).
What can go wrong is a wrong slice (column tile other than the first), a wrong clamp (ragged M / N, bit rows that end inside
the tile's 24 bytes) or a race on the new LDS region.  Shapes are the smallest that reach each of those: a second row tile
of 8 rows, a second column tile of 8 or 24 columns, one 8 x 8 tile, three tiles each way.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    from codae import hip as H
    H.lib()
    return H


@pytest.fixture
def env(monkeypatch, hip):
    """set CODAE_* switches for one test (read by the library at codae_reload_env / codae_create), restored afterwards"""
    names = []

    def set_env(**kw):
        for k, v in kw.items():
            names.append(k)
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, v)
        hip.check(hip.lib().codae_reload_env())
    yield set_env
    for k in names:
        monkeypatch.delenv(k, raising=False)
    hip.check(hip.lib().codae_reload_env())


def f64(t):
    return t.detach().double().cpu().numpy()


# second row tile of 8 rows + second column tile of 8 columns; one 8 x 8 tile; 3 x 3 tiles with 8-row / 8-column last ones
SHAPES = [(264, 200, 64), (8, 8, 64), (520, 392, 128)]


@pytest.mark.parametrize("tile", ["x", "m"])
@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("y_f32", [0, 1], ids=["bf16out", "f32out"])
def test_linear_bf16_exact_integers_with_a_bias_that_differs_per_column(hip, env, tile, M, N, K, with_bias, relu, y_f32):
    """Small-integer operands: every product and partial sum is exact, so the result is the float64 product (rounded once to
    bf16 for a bf16 output) bit for bit.  bias[j] = j % 7 - 3 tells a column from its neighbours and a column tile from the
    next one; without a bias the epilogue must add nothing, whatever LDS holds."""
    env(CODAE_GEMM_TILE=tile)
    g = torch.Generator(device="cpu").manual_seed(M + 2 * N + 3 * K)
    x = torch.randint(-3, 4, (M, K), generator=g).float()
    W = torch.randint(-3, 4, (N, K), generator=g).float()
    b = (torch.arange(N) % 7 - 3).float()
    xb, Wb, bd = x.to(DEV).bfloat16(), W.to(DEV).bfloat16(), b.to(DEV)
    y = torch.full((M, N), float("nan"), device=DEV, dtype=torch.float32 if y_f32 else torch.bfloat16)
    hip.check(hip.lib().codae_linear_bf16(hip.ptr(xb), hip.ptr(Wb), hip.ptr(bd) if with_bias else None, hip.ptr(y), y_f32, M, N, K, relu,
                                          hip.current_stream()))
    torch.cuda.synchronize()
    ref = f64(x) @ f64(W).T + (f64(b) if with_bias else 0.0)
    if relu:
        ref = np.maximum(ref, 0)
    if not y_f32:
        ref = f64(torch.from_numpy(ref).bfloat16())
    assert np.array_equal(f64(y.float()), ref)


# io 216 = 192 + 24 columns (bit rows of 27 bytes, the second column tile's bits end 3 bytes in), 264 = 256 + 8 rows; io 192, 520 rows
STEP_SHAPES = [(3, 72, 264), (3, 64, 520)]
PIPE = dict(CODAE_GEMM_TILE="x", CODAE_NO_CHAIN="1")


def _problem(S, E, B):
    from oracle import dae_oracle as O
    io = S * E
    rng = np.random.default_rng(B + E)
    N = B + 64
    data = rng.random((N, io), dtype=np.float32)
    sched = O.layer_schedule(io, io, 3, 2, False, "embedding")
    params = O.init_params(sched, rng)
    bm, _, _ = O.corrupter_tables([{"size": E, "position": s * E} for s in range(S)], 1)
    mtu = rng.integers(0, S, (N, 1)).astype(np.int32)
    idx = torch.tensor(rng.permutation(N)[:B], dtype=torch.int32, device=DEV)
    return dict(B=B, data=data, sched=sched, params=params, bm=bm, mtu=mtu, idx=idx)


def _trainer(p, clip=1.0):
    from codae.train import HipEmbeddingTrainer
    tr = HipEmbeddingTrainer(p["sched"], torch.tensor(p["data"]), torch.tensor(p["bm"]).to(torch.uint8), torch.tensor(p["mtu"]), 1e-3, 1e-4,
                             clip, max_batch=p["B"], precision="bf16", device=DEV)
    tr.load_params(p["params"])
    return tr


def _two_steps(p):
    tr = _trainer(p)
    for _ in range(2):
        tr.train_batch(p["idx"], run=0)
    eng = tr.engine
    torch.cuda.synchronize()
    return eng.dacts.clone(), eng.grads.clone(), eng.params.clone(), eng.read_scalars()


@pytest.fixture(scope="module")
def pipe_two_steps(hip):
    """two fused steps on the pipelined 256 x 192 tile with the 1-bit masks on, per shape: computed once, compared against by
    the tests below and never modified"""
    import os
    out = {}
    saved = {k: os.environ.get(k) for k in PIPE}
    os.environ.update(PIPE)
    try:
        hip.check(hip.lib().codae_reload_env())
        for S, E, B in STEP_SHAPES:
            out[(S, E, B)] = _two_steps(_problem(S, E, B))
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        hip.check(hip.lib().codae_reload_env())
    return out


def _assert_same(a, b):
    (da, ga, pa, sa), (db, gb, pb, sb) = a, b
    assert float(ga.abs().max()) > 0
    assert torch.equal(da, db), "activation gradients"
    assert torch.equal(ga.view(torch.int32), gb.view(torch.int32)), "gradients"
    assert torch.equal(pa.view(torch.int32), pb.view(torch.int32)), "parameters"
    assert sa == sb, (sa, sb)


@pytest.mark.parametrize("S,E,B", STEP_SHAPES)
def test_parked_relu_bits_give_the_bits_of_the_activation_mask(env, pipe_two_steps, S, E, B):
    """the data gradient masks from the bit tile parked in LDS; CODAE_NO_RELU_BITS=1 masks from the saved activation"""
    env(CODAE_NO_RELU_BITS="1", **PIPE)
    _assert_same(pipe_two_steps[(S, E, B)], _two_steps(_problem(S, E, B)))


@pytest.mark.parametrize("S,E,B", STEP_SHAPES)
def test_next_weights_touch_changes_no_bit(env, pipe_two_steps, S, E, B):
    env(CODAE_NO_PREFETCH="1", **PIPE)
    _assert_same(pipe_two_steps[(S, E, B)], _two_steps(_problem(S, E, B)))


@pytest.mark.parametrize("S,E,B", STEP_SHAPES)
def test_pipelined_tile_gives_the_bits_of_the_one_barrier_kernel(env, S, E, B):
    """One step on the 256 x 192 pipelined tile against the 128 x 128 one-barrier kernel, which takes its bias and masks by plain
    loads: per-layer weight gradients on both sides, the same K split.  Every kernel accumulates a tile's k range in the same
    order: activations, activation gradients and weight gradients bit for bit; bias gradients differ by how many rows a
    partial sum spans."""
    p = _problem(S, E, B)
    outs = []
    for tile in ("x", "s"):
        env(CODAE_GEMM_TILE=tile, CODAE_NO_CHAIN="1", CODAE_WGRAD_SPLITK="1", CODAE_NO_DEFER_WGRAD="1", CODAE_NO_RELU_BITS="1")
        tr = _trainer(p, clip=100.0)
        tr.train_batch(p["idx"], run=0)
        eng = tr.engine
        torch.cuda.synchronize()
        nw = eng.b_off[0]
        outs.append((eng.acts.clone(), eng.dacts.clone(), eng.grads[:nw].clone(), eng.grads[nw:].clone()))
    (aa, da, ga, ba), (ab, db, gb, bb) = outs
    assert float(ga.abs().max()) > 0 and float(ba.abs().max()) > 0
    assert torch.equal(aa, ab), "saved activations"
    assert torch.equal(da, db), "activation gradients"
    assert torch.equal(ga.view(torch.int32), gb.view(torch.int32)), "weight gradients"
    assert float((ba - bb).abs().max()) <= 1e-5 * float(bb.abs().max())


def test_thirty_repeats_of_forward_and_backward_give_one_result(env):
    """Race screen for the parked bias / bit regions: forward with the fused loss, then the whole backward, 30 times on one batch
    at 3 x 72, 264 rows.  Loss, metric sums, the activation-gradient workspace and the bias partial sums: one set of bits."""
    env(**PIPE)
    S, E, B = 3, 72, 264
    p = _problem(S, E, B)
    tr = _trainer(p)
    eng = tr.engine
    batch = tr._batch(p["idx"], 0)
    hyper = eng.hyper(1e-3, 1e-4, 1.0, global_rows=B)
    seen = set()
    for _ in range(30):
        eng.zero_metric_sums()
        eng.bias_parts.zero_()
        eng.step_forward_loss(batch, hyper)
        eng.step_backward(B, 0, eng.L)
        torch.cuda.synchronize()
        sq, sqp, _, loss = eng.read_scalars()
        seen.add((sq, sqp, loss, eng.dacts.cpu().numpy().tobytes(), eng.bias_parts.cpu().numpy().tobytes()))
    assert len(seen) == 1, len(seen)
