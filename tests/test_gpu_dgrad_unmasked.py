"""The data gradient with no ReLU mask at all - the layer behind the code layer - runs an instantiation of its own of the pipelined
256 x 192 kernel (EPI 5, gemm_bf16_pipe.hip): one kind of write-out, nothing parked in LDS but the bias slice.  Its result is
pinned to the 128 x 128 one-barrier kernel's, bit for bit, at a shape with ragged edges both ways - 2500 rows = nine row tiles and
196 rows, 3064 columns = fifteen column tiles and 184 columns - and a contraction of one and of three K-tiles, under both store
policies.  Operands are small integers, so every sum is exact whatever its order: the column sums (the previous layer's bias
gradient) agree bit for bit as well, and both agree with float64.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
M, N = 2500, 3064


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


@pytest.fixture(scope="module")
def operands():
    """per contraction length: dy [M][K], W [K][N] (small integers), the float64 product rounded once to bf16 and its column sums -
    computed once, never modified"""
    out = {}
    for K in (64, 192):
        g = torch.Generator(device="cpu").manual_seed(K)
        dy = torch.randint(-3, 4, (M, K), generator=g).float()
        W = torch.randint(-3, 4, (K, N), generator=g).float()
        ref = (dy.double() @ W.double()).bfloat16()               # |sum| <= 192 * 9: exact in fp32, rounded once
        out[K] = dict(dy=dy.to(DEV).bfloat16(), W=W.to(DEV).bfloat16(), dx=ref.view(torch.int16).numpy(),
                      db=ref.double().sum(0).numpy())             # integers below 2^24 in magnitude: exact in fp32 in any order
    return out


def _dgrad(hip, op, K):
    """codae_dgrad_bf16 with relu_src NULL: dx [M][N] = dy [M][K] . W [K][N], db = column sums of the stored dx"""
    dx = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    db = torch.full((N,), float("nan"), dtype=torch.float32, device=DEV)
    ws = torch.zeros(((M + 127) // 128) * N, dtype=torch.float32, device=DEV)
    hip.check(hip.lib().codae_dgrad_bf16(hip.ptr(op["dy"]), hip.ptr(op["W"]), None, hip.ptr(dx), hip.ptr(db), hip.ptr(ws), M, K, N,
                                         hip.current_stream()))
    torch.cuda.synchronize()
    return dx.view(torch.int16).cpu().numpy(), db.double().cpu().numpy()


@pytest.mark.parametrize("policy", ["plain", "wt"])
@pytest.mark.parametrize("K", [64, 192])
def test_unmasked_data_gradient_gives_the_bits_of_the_one_barrier_kernel(hip, env, operands, K, policy):
    op = operands[K]
    env(CODAE_GEMM_TILE="s", CODAE_STORE_POLICY=None)
    dx_s, db_s = _dgrad(hip, op, K)
    env(CODAE_GEMM_TILE="x", CODAE_STORE_POLICY=policy)
    dx_x, db_x = _dgrad(hip, op, K)
    assert np.array_equal(dx_x, dx_s), np.argwhere(dx_x != dx_s)[:4]
    assert np.array_equal(db_x, db_s)
    assert np.array_equal(dx_x, op["dx"]) and np.array_equal(db_x, op["db"])
    assert np.abs(op["db"]).max() > 0


def test_the_plan_still_reports_the_data_gradient_epilogue(hip, env):
    """the instantiation is the launcher's choice: gemm_bf16_plan keeps saying epilogue 2 for this launch, on the pipelined tile"""
    import ctypes as C
    GEMM_PLAN_FIELDS = 15                                        # CODAE_GEMM_PLAN_FIELDS (include/codae_hip.h)
    env(CODAE_GEMM_TILE="x")
    # a_mode, b_mode, c_f32, M, N, K, split_k, act, fused loss, backward epilogue, coscheduled, store_policy, ldc
    desc = (C.c_int32 * 13)(0, 1, 0, M, N, 192, 1, 0, 0, 1, 0, -1, N)
    out = (C.c_int32 * GEMM_PLAN_FIELDS)()
    hip.check(hip.lib().codae_debug_gemm_bf16_plan(desc, out, GEMM_PLAN_FIELDS))
    family, bm, bn, _, _, epi = list(out)[:6]
    assert (family, bm, bn, epi) == (1, 256, 192, 2)


STEP = dict(CODAE_GEMM_TILE="x", CODAE_NO_CHAIN="1")


def _two_steps(S, E, B):
    """two fused steps of a stack with a code layer (no ReLU behind it: its data gradient is the unmasked one)"""
    from codae.train import HipEmbeddingTrainer
    from oracle import dae_oracle as O
    io = S * E
    rng = np.random.default_rng(B + E)
    n = B + 64
    sched = O.layer_schedule(io, io, 3, 2, False, "embedding")
    assert [r for _, _, r in sched].count(False) == 2            # the code layer and the output layer
    bm, _, _ = O.corrupter_tables([{"size": E, "position": s * E} for s in range(S)], 1)
    tr = HipEmbeddingTrainer(sched, torch.tensor(rng.random((n, io), dtype=np.float32)), torch.tensor(bm).to(torch.uint8),
                             torch.tensor(rng.integers(0, S, (n, 1)).astype(np.int32)), 1e-3, 1e-4, 1.0, max_batch=B, precision="bf16", device=DEV)
    tr.load_params(O.init_params(sched, rng))
    idx = torch.tensor(rng.permutation(n)[:B], dtype=torch.int32, device=DEV)
    for _ in range(2):
        tr.train_batch(idx, run=0)
    eng = tr.engine
    torch.cuda.synchronize()
    return eng.dacts.clone(), eng.grads.clone(), eng.params.clone(), eng.read_scalars()


def test_next_weights_touch_changes_no_bit_of_a_step_with_an_unmasked_data_gradient(hip, env):
    """in the step the unmasked launch also touches the next launch's weights under its epilogue (GemmBf16::prefetch): two steps at
    3 x 72 wide, 264 rows (a second row tile of 8 rows, a second column tile of 24 columns) with and without the touch"""
    env(**STEP)
    a = _two_steps(3, 72, 264)
    env(CODAE_NO_PREFETCH="1", **STEP)
    b = _two_steps(3, 72, 264)
    (da, ga, pa, sa), (db, gb, pb, sb) = a, b
    assert float(ga.abs().max()) > 0
    assert torch.equal(da, db), "activation gradients"
    assert torch.equal(ga.view(torch.int32), gb.view(torch.int32)), "gradients"
    assert torch.equal(pa.view(torch.int32), pb.view(torch.int32)), "parameters"
    assert sa == sb, (sa, sb)
