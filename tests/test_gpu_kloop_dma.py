"""LDS-DMA addressing of the pipelined bf16 GEMM's K loop: {wave-uniform scalar base, loop-invariant 32-bit lane offset}
(gemm_bf16_halftile.h: half_src, glds16).  What can go wrong is an address: a row or column clamp, the K advance in
the scalar base, the dummy loads past the last K-tile, a lane offset whose bit 31 is set (it must be ZERO-extended), a leading
dimension that is not the extent.  A wrong address shows as a wrong product, so every check is the float64 product of the same
small-integer operands (every partial sum is exact in fp32), compared bit for bit.

Shapes are the smallest that reach each case on the forced 256 x 192 / 128 x 192 tiles: M = 8 (every row but the first eight
clamped) and 264 (a full row tile + 8 rows); N = 8 (the column clamp at N - 8) and 200 (192 + 8); K = 64 (one K-tile: every later
load is a dummy), 128, 192 (the odd-count tail of the two-tile loop).  Launches go through codae_debug_gemm_bf16, which spells out
operand modes and leading dimensions, on both loader layouts (CODAE_GEMM_TILE x: one loader wave per SIMD, q: every wave loads) and,
for the forward form, the 128 x 192 tile (m).  The forms that exist only inside an engine step - the fused loss (EPI 3), the 1-bit
mask and unmasked data gradients on the forward-form kernel (EPI 4, 5) and the grouped weight-gradient launch with its bias fold -
run one step of a five-layer stack with three different layer shapes against the same step on the one-barrier 128 x 128 kernels with
the stand-alone loss kernel.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
KC, KS = 0, 1
MS, NS, KSIZES = [8, 264], [8, 200], [64, 128, 192]
TILES = {"x": (256, 192), "q": (256, 192), "m": (128, 192)}


@pytest.fixture(scope="module")
def hip():
    from codae import hip as H
    H.lib()
    return H


@pytest.fixture
def env(monkeypatch, hip):
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


def ints(shape, seed, lo=-3, hi=4):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(lo, hi, shape, generator=g).float()


def strided(t, ld, lead=0):
    """t [r][c] placed in a fresh bf16 allocation with rows ld elements apart, `lead` elements in; the gaps hold 7 (a value a
    wrong address would bring into the product).  -> (allocation, view of the operand)"""
    r, c = t.shape
    buf = torch.full((lead + r * ld,), 7.0, device=DEV, dtype=torch.bfloat16)
    view = buf[lead:].view(r, ld)[:, :c]
    view.copy_(t.to(DEV).bfloat16())
    return buf, view


def assert_pipelined(hip, tile, a_mode, b_mode, c_f32, M, N, K, split, ldc):
    desc = (C.c_int32 * 13)(a_mode, b_mode, c_f32, M, N, K, split, 0, 0, 0, 0, -1, ldc)
    out = (C.c_int32 * 15)()
    hip.check(hip.lib().codae_debug_gemm_bf16_plan(desc, out, 15))
    assert out[0] == 1 and (out[1], out[2]) == TILES[tile], ("not the pipelined tile", list(out))


def gemm(hip, tile, A, lda, a_mode, B, ldb, b_mode, c_f32, M, N, K, split=1, bias=None, relu=0, ldc=None):
    """C [split][M][ldc], NaN where nothing was written"""
    ldc = N if ldc is None else ldc
    assert_pipelined(hip, tile, a_mode, b_mode, c_f32, M, N, K, split, ldc)
    out = torch.full((split, M, ldc), float("nan"), device=DEV, dtype=torch.float32 if c_f32 else torch.bfloat16)
    hip.check(hip.lib().codae_debug_gemm_bf16(hip.ptr(A), lda, a_mode, hip.ptr(B), ldb, b_mode, hip.ptr(out), ldc, c_f32, M, N, K, split,
                                              hip.ptr(bias), relu, hip.current_stream()))
    torch.cuda.synchronize()
    return out


def as_bf16(ref):
    return f64(torch.from_numpy(ref).bfloat16())


@pytest.mark.parametrize("K", KSIZES)
@pytest.mark.parametrize("M,N", [(m, n) for m in MS for n in NS])
@pytest.mark.parametrize("tile", ["x", "q", "m"])
def test_forward_form_with_bias_and_relu(hip, env, tile, M, N, K):
    """k-contiguous x k-contiguous, bf16 out (EPI 1); both operands in rows longer than K, so a K advance that followed the leading
    dimension or a row that followed K would read the 7s between the rows"""
    env(CODAE_GEMM_TILE=tile)
    x, W = ints((M, K), 1000 * M + N + K), ints((N, K), 2000 * M + N + K)
    b = (torch.arange(N) % 7 - 3).float().to(DEV)
    (xa, xv), (wa, wv) = strided(x, K + 72), strided(W, K + 8)
    y = gemm(hip, tile, xv, K + 72, KC, wv, K + 8, KC, 0, M, N, K, bias=b, relu=1)[0]
    ref = as_bf16(np.maximum(f64(x) @ f64(W).T + f64(b), 0))
    assert np.array_equal(f64(y.float()), ref)


@pytest.mark.parametrize("K", KSIZES)
@pytest.mark.parametrize("M,N", [(m, n) for m in MS for n in NS])
@pytest.mark.parametrize("tile", ["x", "q"])
def test_k_strided_b_operand_bf16_out(hip, env, tile, M, N, K):
    """k-contiguous x k-strided (the data gradient through W itself): B [K][ldb] with ldb = N + 16"""
    env(CODAE_GEMM_TILE=tile)
    a, Bm = ints((M, K), 3000 * M + N + K), ints((K, N), 4000 * M + N + K)
    (aa, av), (ba, bv) = strided(a, K), strided(Bm, N + 16)
    y = gemm(hip, tile, av, K, KC, bv, N + 16, KS, 0, M, N, K)[0]
    assert np.array_equal(f64(y.float()), as_bf16(f64(a) @ f64(Bm)))


@pytest.mark.parametrize("K,split", [(64, 1), (128, 1), (192, 1), (128, 2), (192, 2)])
@pytest.mark.parametrize("M,N", [(m, n) for m in MS for n in NS])
@pytest.mark.parametrize("tile", ["x", "q"])
def test_both_operands_k_strided_fp32_out_plain_and_split_k(hip, env, tile, M, N, K, split):
    """the weight-gradient form: A [K][lda], B [K][ldb], fp32 C; split-K 2 writes two partial products (192 rows: K-tiles 1 + 2)"""
    env(CODAE_GEMM_TILE=tile)
    At, Bm = ints((K, M), 5000 * M + N + K), ints((K, N), 6000 * M + N + K)
    (aa, av), (ba, bv) = strided(At, M + 24), strided(Bm, N + 8)
    y = gemm(hip, tile, av, M + 24, KS, bv, N + 8, KS, 1, M, N, K, split=split, ldc=N + 4)
    assert np.array_equal(f64(y[:, :, :N]).sum(axis=0), f64(At).T @ f64(Bm))
    assert bool(torch.isnan(y[:, :, N:]).all()), "columns past N were written"


@pytest.mark.parametrize("tile", ["x", "q"])
def test_unmasked_data_gradient_with_column_sums(hip, env, tile):
    """EPI 5 on the k-strided B form (codae_dgrad_bf16 without a saved activation): dx and its column sums"""
    env(CODAE_GEMM_TILE=tile)
    M, N, K = 264, 128, 200                          # dy [M][N] . W [N][K] -> dx [M][K]
    dy, W = ints((M, N), 71, -2, 3), ints((N, K), 72, -2, 3)
    dyd, Wd = dy.to(DEV).bfloat16(), W.to(DEV).bfloat16()
    dx = torch.full((M, K), float("nan"), device=DEV, dtype=torch.bfloat16)
    db = torch.full((K,), float("nan"), device=DEV)
    ws = torch.zeros(((M + 63) // 64 * K,), device=DEV)
    hip.check(hip.lib().codae_dgrad_bf16(hip.ptr(dyd), hip.ptr(Wd), None, hip.ptr(dx), hip.ptr(db), hip.ptr(ws), M, N, K, hip.current_stream()))
    torch.cuda.synchronize()
    ref = as_bf16(f64(dy) @ f64(W))
    assert np.array_equal(f64(dx.float()), ref)
    assert np.array_equal(f64(db), ref.sum(axis=0))              # (sums of the STORED bf16 values: integers below 2^24, exact)


def need_free(nbytes):
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes + (1 << 30):
        pytest.skip("needs %.1f GiB of free device memory for an operand that spans more than 2 GiB; %.1f free" % (nbytes / 2**30, free / 2**30))


@pytest.mark.parametrize("tile", ["x", "q"])
def test_lane_offsets_with_bit_31_set_k_contiguous(hip, env, tile):
    """A [264][lda] with rows 8 MiB + 128 B apart: rows 256 .. 263 (the second row tile) lie more than 2 GiB behind the base the
    instruction takes, so their 32-bit lane offsets have bit 31 set; the operand starts at offset 0 of its allocation"""
    env(CODAE_GEMM_TILE=tile)
    M, N, K, lda = 264, 200, 192, (1 << 22) + 64
    assert (M - 1) * lda * 2 >= 1 << 31 and M * lda * 2 < 1 << 32
    need_free(M * lda * 2)
    x, W = ints((M, K), 81), ints((N, K), 82)
    buf = torch.zeros((M * lda,), device=DEV, dtype=torch.bfloat16)
    xv = buf.view(M, lda)[:, :K]
    xv.copy_(x.to(DEV).bfloat16())
    assert xv.data_ptr() == buf.data_ptr()
    Wd = W.to(DEV).bfloat16()
    y = gemm(hip, tile, xv, lda, KC, Wd, K, KC, 1, M, N, K)[0]
    assert np.array_equal(f64(y), f64(x) @ f64(W).T)


@pytest.mark.parametrize("tile", ["x", "q"])
def test_lane_offsets_with_bit_31_set_k_strided(hip, env, tile):
    """B [64][ldb] with k-rows 34 MiB apart, 4 KiB into its allocation: the last k-rows of the one K-tile lie more than 2 GiB in"""
    env(CODAE_GEMM_TILE=tile)
    M, N, K, ldb, lead = 264, 200, 64, (1 << 24) + (1 << 20) + 8, 2048
    assert (K - 1) * ldb * 2 >= 1 << 31 and K * ldb * 2 < 1 << 32
    need_free(K * ldb * 2)
    At, Bm = ints((K, M), 91), ints((K, N), 92)
    buf = torch.zeros((lead + K * ldb,), device=DEV, dtype=torch.bfloat16)
    bv = buf[lead:].view(K, ldb)[:, :N]
    bv.copy_(Bm.to(DEV).bfloat16())
    Ad = At.to(DEV).bfloat16()
    y = gemm(hip, tile, Ad, M, KS, bv, ldb, KS, 1, M, N, K)[0]
    assert np.array_equal(f64(y), f64(At).T @ f64(Bm))


# ---- forms that exist only inside a step ------------------------------------------------------
# 1536 -> 1536 -> 1032 -> 1536 -> 1536 -> 1536: weight gradients of three shapes (1536 x 1536, 1032 x 1536, 1536 x 1032), 220 tiles of
# 256 x 192 in all - enough for the engine to take the grouped launch (200) - and 1032 = 5 x 192 + 72 = 4 x 256 + 8
WIDTHS = [1536, 1536, 1032, 1536, 1536, 1536]
B_STEP = 192                                         # three K-tiles for the weight gradients: the loop and its odd tail


def _problem():
    from oracle import dae_oracle as O
    S, E = 3, 512
    io = S * E
    rng = np.random.default_rng(5)
    n = B_STEP + 64
    data = rng.random((n, io), dtype=np.float32)
    sched = [(WIDTHS[l], WIDTHS[l + 1], l + 2 < len(WIDTHS)) for l in range(len(WIDTHS) - 1)]
    params = O.init_params(sched, rng)
    bm, _, _ = O.corrupter_tables([{"size": E, "position": s * E} for s in range(S)], 1)
    mtu = rng.integers(0, S, (n, 1)).astype(np.int32)
    idx = torch.tensor(rng.permutation(n)[:B_STEP], dtype=torch.int32, device=DEV)
    return sched, params, torch.tensor(data), torch.tensor(bm).to(torch.uint8), torch.tensor(mtu), idx


def _one_step(problem):
    from codae.train import HipEmbeddingTrainer
    sched, params, data, bm, mtu, idx = problem
    tr = HipEmbeddingTrainer(sched, data, bm, mtu, 1e-3, 1e-4, 100.0, max_batch=B_STEP, precision="bf16", device=DEV)
    tr.load_params(params)
    tr.train_batch(idx, run=0)
    eng = tr.engine
    torch.cuda.synchronize()
    nw = eng.b_off[0]
    sq, sqp, gsq, loss = eng.read_scalars()
    return eng.grads[:nw].clone(), eng.grads[nw:].clone(), (sq, sqp, loss)


@pytest.fixture(scope="module")
def step_problem():
    return _problem()


@pytest.fixture(scope="module")
def one_barrier_step(hip, step_problem):
    """the step on the 128 x 128 one-barrier kernels, per-layer unsplit weight gradients, saved-activation masks and the
    stand-alone loss kernel (mse_loss_kernel): computed once, never modified"""
    import os
    forced = dict(CODAE_GEMM_TILE="s", CODAE_NO_CHAIN="1", CODAE_NO_DEFER_WGRAD="1", CODAE_WGRAD_SPLITK="1", CODAE_NO_RELU_BITS="1",
                  CODAE_NO_FUSED_LOSS="1")
    saved = {k: os.environ.get(k) for k in forced}
    os.environ.update(forced)
    try:
        hip.check(hip.lib().codae_reload_env())
        return _one_step(step_problem)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        hip.check(hip.lib().codae_reload_env())


@pytest.mark.parametrize("tile", ["x", "q"])
def test_step_with_fused_loss_bit_masks_and_grouped_weight_gradients(hip, env, step_problem, one_barrier_step, tile):
    """Forward (EPI 1), fused loss (EPI 3), 1-bit-mask and unmasked data gradients on the forward-form kernel (EPI 4, 5) and all five
    weight gradients in the grouped launch with the bias finish folded in, on the forced pipelined tile.  Every kernel accumulates a
    tile's k range in the same order, so the weight gradients - which take in every activation and every activation gradient, the
    fused loss's dy among them - equal the one-barrier step's bit for bit.  Bias gradients and the loss are sums of the same terms
    in another grouping: fp32 partial sums of at most 264 terms on either side, so 1e-5 relative to the largest."""
    env(CODAE_GEMM_TILE=tile, CODAE_NO_CHAIN="1")
    gw, gb, (sq, sqp, loss) = _one_step(step_problem)
    rw, rb, (rsq, rsqp, rloss) = one_barrier_step
    assert float(rw.abs().max()) > 0 and float(rb.abs().max()) > 0
    assert torch.equal(gw.view(torch.int32), rw.view(torch.int32)), "weight gradients"
    assert float((gb - rb).abs().max()) <= 1e-5 * float(rb.abs().max())
    assert abs(loss - rloss) <= 1e-5 * abs(rloss) and abs(sq - rsq) <= 1e-5 * abs(rsq) and abs(sqp - rsqp) <= 1e-5 * abs(rsqp)
