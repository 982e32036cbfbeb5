"""NaN / Inf through the kernels and the fused step on a real MI355X, pinned to torch (include/codae_hip.h, "Non-finite
values").

Kernel cases (A, B) run twice, on clean operands and on operands with a few planted non-finite values (nonfinite_ref.py), and
check (1) the planted launch against float64 class by class - NaN, +Inf, -Inf exactly where the reference has them, finite
values at the tolerances the finite-data tests of the same entry use - and (2) that every output that does not depend on a
planted value is BIT-IDENTICAL to the clean launch: rows and columns of a GEMM are independent, ragged tiles, clamped
loads, column-sum partials and split-K slabs included.  Outputs are pre-filled with a finite sentinel, so an element the
kernel never wrote cannot pass for a propagated NaN.

The one exception (contract point 5): the bf16-plane fp32 GEMM (gemm_f32x3.hip) cuts an operand into three bf16 planes, and
the residual planes of an Inf are Inf - Inf.  Where a case may run on that kernel it allows NaN, and only NaN, at outputs
whose float64 reference depends on an Inf ELEMENT of x, W or dy (row 0 of the planting designs).  An Inf bias is added in
fp32 and gets no allowance."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
nn = torch.nn

import nonfinite_ref as R  # noqa: E402
from test_gpu_activation import KIND_IDS, KINDS, cpu_copy  # noqa: E402

DEV = "cuda:0"
SENTINEL = 12345.0
nan, inf = float("nan"), float("inf")


@pytest.fixture(scope="module")
def hip():
    from codae import hip as H
    H.lib()
    return H


@pytest.fixture
def env(hip, monkeypatch):
    """set CODAE_* variables for one test (the library reads them at codae_reload_env / codae_create), restored afterwards"""
    names = []

    def set_(name, value):
        names.append(name)
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
        hip.check(hip.lib().codae_reload_env())
    yield set_
    for n in names:
        monkeypatch.delenv(n, raising=False)
    hip.check(hip.lib().codae_reload_env())


@pytest.fixture(params=["chain", "layers"])
def step_path(request, monkeypatch):
    """Narrow bf16 stacks have two implementations of codae_train_step: the persistent fused chain and the per-layer GEMM
    launches (CODAE_NO_CHAIN=1, read at codae_create).  As in test_gpu_parity.py."""
    if request.param == "layers":
        monkeypatch.setenv("CODAE_NO_CHAIN", "1")
    else:
        monkeypatch.delenv("CODAE_NO_CHAIN", raising=False)
    return request.param


def sync():
    torch.cuda.synchronize()


def rbf(a):
    """float32 array rounded to bf16 values"""
    return torch.tensor(np.asarray(a, dtype=np.float32)).bfloat16().float().numpy()


def up(a, bf16=False):
    t = torch.tensor(np.asarray(a, dtype=np.float32))
    return (t.bfloat16() if bf16 else t).to(DEV)


def out(shape, dtype=torch.float32):
    return torch.full(shape, SENTINEL, dtype=dtype, device=DEV)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy()


def same_bits_outside(clean, planted, touched):
    a, b = bits(clean), bits(planted)
    assert np.array_equal(a[~touched], b[~touched]), "%d untouched outputs changed" % int((a[~touched] != b[~touched]).sum())


def row0(shape):
    m = np.zeros(shape, dtype=bool)
    m[0] = True
    return m


# ---------------------------------------------------------------------------------------------------------------------
# A. forward entries
# ---------------------------------------------------------------------------------------------------------------------
def forward_case(launch, M, N, K, module, rtol, atol, bf16_ops=False, out_dtypes=(torch.float32,), x3=False, bias_cols=False,
                 wscale=1.0):
    """launch(x, W, b, y): one forward entry.  Clean and planted run, the two checks of the module docstring."""
    rng = np.random.default_rng(M * 7 + N * 3 + K)
    x = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((N, K)) * wscale).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    if bf16_ops:
        x, W = rbf(x), rbf(W)
    xp, Wp, bp = x.copy(), W.copy(), b.copy()
    touched = R.plant_forward(xp, Wp, bp)
    if bias_cols:                                  # three ordinary columns: the activation sees +Inf, -Inf and NaN
        bp[1], bp[2], bp[3] = inf, -inf, nan
        touched[:, 1:4] = True
    ref_clean, ref = R.forward_ref(x, W, b, module), R.forward_ref(xp, Wp, bp, module)
    for dt in out_dtypes:
        ys = []
        for xa, Wa, ba in ((x, W, b), (xp, Wp, bp)):
            y = out((M, N), dt)
            launch(up(xa, bf16_ops), up(Wa, bf16_ops), up(ba), y)
            sync()
            ys.append(y)
        R.assert_same(ys[0].double(), ref_clean, rtol, atol)
        R.assert_same(ys[1].double(), ref, rtol, atol, allow_nan_at=row0((M, N)) if x3 else None)
        same_bits_outside(ys[0], ys[1], touched)


@pytest.mark.parametrize("mode,M,N,K", [("native", 37, 11, 11), ("native", 130, 200, 77), ("native", 256, 256, 256),
                                        ("x3", 128, 128, 32), ("x3", 200, 132, 64)])
@pytest.mark.parametrize("relu", [0, 1])
def test_linear_f32(hip, env, mode, M, N, K, relu):
    """codae_linear_f32 on the fp32-MFMA kernel (strict) and on the bf16-plane kernel, where NaN - and only NaN - is allowed
    in row 0, whose reference depends on the Inf element x[0, 0] (contract point 5; the -Inf bias gets no allowance)."""
    env("CODAE_F32_GEMM", mode)
    L, s = hip.lib(), hip.current_stream()
    forward_case(lambda x, W, b, y: hip.check(L.codae_linear_f32(hip.ptr(x), hip.ptr(W), hip.ptr(b), hip.ptr(y), M, N, K, relu, s)),
                 M, N, K, nn.ReLU() if relu else None, 1e-3, 1e-4 * math.sqrt(K), x3=mode == "x3")


BF16_SHAPES = [(200, 192, 128), (8, 64, 64), (520, 448, 192)]
# rtol of a bf16 output: one rounding to 8 significant bits (2^-9) on top of fp32 accumulation; the finite-data tests use 1e-2
BF16_RTOL, BF16_ATOL = 1e-2, 1e-2


@pytest.mark.parametrize("tile,y_f32", [(t, f) for t in "sqx" for f in (0, 1)] + [("m", 0)])
@pytest.mark.parametrize("M,N,K", BF16_SHAPES)
@pytest.mark.parametrize("relu", [0, 1])
def test_linear_bf16(hip, env, tile, y_f32, M, N, K, relu):
    """codae_linear_bf16 on every workgroup tile (s 128 x 128, q / x 256 x 192 pipelined, m 128 x 192 with a bf16 output)
    against the float64 product of the bf16-rounded operands."""
    env("CODAE_GEMM_TILE", tile)
    L, s = hip.lib(), hip.current_stream()
    forward_case(lambda x, W, b, y: hip.check(L.codae_linear_bf16(hip.ptr(x), hip.ptr(W), hip.ptr(b), hip.ptr(y), y_f32, M, N, K, relu, s)),
                 M, N, K, nn.ReLU() if relu else None, BF16_RTOL, BF16_ATOL, bf16_ops=True,
                 out_dtypes=(torch.float32 if y_f32 else torch.bfloat16,), wscale=2 / math.sqrt(K))


def engine_act(kind):
    from codae.model.activation import as_engine_act
    module = KINDS[kind](True)                     # (the reference's call: activation(True))
    if hasattr(module, "inplace"):
        module.inplace = False                     # the float64 reference differentiates it from its input
    return module, as_engine_act(module)


@pytest.mark.parametrize("kind", range(len(KINDS)), ids=KIND_IDS)
@pytest.mark.parametrize("f32_gemm", [None, "native"], ids=["default", "native"])
def test_linear_act_f32(hip, env, kind, f32_gemm):
    """every activation kind sees NaN, +Inf and -Inf pre-activations and maps them as its torch.nn module does.  Default
    dispatch may take the bf16-plane kernel: NaN allowed in row 0 (contract point 5), nowhere else."""
    env("CODAE_F32_GEMM", f32_gemm)
    M, N, K = 200, 136, 128
    module, (k, p0, p1, p2) = engine_act(kind)
    L, s = hip.lib(), hip.current_stream()
    forward_case(lambda x, W, b, y: hip.check(L.codae_linear_act_f32(hip.ptr(x), hip.ptr(W), hip.ptr(b), hip.ptr(y), M, N, K, k, p0, p1, p2, s)),
                 M, N, K, module, 1e-3, 1e-5, x3=f32_gemm is None, bias_cols=True, wscale=2 / math.sqrt(K))


@pytest.mark.parametrize("kind", range(len(KINDS)), ids=KIND_IDS)
def test_linear_act_bf16(hip, kind):
    M, N, K = 200, 128, 192
    module, (k, p0, p1, p2) = engine_act(kind)
    L, s = hip.lib(), hip.current_stream()
    for y_f32 in (0, 1):
        forward_case(lambda x, W, b, y: hip.check(L.codae_linear_act_bf16(hip.ptr(x), hip.ptr(W), hip.ptr(b), hip.ptr(y), y_f32, M, N, K,
                                                                          k, p0, p1, p2, s)),
                     M, N, K, module, BF16_RTOL, BF16_ATOL, bf16_ops=True, out_dtypes=(torch.float32 if y_f32 else torch.bfloat16,),
                     bias_cols=True, wscale=2 / math.sqrt(K))


@pytest.mark.parametrize("kind", [None, nn.ELU], ids=["relu", "elu"])
def test_split_k_forward_epilogue(kind):
    """fp32 engine at io 384, batch 128 (as test_split_k_slab_reduce_epilogue): the forward GEMMs are split over K into slabs
    and finished by reduce_slabs_epi, whose epilogue applies bias and activation.  A NaN in the last batch row and a -Inf
    bias of a first-layer unit: the last row of the output is NaN, every other row is bit-identical to the run without the
    NaN and equal to the float64 CPU forward.  (No Inf element: no plane-kernel allowance is needed.)  Which
    kernel a shape is dispatched to is not visible through the ABI: like the test it follows, this relies on the dispatch
    rule for small batches."""
    from codae.model import EmbeddingDenoisingAutoencoder
    torch.manual_seed(4)
    kw = {} if kind is None else {"activation": kind}
    m = EmbeddingDenoisingAutoencoder(384, 384, 128, 2, 2, False, **kw).to(DEV)
    m.precision = "f32"
    with torch.no_grad():
        m.input_layer[0].bias[3] = -inf
    x = np.random.default_rng(9).random((128, 384)).astype(np.float32)
    xp = x.copy()
    xp[127, 200] = nan
    with torch.no_grad():
        y0 = m(torch.tensor(x, device=DEV)).clone()
        y1 = m(torch.tensor(xp, device=DEV)).clone()
        sync()
        ref = cpu_copy(m)(torch.tensor(xp, dtype=torch.float64)).numpy()
    assert np.isnan(ref[127]).all() and np.isfinite(ref[:127]).all()
    R.assert_same(y1.double(), ref, 1e-3, 1e-5)
    touched = np.zeros((128, 384), dtype=bool)
    touched[127] = True
    same_bits_outside(y0, y1, touched)


# ---------------------------------------------------------------------------------------------------------------------
# B. backward entries
# ---------------------------------------------------------------------------------------------------------------------
F32_BWD = [("native", 37, 11, 11), ("native", 130, 200, 77), ("x3", 200, 132, 64)]


@pytest.mark.parametrize("mode,M,N,K", F32_BWD)
@pytest.mark.parametrize("with_src", [True, False], ids=["relu_src", "null"])
def test_dgrad_f32(hip, env, mode, M, N, K, with_src):
    """dx = (dy W) selected by relu_src > 0.  x3: NaN allowed in row 0 (the Inf element dy[0, 0])."""
    env("CODAE_F32_GEMM", mode)
    rng = np.random.default_rng(M + N + K)
    dy, W, h = (rng.standard_normal(sh).astype(np.float32) for sh in ((M, N), (N, K), (M, K)))
    dyp, Wp = dy.copy(), W.copy()
    tdx, _ = R.plant_backward(dyp, Wp)
    hd = up(h) if with_src else None
    dxs = []
    for a, b in ((dy, W), (dyp, Wp)):
        dx, ad, bd = out((M, K)), up(a), up(b)        # (named: a temporary's memory would be reused before the launch runs)
        hip.check(hip.lib().codae_dgrad_f32(hip.ptr(ad), hip.ptr(bd), hip.ptr(hd), hip.ptr(dx), M, N, K, hip.current_stream()))
        sync()
        dxs.append(dx)
    src = h if with_src else None
    R.assert_same(dxs[0].double(), R.dgrad_relu_ref(dy, W, src), 0, 1e-4 * math.sqrt(N))
    R.assert_same(dxs[1].double(), R.dgrad_relu_ref(dyp, Wp, src), 0, 1e-4 * math.sqrt(N), allow_nan_at=row0((M, K)) if mode == "x3" else None)
    same_bits_outside(dxs[0], dxs[1], tdx)


def check_colsum(db_clean, db, ref_dx_stored):
    """db = column sums of the stored dx: a column that holds a NaN sums to NaN, one with an Inf (and no NaN) to that Inf;
    every finite column is bit-identical to the clean launch"""
    with np.errstate(all="ignore"):
        cref = R.classes(ref_dx_stored.sum(0))
    assert np.array_equal(R.classes(db), cref)
    fin = cref == R.FINITE
    assert np.array_equal(bits(db_clean)[fin], bits(db)[fin])


@pytest.mark.parametrize("tile", ["s", "q", "x"])
@pytest.mark.parametrize("M,N,K", [(200, 192, 128), (520, 448, 192)])
@pytest.mark.parametrize("with_src", [True, False], ids=["relu_src", "null"])
def test_dgrad_bf16(hip, env, tile, M, N, K, with_src):
    env("CODAE_GEMM_TILE", tile)
    rng = np.random.default_rng(11 * M + N + K)
    dy = rbf(rng.standard_normal((M, N))); W = rbf(rng.standard_normal((N, K)) * 2 / math.sqrt(N)); h = rbf(rng.standard_normal((M, K)))
    dyp, Wp = dy.copy(), W.copy()
    tdx, _ = R.plant_backward(dyp, Wp)
    hd = up(h, True) if with_src else None
    res = []
    for a, b in ((dy, W), (dyp, Wp)):
        dx = out((M, K), torch.bfloat16); db = out((K,)); ws = out(((M + 63) // 64 * K,))
        ad, bd = up(a, True), up(b, True)
        hip.check(hip.lib().codae_dgrad_bf16(hip.ptr(ad), hip.ptr(bd), hip.ptr(hd), hip.ptr(dx), hip.ptr(db), hip.ptr(ws),
                                             M, N, K, hip.current_stream()))
        sync()
        res.append((dx, db))
    src = h if with_src else None
    ref = R.dgrad_relu_ref(dyp, Wp, src)
    R.assert_same(res[0][0].double(), R.dgrad_relu_ref(dy, W, src), BF16_RTOL, BF16_ATOL)
    R.assert_same(res[1][0].double(), ref, BF16_RTOL, BF16_ATOL)
    same_bits_outside(res[0][0], res[1][0], tdx)
    check_colsum(res[0][1], res[1][1], ref)
    assert np.allclose(res[0][1].cpu().numpy(), res[0][0].double().cpu().numpy().sum(0), rtol=1e-3, atol=1e-2)


@pytest.mark.parametrize("mode,M,N,K", F32_BWD)
def test_wgrad_f32(hip, env, mode, M, N, K):
    """dW = dy^T x, db = colsum(dy): the NaN dy[M-1, N//2] makes exactly row N//2 of dW and db[N//2] NaN, the +Inf dy[0, 0]
    row 0 of dW +-Inf by the sign of x[0, :] and db[0] +Inf.  x3: NaN allowed in row 0 of dW (not in db: summed in fp32)."""
    env("CODAE_F32_GEMM", mode)
    rng = np.random.default_rng(M * N + K)
    dy, x = rng.standard_normal((M, N)).astype(np.float32), rng.standard_normal((M, K)).astype(np.float32)
    dyp = dy.copy()
    _, tdw = R.plant_backward(dyp, np.zeros((N, K)))
    res = []
    for a in (dy, dyp):
        dW = out((N, K)); db = out((N,))
        ad, xd = up(a), up(x)
        hip.check(hip.lib().codae_wgrad_f32(hip.ptr(ad), hip.ptr(xd), hip.ptr(dW), hip.ptr(db), M, N, K, hip.current_stream()))
        sync()
        res.append((dW, db))
    atol = 1e-4 * math.sqrt(M)
    for (dW, db), d in zip(res, (dy, dyp)):
        rW, rb = R.wgrad_ref(d, x)
        R.assert_same(dW.double(), rW, 0, atol, allow_nan_at=row0((N, K)) if mode == "x3" and d is dyp else None)
        R.assert_same(db.double(), rb, 0, atol)
    same_bits_outside(res[0][0], res[1][0], tdw)
    same_bits_outside(res[0][1], res[1][1], tdw[:, 0])
    assert torch.isnan(res[1][0][N // 2]).all() and torch.isnan(res[1][1][N // 2])
    assert float(res[1][1][0]) == inf


@pytest.mark.parametrize("M,N,K", [(512, 192, 128), (1536, 520, 200)])
@pytest.mark.parametrize("slabs", [True, False], ids=["slabs", "no-slabs"])
def test_wgrad_bf16(hip, M, N, K, slabs):
    rng = np.random.default_rng(M + N * K)
    dy, x = rbf(rng.standard_normal((M, N))), rbf(rng.standard_normal((M, K)))
    dyp = dy.copy()
    _, tdw = R.plant_backward(dyp, np.zeros((N, K)))
    ws = torch.empty(8 * N * K, device=DEV) if slabs else None
    res = []
    for a in (dy, dyp):
        dW = out((N, K))
        ad, xd = up(a, True), up(x, True)
        hip.check(hip.lib().codae_wgrad_bf16(hip.ptr(ad), hip.ptr(xd), hip.ptr(dW), hip.ptr(ws), 8 * N * K * 4 if slabs else 0,
                                             M, N, K, hip.current_stream()))
        sync()
        res.append(dW)
    # fp32 accumulation of M exact bf16 products of unit scale: the fp32 kernels' bound
    for dW, d in zip(res, (dy, dyp)):
        R.assert_same(dW.double(), R.wgrad_ref(d, x)[0], 1e-3, 1e-4 * math.sqrt(M))
    same_bits_outside(res[0], res[1], tdw)


def dgrad_act_problem(M, N, K, module, bf16_ops):
    """dy, W and a saved activation h = act(v) for the data gradient of one layer.  v is drawn on the bf16 grid inside
    [-4, 4]: where the activation passes v through (or scales it) h is then exact in either storage type, and a saturating
    activation's output stays far enough from its limit that rounding h cannot take the derivative, which the kernels read
    off h, to 0 or past it (ELU at v = -8 rounds to -1 in bf16: a property of the storage type, not of the kernel)."""
    rng = np.random.default_rng(M + 5 * N + K)
    dy = rng.standard_normal((M, N)).astype(np.float32)
    W = (rng.standard_normal((N, K)) / math.sqrt(N)).astype(np.float32)
    v = rbf(np.clip(rng.standard_normal((M, K)) * 3, -4, 4))
    if isinstance(module, nn.Softplus):
        # torch's Softplus jumps DOWN at b v = t (from log1p(e^t) to t), so an output with b y in (t, log1p(e^t)] has two
        # preimages with derivatives 1 and sigmoid(t): no derivative-from-output can tell them apart (off by 6.7e-3 at
        # t = 5, 2e-9 at the default 20).  Keep v out of the lower preimage band; 1/16 stays on the bf16 grid.
        b_, t_ = float(module.beta), float(module.threshold)
        band = (v * b_ <= t_) & (v * b_ > 2 * t_ - math.log1p(math.exp(t_)) - 1e-3)
        v[band] += 0.0625
    if bf16_ops:
        dy, W = rbf(dy), rbf(W)
    dyp, Wp = dy.copy(), W.copy()
    tdx, _ = R.plant_backward(dyp, Wp)
    h, ref_clean = R.dgrad_act_ref(dy, W, module, v)
    _, ref = R.dgrad_act_ref(dyp, Wp, module, v)
    return dy, W, dyp, Wp, h, tdx, ref_clean, ref


@pytest.mark.parametrize("kind", range(len(KINDS)), ids=KIND_IDS)
@pytest.mark.parametrize("f32_gemm", [None, "native"], ids=["default", "native"])
def test_dgrad_act_f32(hip, env, kind, f32_gemm):
    """dx = (dy W) act'(h) against torch's float64 autograd: ReLU, ReLU6 and Hardsigmoid select (0 under a dead unit even for a
    NaN gradient), the other kinds multiply.  Default dispatch: NaN allowed in row 0 (plane kernel, contract point 5)."""
    env("CODAE_F32_GEMM", f32_gemm)
    M, N, K = 200, 136, 128
    module, (k, p0, p1, p2) = engine_act(kind)
    dy, W, dyp, Wp, h, tdx, ref_clean, ref = dgrad_act_problem(M, N, K, module, False)
    dxs = []
    for a, b in ((dy, W), (dyp, Wp)):
        dx, ad, bd, hd = out((M, K)), up(a), up(b), up(h)
        hip.check(hip.lib().codae_dgrad_act_f32(hip.ptr(ad), hip.ptr(bd), hip.ptr(hd), hip.ptr(dx), M, N, K, k, p0, p1, p2,
                                                hip.current_stream()))
        sync()
        dxs.append(dx)
    R.assert_same(dxs[0].double(), ref_clean, 1e-3, 1e-5)
    R.assert_same(dxs[1].double(), ref, 1e-3, 1e-5, allow_nan_at=row0((M, K)) if f32_gemm is None else None)
    same_bits_outside(dxs[0], dxs[1], tdx)


@pytest.mark.parametrize("kind", range(len(KINDS)), ids=KIND_IDS)
def test_dgrad_act_bf16(hip, kind):
    M, N, K = 200, 128, 192
    module, (k, p0, p1, p2) = engine_act(kind)
    dy, W, dyp, Wp, h, tdx, ref_clean, ref = dgrad_act_problem(M, N, K, module, True)
    res = []
    for a, b in ((dy, W), (dyp, Wp)):
        dx = out((M, K), torch.bfloat16); db = out((K,)); ws = out(((M + 63) // 64 * K,))
        ad, bd, hd = up(a, True), up(b, True), up(h, True)
        hip.check(hip.lib().codae_dgrad_act_bf16(hip.ptr(ad), hip.ptr(bd), hip.ptr(hd), hip.ptr(dx), hip.ptr(db),
                                                 hip.ptr(ws), M, N, K, k, p0, p1, p2, hip.current_stream()))
        sync()
        res.append((dx, db))
    # (the existing tolerance of the generic bf16 data gradient: two roundings to bf16 and the derivative of a rounded h)
    R.assert_same(res[0][0].double(), ref_clean, 2e-2, 2e-2)
    R.assert_same(res[1][0].double(), ref, 2e-2, 2e-2)
    same_bits_outside(res[0][0], res[1][0], tdx)
    check_colsum(res[0][1], res[1][1], ref)


# ---------------------------------------------------------------------------------------------------------------------
# C. elementwise
# ---------------------------------------------------------------------------------------------------------------------
def test_mse_loss_propagates_and_recovers(hip):
    rng = np.random.default_rng(3)
    B, io = 77, 48
    n = B * io
    x = rng.random((B, io), dtype=np.float32); y = rng.random((B, io), dtype=np.float32)
    fm = (rng.random((B, io)) > 0.3).astype(np.float32)
    yp = y.copy()
    yp[3, 5], yp[10, 7] = nan, inf
    fm[3, 5] = fm[10, 7] = 0                       # blanked: both count into the partial sum too
    sc = torch.zeros(hip.S_COUNT, dtype=torch.float64, device=DEV)
    dy = out((B, io))
    xd, fd, ypd, yd = up(x), up(fm), up(yp), up(y)
    args = lambda yy: (hip.ptr(xd), hip.ptr(yy), hip.ptr(fd), hip.ptr(dy), n, 1.0 / n, hip.ptr(sc), hip.current_stream())  # noqa: E731
    hip.check(hip.lib().codae_mse_loss_fwd_bwd(*args(ypd)))
    sync()
    with np.errstate(all="ignore"):
        ref = -2 * (x.astype(np.float64) - yp) / n
    R.assert_same(dy.double(), ref, 1e-5, 1e-9)
    assert float(dy[10, 7]) == inf and math.isnan(float(dy[3, 5]))
    for k in (hip.S_SQ_FULL, hip.S_SQ_PARTIAL, hip.S_LAST_LOSS):
        assert not math.isfinite(float(sc[k])), k
    sc.zero_()
    hip.check(hip.lib().codae_mse_loss_fwd_bwd(*args(yd)))
    sync()
    d = x.astype(np.float64) - y
    assert abs(float(sc[hip.S_SQ_FULL]) - (d ** 2).sum()) < 1e-3 and abs(float(sc[hip.S_LAST_LOSS]) - (d ** 2).mean()) < 1e-6
    assert torch.isfinite(dy).all()


def adam_case(hip, n, grad, p0, clip, dtype):
    """one codae_clip_adam step from zero moments against clip_grad_norm_ + torch.optim.Adam in `dtype` on the CPU"""
    ref_p = torch.nn.Parameter(torch.tensor(p0).to(dtype))
    opt = torch.optim.Adam([ref_p], lr=1e-3, weight_decay=1e-2)
    ref_p.grad = torch.tensor(grad).to(dtype)
    if clip:
        torch.nn.utils.clip_grad_norm_([ref_p], 1.0)
    opt.step()
    st = opt.state[ref_p]
    p, g = up(p0), up(grad)
    m = torch.zeros(n, device=DEV); v = torch.zeros(n, device=DEV)
    sc = torch.zeros(hip.S_COUNT, dtype=torch.float64, device=DEV)
    hp = hip.Hyper(1e-3, 1e-2, 0.9, 0.999, 1e-8, 1.0 if clip else 0.0, 1, 0.0)
    hip.check(hip.lib().codae_clip_adam(hip.ptr(p), hip.ptr(g), hip.ptr(m), hip.ptr(v), n, C.byref(hp), hip.ptr(sc), hip.current_stream()))
    sync()
    gsq = float(sc[hip.S_GRAD_SQ]) + float(sc[hip.S_GRAD_SQ_SLOTS:hip.S_GRAD_SQ_SLOTS + hip.S_N_SLOTS].sum())
    return p, m, v, gsq, ref_p.detach(), st["exp_avg"], st["exp_avg_sq"]


@pytest.mark.parametrize("n", [5, 1000])
@pytest.mark.parametrize("case", ["nan", "inf", "overflow", "nan-noclip", "inf-noclip"])
def test_clip_adam_nonfinite_gradients(hip, n, case):
    """nan: a NaN norm gives a NaN coefficient - every parameter and both moments NaN, as torch.  inf: an infinite norm
    gives coefficient 0 - NaN (Inf * 0) at that element, plain weight-decay updates elsewhere.  overflow: finite gradients
    of 3e19 whose sum of squares exceeds fp32's range - the norm kernels sum g^2 in fp32 as torch's fp32 clip does, so the
    norm is +Inf and the coefficient 0; the reference for this case is therefore torch in float32 (in float64 the norm is
    finite).  noclip (max_grad_norm = 0): only the non-finite elements go NaN, as torch's Adam alone does."""
    rng = np.random.default_rng(n)
    p0 = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 3).astype(np.float32)
    k = n // 2
    if case.startswith("nan"):
        g[k] = nan
    elif case.startswith("inf"):
        g[k] = inf
    else:
        g[:] = 3e19
    clip = not case.endswith("noclip")
    p, m, v, gsq, rp, rm, rv = adam_case(hip, n, g, p0, clip, torch.float32 if case == "overflow" else torch.float64)
    R.assert_same(p.double(), rp.double(), 1e-3, 1e-5)
    R.assert_same(m.double(), rm.double(), 1e-3, 1e-7)
    if case != "overflow":        # (v = 1e-3 g^2 of a clipped gradient; under "overflow" it is (0.01 p)^2 1e-3: compare loosely scaled)
        R.assert_same(v.double(), rv.double(), 1e-3, 1e-9)
    others = np.arange(n) != k
    if case == "nan":
        assert torch.isnan(p).all() and torch.isnan(m).all() and torch.isnan(v).all() and math.isnan(gsq)
    elif case == "inf":
        assert math.isnan(float(p[k])) and torch.isfinite(p.cpu()[others]).all() and gsq == inf
    elif case == "overflow":
        assert gsq == inf and torch.isfinite(p).all()
        assert np.allclose(v.cpu().numpy(), 1e-3 * (0.01 * p0.astype(np.float64)) ** 2, rtol=1e-3, atol=0)   # coefficient exactly 0
    else:
        assert math.isnan(float(p[k])) and torch.isfinite(p.cpu()[others]).all()


def test_span_sumsq_and_update_span_with_a_nan_norm(hip):
    """the sharded data-parallel update (DataParallel._sharded_update): a NaN in one rank's share of sum g^2 reaches every
    rank through the all-reduce; each then updates its span [lo, hi) with it - every element of the span, both moments and
    the bf16 shadow go NaN, nothing outside the span is touched.  total_sq = +Inf: coefficient 0, a weight-decay-only step."""
    from codae.hip.engine import DaeEngine
    eng = DaeEngine(R.SCHEDULE, 64, "bf16", torch.device(DEV))
    _, _, params = R.step_problem(None)
    eng.load_params(params)
    g = torch.Generator().manual_seed(1)
    eng.grads.copy_(torch.randn(eng.n_param, generator=g))
    lo, hi = eng.w_off[1], eng.w_off[1] + 64 * 64
    acc = eng.new_accumulator()
    eng.span_sumsq(lo, hi, acc)
    sync()
    assert abs(float(acc) - float((eng.grads[lo:hi].double() ** 2).sum())) <= 1e-5 * float(acc)
    eng.grads[lo + 5] = nan
    acc = eng.new_accumulator()
    eng.span_sumsq(lo, hi, acc)
    sync()
    assert math.isnan(float(acc))
    before = [t.clone() for t in (eng._params, eng.adam_m, eng.adam_v, eng.shadow)]
    eng.step_update_span(eng.hyper(1e-3, 1e-2, 1.0, step=1), lo, hi, acc)
    sync()
    for t, b in zip((eng._params, eng.adam_m, eng.adam_v, eng.shadow), before):
        assert torch.isnan(t[lo:hi]).all()
        assert np.array_equal(bits(t[:lo]), bits(b[:lo])) and np.array_equal(bits(t[hi:]), bits(b[hi:]))
    # +Inf: coefficient 0 on another span (finite gradients): p <- Adam(weight decay alone)
    lo2, hi2 = eng.w_off[0], eng.w_off[0] + 64
    p0 = eng._params[lo2:hi2].double().cpu()
    eng.step_update_span(eng.hyper(1e-3, 1e-2, 1.0, step=1), lo2, hi2, torch.tensor([inf], dtype=torch.float64, device=DEV))
    sync()
    ref = torch.nn.Parameter(p0.clone())
    ref.grad = torch.zeros_like(p0)
    torch.optim.Adam([ref], lr=1e-3, weight_decay=1e-2).step()
    R.assert_same(eng._params[lo2:hi2].double(), ref.detach(), 1e-3, 1e-5)


def test_corrupt_is_a_product(hip):
    """codae_corrupt = oracle.corrupt = input * mask: a NaN or Inf under a 0 mask is NaN (the reference multiplies)"""
    from oracle import dae_oracle as O
    rng = np.random.default_rng(0)
    x = rng.random((37, 11)).astype(np.float32)
    fm = (rng.random((37, 11)) > 0.4).astype(np.float32)
    x[3, 4], fm[3, 4] = nan, 0
    x[5, 6], fm[5, 6] = inf, 0
    x[7, 8], fm[7, 8] = -inf, 1
    o, xd, fd = out((37, 11)), up(x), up(fm)
    hip.check(hip.lib().codae_corrupt(hip.ptr(xd), hip.ptr(fd), hip.ptr(o), x.size, hip.current_stream()))
    sync()
    with np.errstate(all="ignore"):
        ref = O.corrupt(x, fm)
    assert np.isnan(ref[3, 4]) and np.isnan(ref[5, 6]) and ref[7, 8] == -inf
    assert np.array_equal(o.cpu().numpy(), ref, equal_nan=True)


@pytest.mark.parametrize("n", [7, 1003])
def test_cast_f32_to_bf16_is_torchs_rounding(hip, n):
    """codae_cast_f32_to_bf16 (the shadow refresh) bit for bit against torch.Tensor.bfloat16(): NaN, +-Inf, the two
    neighbours of the overflow threshold (3.4e38 rounds to Inf, 3.39e38 to the largest finite bf16), a denormal, -0, exact
    ties on even and odd mantissas, random values.  n = 7: the scalar tail alone; 1003: the float4 body and a 3-element tail.
    A NaN must come out a NaN; its payload is not compared, torch's own scalar and vector CPU conversions disagree on it
    (0x7fc0 and 0xffff)."""
    rng = np.random.default_rng(2)
    special = np.array([nan, inf, -inf, 3.4e38, 3.39e38, -0.0, 1e-40, 0.0], dtype=np.float32)
    hi16 = np.arange(0x3f78, 0x3f88, dtype=np.uint32)                       # around 1.0, even and odd, both signs below
    ties = ((hi16 << 16) | 0x8000).view(np.float32)
    ties = np.concatenate([ties, -ties])
    rand = (rng.standard_normal(1000) * np.exp(rng.uniform(-30, 30, 1000))).astype(np.float32)
    src = np.concatenate([special, ties, rand])[:n].copy()
    dst, sd = torch.zeros(n, dtype=torch.bfloat16, device=DEV), up(src)
    hip.check(hip.lib().codae_cast_f32_to_bf16(hip.ptr(sd), hip.ptr(dst), n, hip.current_stream()))
    sync()
    want = torch.tensor(src).bfloat16()
    isn = np.isnan(src)
    # (0x7fc0 / 0xffff: torch's two conversions of this quiet NaN; a signalling pattern or a payload collapsed to Inf is neither)
    assert all(int(b) & 0xffff in (0x7fc0, 0xffff) for b in bits(dst)[isn])
    assert np.array_equal(bits(dst)[~isn], bits(want)[~isn]), np.flatnonzero(bits(dst) != bits(want))[:8]


# ---------------------------------------------------------------------------------------------------------------------
# D. whole steps
# ---------------------------------------------------------------------------------------------------------------------
def make_trainer(scenario, precision, use_graph=False, data_from=None):
    from codae.train import HipEmbeddingTrainer
    data, mask, params = R.step_problem(scenario)
    if data_from is not None:
        data = R.step_problem(data_from)[0]
    tr = HipEmbeddingTrainer(R.SCHEDULE, torch.tensor(data), torch.tensor(mask[None, :]).to(torch.uint8),
                             torch.zeros((R.B, 1), dtype=torch.int32), R.LR, R.WD, R.CLIP, max_batch=R.B, precision=precision,
                             device=DEV, use_graph=use_graph)
    tr.load_params(params)
    return tr


def all_rows():
    return torch.arange(R.B, dtype=torch.int32, device=DEV)


def one_step(scenario, precision, use_graph=False):
    tr = make_trainer(scenario, precision, use_graph)
    tr.train_batch(all_rows(), run=0)
    sync()
    return tr, tr.engine.read_scalars()[3]


def assert_step_went_nan(tr, loss, scenario, precision):
    """contract points 4 and 3 of include/codae_hip.h ("Non-finite values"): a non-finite loss; of the reference's class (the fp32 engine's plane kernel may
    turn the reference's +Inf into NaN: contract point 5); every parameter, both moments and the bf16 shadows NaN"""
    ref = R.reference_step(scenario, torch.float32)
    assert not math.isfinite(loss), "finite loss %r on a step whose reference loss is %r" % (loss, ref["loss"])
    got, want = int(R.classes(np.float64(loss))), int(R.classes(np.float64(ref["loss"])))
    assert got == want or (precision == "f32" and got == R.NAN), (loss, ref["loss"])
    eng = tr.engine
    for l, (w, b) in enumerate(tr.params()):
        assert torch.isnan(w).all() and torch.isnan(b).all(), (l, int(torch.isfinite(w).sum()), int(torch.isfinite(b).sum()))
        for flat in (eng.adam_m, eng.adam_v):
            assert torch.isnan(eng._view(flat, l, False)).all() and torch.isnan(eng._view(flat, l, True)).all(), l
        if eng.shadow is not None:
            assert torch.isnan(eng._view(eng.shadow, l, False)).all(), l


@pytest.mark.parametrize("scenario", R.SCENARIOS)
def test_step_f32_with_a_nonfinite_reference_loss_goes_all_nan(scenario):
    tr, loss = one_step(scenario, "f32")
    assert_step_went_nan(tr, loss, scenario, "f32")


@pytest.mark.parametrize("scenario", R.SCENARIOS)
def test_step_bf16_with_a_nonfinite_reference_loss_goes_all_nan(scenario, step_path):
    tr, loss = one_step(scenario, "bf16")
    assert tr.engine.step_path(R.B) == step_path
    assert_step_went_nan(tr, loss, scenario, "bf16")


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_control_step_is_finite_and_equals_the_reference(precision):
    """the same problem with nothing planted: finite, and the reference step (float64) at the tolerances the parity tests and
    smoke() use for one step (fp32: rtol 1e-3 / atol 1e-5; bf16: 2e-2 on the loss, atol 2.5e-3 on the parameters)"""
    tr, loss = one_step(None, precision)
    ref = R.reference_step(None, torch.float64)
    tol, atol = (1e-3, 1e-5) if precision == "f32" else (2e-2, 2.5e-3)
    assert math.isfinite(loss) and abs(loss - ref["loss"]) <= tol * ref["loss"], (loss, ref["loss"])
    for (w, b), (rw, rb) in zip(tr.params(), ref["params"]):
        assert np.allclose(w.double().cpu().numpy(), rw, rtol=1e-3, atol=atol) and np.allclose(b.double().cpu().numpy(), rb, rtol=1e-3, atol=atol)


def eval_s5(precision, step_path=None):
    ys = []
    for scenario in (None, "S5"):
        tr = make_trainer(scenario, precision)
        assert step_path is None or tr.engine.step_path(R.B) == step_path
        tr.engine.zero_metric_sums()
        y = tr.eval_batch(all_rows(), run=0, want_y=True)
        sync()
        ys.append((y.clone(), tr.epoch_sums()))
    (y0, sums0), (y1, sums1) = ys
    assert torch.isnan(y1[R.B - 1]).all()
    assert np.array_equal(bits(y0[:R.B - 1]), bits(y1[:R.B - 1]))
    assert all(math.isfinite(s) for s in sums0) and all(math.isnan(s) for s in sums1), (sums0, sums1)
    ref = R.reference_step("S5", torch.float64)["y"]
    assert np.array_equal(R.classes(y1), R.classes(ref))


def test_eval_step_f32_keeps_a_nan_row_to_itself():
    eval_s5("f32")


def test_eval_step_bf16_keeps_a_nan_row_to_itself(step_path):
    eval_s5("bf16", step_path)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_graph_replay_gives_the_classes_of_the_eager_step(precision):
    tr_e, loss_e = one_step("S1", precision)
    tr_g, loss_g = one_step("S1", precision, use_graph=True)
    assert R.classes(np.float64(loss_g)) == R.classes(np.float64(loss_e))
    assert_step_went_nan(tr_g, loss_g, "S1", precision)
    for (w, b), (w2, b2) in zip(tr_e.params(), tr_g.params()):
        assert np.array_equal(R.classes(w), R.classes(w2)) and np.array_equal(R.classes(b), R.classes(b2))


@pytest.mark.parametrize("S,E,B", [(3, 128, 1000), (3, 320, 8192)], ids=["tile128x128", "tile256x192"])
def test_fused_loss_epilogues_report_a_nan_loss(monkeypatch, S, E, B):
    """the bf16 per-layer step with the MSE loss folded into the last forward GEMM, on both of its tiles (the shapes of
    test_fused_loss_epilogue_matches_separate_loss_kernel), with a NaN at W[1][5, 7]: NaN loss, every parameter NaN"""
    from codae.train import HipEmbeddingTrainer
    from oracle import dae_oracle as O
    monkeypatch.setenv("CODAE_NO_CHAIN", "1")
    monkeypatch.delenv("CODAE_NO_FUSED_LOSS", raising=False)
    io = S * E
    rng = np.random.default_rng(11)
    N = B + 100
    data = rng.random((N, io), dtype=np.float32)
    sched = O.layer_schedule(io, io, 2, 2, False, "embedding")
    params = [(w.copy(), b.copy()) for w, b in O.init_params(sched, rng)]
    params[1][0][5, 7] = nan
    bm, _, _ = O.corrupter_tables([{"size": E, "position": s * E} for s in range(S)], 1)
    mtu = rng.integers(0, S, (N, 1)).astype(np.int32)
    idx = torch.tensor(rng.permutation(N)[:B], dtype=torch.int32, device=DEV)
    tr = HipEmbeddingTrainer(sched, torch.tensor(data), torch.tensor(bm).to(torch.uint8), torch.tensor(mtu), 1e-3, 1e-4, 1.0,
                             max_batch=B, precision="bf16", device=DEV)
    tr.load_params(params)
    assert tr.engine.step_path(B) == "layers"
    tr.train_batch(idx, run=0)
    sync()
    assert math.isnan(tr.engine.read_scalars()[3])
    for l, (w, b) in enumerate(tr.params()):
        assert torch.isnan(w).all() and torch.isnan(b).all(), l


@pytest.mark.parametrize("factory", [None, nn.Hardsigmoid], ids=["default-relu", "hardsigmoid"])
def test_dropin_forward_with_a_nan_hidden_bias(factory):
    """codae.model class in fp32 (the constructor's default activation, ReLU, and nn.Hardsigmoid) with a NaN in a hidden
    bias: the forward output is NaN exactly where torch's CPU float64 forward of the same modules is.  (The classes build
    their stack by calling activation(True), as the reference does, so activation=None cannot be constructed; the identity
    epilogue with a NaN is covered through the C ABI by test_linear_f32 / test_linear_bf16 with relu = 0.)"""
    from codae.model import EmbeddingDenoisingAutoencoder
    torch.manual_seed(5)
    kw = {} if factory is None else {"activation": factory}
    m = EmbeddingDenoisingAutoencoder(192, 64, 64, 2, 2, False, **kw).to(DEV)
    m.precision = "f32"
    with torch.no_grad():
        m.input_layer[0].bias[5] = nan
    x = np.random.default_rng(6).random((R.B, 192)).astype(np.float32)
    with torch.no_grad():
        y = m(torch.tensor(x, device=DEV))
        sync()
        ref = cpu_copy(m)(torch.tensor(x, dtype=torch.float64)).numpy()
    assert np.isnan(ref).any()
    R.assert_same(y.double(), ref, 1e-3, 1e-5)
