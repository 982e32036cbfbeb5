"""Float64 / torch-CPU references for the non-finite contract (include/codae_hip.h, "Non-finite values"): class maps, the
planting designs of the kernel tests, and the clipped Adam step of the whole-step scenarios.  No GPU, no HIP library."""
import numpy as np
import torch

FINITE, NEG_INF, POS_INF, NAN = 0, 1, 2, 3


def _np(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().double().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def classes(a):
    """int map of a: 0 finite, 1 -Inf, 2 +Inf, 3 NaN"""
    a = _np(a)
    out = np.zeros(a.shape, dtype=np.int8)
    out[np.isneginf(a)] = NEG_INF
    out[np.isposinf(a)] = POS_INF
    out[np.isnan(a)] = NAN
    return out


def assert_same(got, ref, rtol, atol, allow_nan_at=None):
    """got and ref have the same class map and their finite entries agree within rtol / atol.  Where the boolean mask
    allow_nan_at is set, got may be NaN instead of what ref holds (and nothing else instead)."""
    got, ref = _np(got), _np(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    cg, cr = classes(got), classes(ref)
    bad = cg != cr
    if allow_nan_at is not None:
        bad &= ~(np.asarray(allow_nan_at, dtype=bool) & (cg == NAN))
    if bad.any():
        where = np.argwhere(bad)
        first = tuple(where[0])
        raise AssertionError("%d entries of another class than the reference; first at %s: got %r, reference %r"
                             % (len(where), first, got[first], ref[first]))
    fin = (cg == FINITE) & (cr == FINITE)
    err = np.abs(got[fin] - ref[fin])
    tol = atol + rtol * np.abs(ref[fin])
    if (err > tol).any():
        k = int(np.argmax(err - tol))
        raise AssertionError("finite entries differ: got %r, reference %r (rtol %g, atol %g)" % (got[fin][k], ref[fin][k], rtol, atol))


# ---- planting -------------------------------------------------------------------------------------------------------
# (M, N, K) at which the class map of the planted forward was compared in float64, fp32 and a permuted bf16 product
PLANT_SHAPES = [(37, 11, 11), (130, 200, 77), (200, 132, 64), (8, 64, 64), (520, 448, 192), (200, 192, 128), (1, 1, 1)]


def plant_forward(x, W, b):
    """y = x W^T + b with four non-finite operands (in place; numpy arrays or CPU tensors):
      x[M-1, K//2] = NaN   the last row: the one a ragged tile's clamped loads read again
      x[0, 0] = +Inf       W[N-1, K-1] = NaN       b[N//2] = -Inf
    Returns the boolean [M, N] mask of the outputs that depend on one of them: rows 0 and M-1, columns N-1 and N//2.  Every
    output sees at most one Inf product plus the Inf bias, so no summation order can change a class."""
    M, K = x.shape
    N = W.shape[0]
    x[M - 1, K // 2] = float("nan")
    x[0, 0] = float("inf")
    W[N - 1, K - 1] = float("nan")
    b[N // 2] = float("-inf")
    touched = np.zeros((M, N), dtype=bool)
    touched[0, :] = touched[M - 1, :] = True
    touched[:, N - 1] = touched[:, N // 2] = True
    return touched


def plant_backward(dy, W):
    """dy[M-1, N//2] = NaN, dy[0, 0] = +Inf, W[N-1, K-1] = NaN (in place); the saved activations stay finite.
    Returns (touched_dx [M, K]: rows 0 and M-1, column K-1; touched_dW [N, K]: rows 0 and N//2 - what dy W and dy^T x
    can make non-finite)."""
    M, N = dy.shape
    K = W.shape[1]
    dy[M - 1, N // 2] = float("nan")
    dy[0, 0] = float("inf")
    W[N - 1, K - 1] = float("nan")
    tdx = np.zeros((M, K), dtype=bool)
    tdx[0, :] = tdx[M - 1, :] = True
    tdx[:, K - 1] = True
    tdw = np.zeros((N, K), dtype=bool)
    tdw[0, :] = tdw[N // 2, :] = True
    return tdx, tdw


# ---- float64 references ---------------------------------------------------------------------------------------------
def act64(module, v):
    """a torch.nn activation module (None: identity) on a float64 array, on the CPU"""
    v = _np(v)
    if module is None:
        return v
    with torch.no_grad():
        return module(torch.from_numpy(v.copy())).numpy()


def forward_ref(x, W, b, module=None):
    """act(x W^T + b) in float64; module: a torch.nn activation (not in place) or None"""
    with np.errstate(all="ignore"):
        v = _np(x) @ _np(W).T
        if b is not None:
            v = v + _np(b)
    return act64(module, v)


def dgrad_relu_ref(dy, W, h=None):
    """(dy W) selected by h > 0: a select, not a product - NaN * 0 would be NaN, torch's threshold_backward gives 0"""
    with np.errstate(all="ignore"):
        g = _np(dy) @ _np(W)
    return g if h is None else np.where(_np(h) > 0, g, 0.0)


def dgrad_act_ref(dy, W, module, v):
    """torch CPU float64 autograd of h = act(v) with the incoming gradient g = dy W: (h, dx).  The derivative is taken from
    the INPUT v here and from the saved output h in the kernels; with h finite the two agree."""
    with np.errstate(all="ignore"):
        g = _np(dy) @ _np(W)
    vt = torch.from_numpy(_np(v).copy()).requires_grad_(True)
    h = module(vt)
    h.backward(torch.from_numpy(g))
    return h.detach().numpy(), vt.grad.numpy()


def wgrad_ref(dy, x):
    with np.errstate(all="ignore"):
        return _np(dy).T @ _np(x), _np(dy).sum(0)


def forward_class_maps(M, N, K, seed=0):
    """class maps of the planted pre-activation in three arithmetics: numpy float64, torch fp32, and a product of the
    bf16-rounded operands summed over a permuted K (another order, another rounding); plus the touched mask"""
    rng = np.random.default_rng(seed + M + 3 * N + 7 * K)
    x = rng.standard_normal((M, K)); W = rng.standard_normal((N, K)); b = rng.standard_normal(N)
    touched = plant_forward(x, W, b)
    m64 = classes(forward_ref(x, W, b))
    xt, Wt, bt = (torch.tensor(a, dtype=torch.float32) for a in (x, W, b))
    m32 = classes(xt @ Wt.T + bt)
    perm = rng.permutation(K)
    xb, Wb = (t.bfloat16().double().numpy()[:, perm] for t in (xt, Wt))
    with np.errstate(all="ignore"):
        acc = np.zeros((M, N), dtype=np.float32)
        for k in range(K):
            acc = (acc + np.outer(xb[:, k], Wb[:, k]).astype(np.float32)).astype(np.float32)
        mbf = classes(acc + bt.numpy())
    return m64, m32, mbf, touched


# ---- whole steps ----------------------------------------------------------------------------------------------------
S, E, B = 3, 64, 40
IO = S * E
SCHEDULE = [(IO, E, True), (E, E, True), (E, IO, False)]
LR, WD, CLIP = 1e-3, 1e-2, 1.0
SCENARIOS = ("S1", "S2", "S3", "S4", "S5", "S6")


def step_problem(scenario=None):
    """(data [B, IO] fp32 in [0.1, 0.9) - positive, so that Inf * x keeps its sign -, mask [IO] with slot 0 blanked,
    params [(W, b)] fp32 from a seeded Xavier draw) with `scenario` planted; None: the finite control.
      S1 NaN at W[1][5, 7]            S2 NaN at b[0][11]
      S3 W[0][3, 64:] = W[0][9, 64:] = +Inf, W[1][:, 3] = |.|, W[1][:, 9] = -|.|   (Inf - Inf one layer later)
      S4 W[0][3, 100] = +Inf, W[1][:, 3] = |.|, W[2] = |.|                          (the loss is +Inf)
      S5 NaN at data[39, 100], the last row of the batch
      S6 S3 with the finite 3e38 in place of Inf: overflows in fp32 only"""
    rng = np.random.default_rng(20)
    data = (0.1 + 0.8 * rng.random((B, IO))).astype(np.float32)
    mask = np.ones(IO, dtype=np.float32)
    mask[:E] = 0
    params = []
    for k, n, _ in SCHEDULE:
        a = (6.0 / (k + n)) ** 0.5
        params.append([((rng.random((n, k)) * 2 - 1) * a).astype(np.float32), ((rng.random(n) * 2 - 1) * 0.1).astype(np.float32)])
    nan, inf = float("nan"), float("inf")
    if scenario == "S1":
        params[1][0][5, 7] = nan
    elif scenario == "S2":
        params[0][1][11] = nan
    elif scenario in ("S3", "S6"):
        big = inf if scenario == "S3" else 3e38
        params[0][0][3, E:] = big
        params[0][0][9, E:] = big
        params[1][0][:, 3] = np.abs(params[1][0][:, 3])
        params[1][0][:, 9] = -np.abs(params[1][0][:, 9])
    elif scenario == "S4":
        params[0][0][3, 100] = inf
        params[1][0][:, 3] = np.abs(params[1][0][:, 3])
        params[2][0][:] = np.abs(params[2][0])
    elif scenario == "S5":
        data[B - 1, 100] = nan
    elif scenario is not None:
        raise ValueError(scenario)
    return data, mask, [(w, b) for w, b in params]


def reference_model(params, dtype):
    mods = []
    for (w, b), (_, _, relu) in zip(params, SCHEDULE):
        lin = torch.nn.Linear(w.shape[1], w.shape[0]).to(dtype)
        with torch.no_grad():
            lin.weight.copy_(torch.tensor(w).to(dtype))
            lin.bias.copy_(torch.tensor(b).to(dtype))
        mods.append(lin)
        if relu:
            mods.append(torch.nn.ReLU())
    return torch.nn.Sequential(*mods)


_STEP_CACHE = {}


def reference_step(scenario, dtype=torch.float32):
    """One step of the reference's loop body on the CPU in `dtype`: y = model(data * mask), MSELoss(y, data), backward,
    clip_grad_norm_(params, 1), Adam(lr 1e-3, weight_decay 1e-2).step().  Returns {"loss": float, "y": array,
    "params": [(W, b)] after the step}.  Computed once per (scenario, dtype); callers must not modify the result."""
    key = (scenario, dtype)
    if key not in _STEP_CACHE:
        data, mask, params = step_problem(scenario)
        model = reference_model(params, dtype)
        x = torch.tensor(data).to(dtype)
        y = model(x * torch.tensor(mask).to(dtype))
        loss = torch.nn.MSELoss()(y, x)
        opt = torch.optim.Adam(model.parameters(), lr=LR, weight_decay=WD)
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), CLIP)
        opt.step()
        lins = [m for m in model if isinstance(m, torch.nn.Linear)]
        _STEP_CACHE[key] = {"loss": float(loss.detach()), "y": y.detach().double().numpy(),
                            "params": [(m.weight.detach().double().numpy(), m.bias.detach().double().numpy()) for m in lins]}
    return _STEP_CACHE[key]
