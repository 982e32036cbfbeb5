"""float64 numpy restatement of the optimizer kinds and the learning-rate schedule of include/codae_hip.h ("Optimizer and
schedule"), with the rounding-error bounds an fp32 evaluation must stay inside, written from the definition for the tests: it shares
no code with the kernels or with codae.tool.optimizer.  Hyper (the fp32 hyperparameters, widened) and clip_coef32 are adam_ref's.

  w(t) = W > 0 and t <= W ? t / W : 1,  q(t) = clamp((t - W) / (T - W), 0, 1)
  f(t) = w(t) * {constant 1 | cosine mf + (1 - mf)(1 + cos(pi q)) / 2 | linear 1 - (1 - mf) q | step gamma^floor((t - 1) / period)}
  lr_t = float32(lr f(t))                                                                               (factor, lr_t)
  adam   g' = g coef + wd p;  m' = b1 m + (1 - b1) g';  v' = b2 v + (1 - b2) g'^2;  d = v'
  adamw  g' = g coef;  p1 = p (1 - lr_t wd);  m', v' from g';  d = v'
    amsgrad: vmax' = maximum(vmax, v'), NaN staying;  d = vmax'
         p' = (p | p1) - lr_t / bc1 m' / (sqrt(d) / sqrt(bc2) + eps)
  sgd    g' = g coef + wd p;  m' = mu m + g';  u = nesterov ? g' + mu m' : m';  p' = p - lr_t u;  v untouched     (step64)

bounds(): adam_ref.bounds (u = 2^-24; G, A, Bv as there, with G = |g coef| alone under adamw) with these changes:
  - lr_t takes lr's place, and 2 u |upd| is added for ITS rounding: the device's double cos / pow may differ from numpy's in the last
    place before the cast to fp32;
  - adamw: one u |p| more, for p (1 - lr_t wd);
  - amsgrad: d = vmax' in the denominator term; tol_vmax = tol_v (a maximum moves by no more than its operand);
  - sgd: tol_m = 4 u (|mu m| + G);  tol_p = 2 u |p'| + lr_t (tol_m (1 + mu) + 4 u (|g'| + |mu m'|)) + 2 u |upd|, upd = lr_t u.
They are measured against step32_emulated (tests/test_optimizer_host.py asserts the worst |error| / bound <= 0.75), never against a
GPU run.
"""
import collections
import math

import numpy as np

import adam_ref as AR
from adam_ref import U, Hyper, clip_coef32, hyper, hyper_of_struct, planted_state  # noqa: F401  (re-used by import, as they are)

# kind: "adam" | "adamw" | "sgd"; sched: "constant" | "cosine" | "linear" | "step"; mu, min_factor, gamma: fp32 values, widened
Opt = collections.namedtuple("Opt", "kind amsgrad mu nesterov sched warmup total period min_factor gamma")


def opt(kind="adam", amsgrad=False, momentum=0.0, nesterov=False, sched="constant", warmup=0, total=0, period=1, min_factor=0.0,
        gamma=1.0):
    w = AR._w
    return Opt(kind, bool(amsgrad), w(momentum), bool(nesterov), sched, int(warmup), int(total), int(period), w(min_factor), w(gamma))


def opt_of(o):
    """From a codae.tool.Optimizer."""
    s = o.schedule
    return opt(o.kind, o.amsgrad, o.momentum, o.nesterov, s.kind, s.warmup, s.total or 0, s.period, s.min_factor, s.gamma)


def factor(o, t):
    """f(t), float64."""
    t = float(t)
    W = float(o.warmup)
    w = t / W if o.warmup > 0 and t <= W else 1.0
    if o.sched == "constant":
        return w
    if o.sched == "step":
        return w * o.gamma ** math.floor((t - 1.0) / o.period)
    q = min(max((t - W) / (o.total - W), 0.0), 1.0)
    if o.sched == "cosine":
        return w * (o.min_factor + (1.0 - o.min_factor) * (1.0 + math.cos(math.pi * q)) / 2.0)
    assert o.sched == "linear", o.sched
    return w * (1.0 - (1.0 - o.min_factor) * q)


def lr_t(h, o, rounded=True):
    """lr f(t) as the update uses it: rounded to fp32 (and widened again).  rounded=False: the float64 product, what a float64
    torch optimizer under LambdaLR uses."""
    x = h.lr * factor(o, h.t)
    return float(np.float32(x)) if rounded else x


def _f64(a):
    return None if a is None else np.asarray(a).astype(np.float64)


def step64(p, g, m, v, vmax, h, o, coef, rounded_lr=True):
    """{"p", "m", "v", "vmax"} in float64 from the inputs as given (v / vmax None where the kind does not keep them)."""
    p, g, m, v, vmax = (_f64(a) for a in (p, g, m, v, vmax))
    c = float(np.float32(coef))
    lr = lr_t(h, o, rounded_lr)
    if o.kind == "sgd":
        g1 = g * c + h.wd * p
        m1 = o.mu * m + g1
        u = g1 + o.mu * m1 if o.nesterov else m1
        return {"p": p - lr * u, "m": m1, "v": None, "vmax": None}
    bc1, bc2 = AR.bias_corrections(h)
    if o.kind == "adamw":
        g1 = g * c
        p = p * (1.0 - lr * h.wd)
    else:
        assert o.kind == "adam", o.kind
        g1 = g * c + h.wd * p
    m1 = h.b1 * m + (1.0 - h.b1) * g1
    v1 = h.b2 * v + (1.0 - h.b2) * g1 * g1
    d, x1 = v1, None
    if o.amsgrad:
        with np.errstate(invalid="ignore"):
            x1 = np.where(np.isnan(v1) | np.isnan(vmax), np.nan, np.maximum(vmax, v1))
        d = x1
    return {"p": p - lr / bc1 * m1 / (np.sqrt(d) / np.sqrt(bc2) + h.eps), "m": m1, "v": v1, "vmax": x1}


def bounds(p, g, m, v, vmax, h, o, coef):
    """{"p", "m", "v", "vmax"}: what |fp32 result - step64| may reach, per element (module docstring); None where there is no state."""
    p, g, m, v, vmax = (_f64(a) for a in (p, g, m, v, vmax))
    c = float(np.float32(coef))
    lr = lr_t(h, o)
    w = step64(p, g, m, v, vmax, h, o, coef)
    if o.kind == "sgd":
        G = np.abs(g * c) + np.abs(h.wd * p)
        g1 = g * c + h.wd * p
        tol_m = 4.0 * U * (np.abs(o.mu * m) + G)
        u = g1 + o.mu * w["m"] if o.nesterov else w["m"]
        upd = np.abs(lr * u)
        tol_p = 2.0 * U * np.abs(w["p"]) + lr * (tol_m * (1.0 + o.mu) + 4.0 * U * (np.abs(g1) + np.abs(o.mu * w["m"]))) + 2.0 * U * upd
        return {"p": tol_p, "m": tol_m, "v": None, "vmax": None}
    bc1, bc2 = AR.bias_corrections(h)
    G = np.abs(g * c) + (0.0 if o.kind == "adamw" else np.abs(h.wd * p))
    A = np.abs(h.b1 * m) + (1.0 - h.b1) * G
    Bv = h.b2 * v + (1.0 - h.b2) * G * G
    tol_m = 8.0 * U * A
    tol_v = 16.0 * U * Bv + 1e-37
    d = w["vmax"] if o.amsgrad else w["v"]
    rv = np.sqrt(d)
    denom = rv / np.sqrt(bc2) + h.eps
    upd = np.abs(lr / bc1 * w["m"] / denom)
    with np.errstate(divide="ignore"):
        d_denom = np.minimum(0.5 * tol_v / rv, np.sqrt(tol_v)) / np.sqrt(bc2)
    tol_p = 2.0 * U * np.abs(w["p"]) + (lr / bc1) / denom * tol_m + upd * d_denom / denom + 16.0 * U * upd + 2.0 * U * upd
    if o.kind == "adamw":
        tol_p = tol_p + U * np.abs(p)
    return {"p": tol_p, "m": tol_m, "v": tol_v, "vmax": tol_v if o.amsgrad else None}


def step32_emulated(p, g, m, v, vmax, h, o, coef):
    """The kernels' arithmetic in numpy float32, one operation at a time (no fused multiply-add); lr_t and the two bias-correction
    factors are computed in float64 and cast, as the kernel prologue does.  Same keys as step64, float32."""
    f = np.float32
    p, g, m = (np.asarray(a, dtype=np.float32) for a in (p, g, m))
    lr = f(lr_t(h, o))
    wd, c = f(h.wd), f(coef)
    with np.errstate(under="ignore", invalid="ignore"):
        if o.kind == "sgd":
            mu = f(o.mu)
            g1 = g * c + wd * p
            m1 = mu * m + g1
            u = g1 + mu * m1 if o.nesterov else m1
            out = {"p": p - lr * u, "m": m1, "v": None, "vmax": None}
        else:
            v = np.asarray(v, dtype=np.float32)
            bc1, bc2 = AR.bias_corrections(h)
            lr_over_bc1 = f(float(lr) / bc1)
            inv_sqrt_bc2 = f(1.0 / np.sqrt(bc2))
            b1, b2, eps = f(h.b1), f(h.b2), f(h.eps)
            if o.kind == "adamw":
                g1 = g * c
                p = p - (lr * wd) * p                   # (p (1 - lr_t wd) as the kernel evaluates it: one rounding at p's size)
            else:
                g1 = g * c + wd * p
            m1 = b1 * m + (f(1) - b1) * g1
            v1 = b2 * v + (f(1) - b2) * g1 * g1
            d, x1 = v1, None
            if o.amsgrad:
                x = np.asarray(vmax, dtype=np.float32)
                x1 = np.where((v1 > x) | np.isnan(v1), v1, x)
                d = x1
            denom = np.sqrt(d) * inv_sqrt_bc2 + eps
            out = {"p": p - lr_over_bc1 * (m1 / denom), "m": m1, "v": v1, "vmax": x1}
    assert all(a is None or a.dtype == np.float32 for a in out.values())
    return out


KEYS = ("p", "m", "v", "vmax")


def worst_ratios(got, want, tol):
    """{key: max |got - want| / tol} over the keys the kind keeps (adam_ref.worst_ratios: non-finite = inf, error under a zero bound = inf)."""
    ks = [k for k in KEYS if want[k] is not None]
    r = AR.worst_ratios([got[k] for k in ks], [want[k] for k in ks], [tol[k] for k in ks])
    return dict(zip(ks, r))


def planted_vmax(v, seed):
    """AMSGrad's running maximum for a planted v: v times a factor in [0.25, 4) - above the new v' at some elements, below it at others;
    zero wherever v is (a first step)."""
    rng = np.random.default_rng(seed)
    v = np.asarray(v, dtype=np.float32)
    return (v.astype(np.float64) * 4.0 ** rng.uniform(-1.0, 1.0, v.shape)).astype(np.float32)
