"""float64 numpy restatement of the layer-wise trust-ratio kinds of include/codae_hip.h ("Layer-wise trust ratios": LAMB and LARS),
an fp32 one-operation-at-a-time emulation of the order the header fixes, and the rounding-error bounds an fp32 evaluation must stay
inside - written from the definition for the tests: no code shared with the kernels or with codae.tool.optimizer.  Hyper, the
schedule (lr_t) and U are adam_ref's / optim_ref's.

One tensor at a time: a MATRIX (its own ratio) or a BIAS (matrix=False: ratio 1, wd' = decay_bias ? wd : 0).
  lamb  g' = g coef;  m' = b1 m + (1 - b1) g';  v' = b2 v + (1 - b2) g'^2;  r = (m' / bc1) / (sqrt(v') / sqrt(bc2) + eps)
        u = r + wd' p;  phi = P > 0 and U > 0 ? P / U : 1, min(phi, trust_clip) when trust_clip > 0;  p' = p - lr_t phi u
  lars  g' = g coef;  lambda = P > 0 and G > 0 ? trust_coef P / (G + wd P + eps) : 1, clipped alike
        d = lambda (g' + wd' p);  m' = mu m + d;  u = nesterov ? d + mu m' : m';  p' = p - lr_t u;  v untouched            (step64)
  P = ||p||, U = ||u||, G = ||g'|| over the tensor.  A comparison with a NaN norm is false: the ratio is 1.

bounds(), u = 2^-24, TINY = the smallest normal fp32 number:
  elements (lamb), with G = |g coef|, A = |b1 m| + (1 - b1) G, Bv = b2 v + (1 - b2) G^2 as in adam_ref / optim_ref's adamw:
    tol_m = 8 u A;  tol_v = 16 u Bv + SUBNORMAL (= 8 TINY: results below the smallest normal number)
    tol_r = tol_m / (bc1 denom) + |r| d_denom / denom + 16 u |r|        (optim_ref's p terms of adamw, without the factor lr_t)
    tol_u = tol_r + 4 u (|r| + |wd' p|)                                 (the product, the sum, relative to the sum of magnitudes)
  norms: the squares are fp32 (one rounding each: the norm moves by u ||x|| at most; a square that underflows loses at most TINY:
    sqrt(n TINY) on the norm, as |sqrt a - sqrt b| <= sqrt|a - b|), the sums double:
    dP = 2 u P + sqrt(n TINY);   dX = ||tol_x|| + 2 u X + sqrt(n TINY)   for X = U (tol_u) or G (tol_g' = u |g coef|)
    (| ||x + delta|| - ||x|| | <= ||delta||)
  ratio: lamb  tol_phi = phi (dP / P + dU / U) / (1 - dU / U) + 4 u phi                (quotient in double, the cast to fp32)
         lars  tol_lam = lam (dP / P + (dG + wd dP) / (G + wd P + eps)) / (1 - (dG + wd dP) / (G + wd P + eps)) + 4 u lam
         0 where the definition gives exactly 1 (a zero norm, a bias); unchanged under trust_clip (a minimum moves by no more)
  p' (lamb): 2 u |p'| + lr_t phi tol_u + lr_t |u| tol_phi + 8 u |upd|,  upd = lr_t phi u
             (lr_t's own rounding, lr_t phi, the product, the subtraction)
  lars: tol_d = |g' + wd' p| tol_lam + 4 u lam (|g'| + |wd' p|);  tol_m = tol_d + 4 u (|mu m| + |d|)
        tol_u = nesterov ? tol_d + mu tol_m + 4 u (|d| + |mu m'|) : tol_m
        p': 2 u |p'| + lr_t tol_u + 6 u |upd|,  upd = lr_t u
They are measured against step32_emulated (tests/test_trust_host.py asserts the worst |error| / bound <= 0.75), never against a GPU
run.
"""
import collections

import numpy as np

import adam_ref as AR
import optim_ref as OR
from adam_ref import U

TINY = float(np.finfo(np.float32).tiny)
SUBNORMAL = 8.0 * TINY          # a v' below the smallest normal fp32 number loses its low bits: absolute, not relative (8 TINY = 9.4e-38)

# kind: "lamb" | "lars"; mu, trust_coef, trust_clip: fp32 values, widened; sched: an optim_ref.Opt that carries the schedule
Trust = collections.namedtuple("Trust", "kind mu nesterov trust_coef trust_clip decay_bias sched")


def trust(kind, momentum=0.0, nesterov=False, trust_coef=1e-3, trust_clip=0.0, decay_bias=False, **sched):
    assert kind in ("lamb", "lars"), kind
    w = AR._w
    return Trust(kind, w(momentum), bool(nesterov), w(trust_coef), w(trust_clip), bool(decay_bias), OR.opt("sgd", **sched))


def trust_of(o):
    """From a codae.tool.Optimizer."""
    s = o.schedule
    return trust(o.kind, o.momentum, o.nesterov, o.trust_coef, o.trust_clip, o.decay_bias, sched=s.kind, warmup=s.warmup,
                 total=s.total or 0, period=s.period, min_factor=s.min_factor, gamma=s.gamma)


def lr_t(h, tr):
    return OR.lr_t(h, tr.sched)


def _f64(a):
    return None if a is None else np.asarray(a).astype(np.float64).reshape(-1)


def _norm(x):
    with np.errstate(all="ignore"):
        return float(np.sqrt((x * x).sum()))


def _ratio(tr, h, P, D):
    r = 1.0
    if P > 0.0 and D > 0.0:
        r = P / D if tr.kind == "lamb" else tr.trust_coef * P / (D + h.wd * P + h.eps)
    if tr.trust_clip > 0.0 and r > tr.trust_clip:
        r = tr.trust_clip
    return r


def _lamb_dir64(p, g, m, v, h, c, wd1):
    bc1, bc2 = AR.bias_corrections(h)
    g1 = g * c
    m1 = h.b1 * m + (1.0 - h.b1) * g1
    v1 = h.b2 * v + (1.0 - h.b2) * g1 * g1
    with np.errstate(invalid="ignore"):
        denom = np.sqrt(v1) / np.sqrt(bc2) + h.eps
    r = (m1 / bc1) / denom
    return g1, m1, v1, denom, r, r + wd1 * p


def step64(p, g, m, v, h, tr, coef, matrix=True, ratio=None):
    """{"p", "m", "v", "ratio"} in float64 from the inputs as given (flattened; v None under lars).  ratio: use this one instead of the
    tensor's own (the ratio a device run read back, to tell an element's error from the ratio's)."""
    p, g, m, v = (_f64(a) for a in (p, g, m, v))
    c = float(np.float32(coef))
    lr = lr_t(h, tr)
    wd1 = h.wd if matrix or tr.decay_bias else 0.0
    if tr.kind == "lamb":
        g1, m1, v1, _, _, u = _lamb_dir64(p, g, m, v, h, c, wd1)
        phi = (_ratio(tr, h, _norm(p), _norm(u)) if matrix else 1.0) if ratio is None else float(ratio)
        return {"p": p - lr * phi * u, "m": m1, "v": v1, "ratio": phi}
    g1 = g * c
    lam = (_ratio(tr, h, _norm(p), _norm(g1)) if matrix else 1.0) if ratio is None else float(ratio)
    d = lam * (g1 + wd1 * p)
    m1 = tr.mu * m + d
    u = d + tr.mu * m1 if tr.nesterov else m1
    return {"p": p - lr * u, "m": m1, "v": None, "ratio": lam}


def bounds(p, g, m, v, h, tr, coef, matrix=True):
    """{"p", "m", "v", "ratio"}: what |fp32 result - step64| may reach (module docstring); "ratio" a scalar."""
    p, g, m, v = (_f64(a) for a in (p, g, m, v))
    c = float(np.float32(coef))
    lr = lr_t(h, tr)
    wd1 = h.wd if matrix or tr.decay_bias else 0.0
    n = p.size
    under = np.sqrt(n * TINY)
    P = _norm(p)
    dP = 2.0 * U * P + under
    w = step64(p, g, m, v, h, tr, coef, matrix)
    G = np.abs(g * c)
    if tr.kind == "lamb":
        bc1, bc2 = AR.bias_corrections(h)
        g1, m1, v1, denom, r, u = _lamb_dir64(p, g, m, v, h, c, wd1)
        A = np.abs(h.b1 * m) + (1.0 - h.b1) * G
        Bv = h.b2 * v + (1.0 - h.b2) * G * G
        tol_m = 8.0 * U * A
        tol_v = 16.0 * U * Bv + SUBNORMAL
        rv = np.sqrt(v1)
        with np.errstate(divide="ignore", invalid="ignore"):
            d_denom = np.minimum(0.5 * tol_v / rv, np.sqrt(tol_v)) / np.sqrt(bc2)
        tol_r = tol_m / (bc1 * denom) + np.abs(r) * d_denom / denom + 16.0 * U * np.abs(r)
        tol_u = tol_r + 4.0 * U * (np.abs(r) + np.abs(wd1 * p))
        phi, tol_phi = w["ratio"], 0.0
        Un = _norm(u)
        if matrix and P > 0.0 and Un > 0.0:
            dU = _norm(tol_u) + 2.0 * U * Un + under
            rel = dU / Un
            tol_phi = phi * (dP / P + rel) / (1.0 - rel) + 4.0 * U * phi if rel < 1.0 else float("inf")
        upd = np.abs(lr * phi * u)
        tol_p = 2.0 * U * np.abs(w["p"]) + lr * phi * tol_u + lr * np.abs(u) * tol_phi + 8.0 * U * upd
        return {"p": tol_p, "m": tol_m, "v": tol_v, "ratio": tol_phi}
    g1 = g * c
    lam, tol_lam = w["ratio"], 0.0
    Gn = _norm(g1)
    if matrix and P > 0.0 and Gn > 0.0:
        dG = _norm(U * G) + 2.0 * U * Gn + under
        den = Gn + h.wd * P + h.eps
        rel = (dG + h.wd * dP) / den
        tol_lam = lam * (dP / P + rel) / (1.0 - rel) + 4.0 * U * lam if rel < 1.0 else float("inf")
    s = g1 + wd1 * p
    mag = G + np.abs(wd1 * p)
    d = lam * s
    tol_d = np.abs(s) * tol_lam + 4.0 * U * lam * mag
    tol_m = tol_d + 4.0 * U * (np.abs(tr.mu * m) + np.abs(d))
    if tr.nesterov:
        tol_u = tol_d + tr.mu * tol_m + 4.0 * U * (np.abs(d) + np.abs(tr.mu * w["m"]))
        u = d + tr.mu * w["m"]
    else:
        tol_u, u = tol_m, w["m"]
    upd = np.abs(lr * u)
    tol_p = 2.0 * U * np.abs(w["p"]) + lr * tol_u + 6.0 * U * upd
    return {"p": tol_p, "m": tol_m, "v": None, "ratio": tol_lam}


def step32_emulated(p, g, m, v, h, tr, coef, matrix=True):
    """The header's fp32 order in numpy float32, one operation at a time (no fused multiply-add): squares in fp32, their sums and the
    ratio in float64, the ratio cast to fp32.  Same keys as step64; arrays float32, "ratio" a float32."""
    f = np.float32
    p, g, m = (np.asarray(a, dtype=np.float32).reshape(-1) for a in (p, g, m))
    lr, c = f(lr_t(h, tr)), f(coef)
    wd1 = f(h.wd if matrix or tr.decay_bias else 0.0)

    def norm(x):
        return float(np.sqrt((x * x).astype(np.float64).sum()))
    with np.errstate(under="ignore", invalid="ignore", over="ignore"):
        g1 = g * c
        if tr.kind == "lamb":
            v = np.asarray(v, dtype=np.float32).reshape(-1)
            bc1, bc2 = AR.bias_corrections(h)
            inv_bc1, inv_sqrt_bc2 = f(1.0 / bc1), f(1.0 / np.sqrt(bc2))
            b1, b2, eps = f(h.b1), f(h.b2), f(h.eps)
            m1 = b1 * m + (f(1) - b1) * g1
            v1 = b2 * v + ((f(1) - b2) * g1) * g1
            denom = np.sqrt(v1) * inv_sqrt_bc2 + eps
            u = (m1 / denom) * inv_bc1 + wd1 * p
            phi = f(_ratio(tr, h, norm(p), norm(u)) if matrix else 1.0)
            out = {"p": p - (lr * phi) * u, "m": m1, "v": v1, "ratio": phi}
        else:
            lam = f(_ratio(tr, h, norm(p), norm(g1)) if matrix else 1.0)
            mu = f(tr.mu)
            d = lam * (g1 + wd1 * p)
            m1 = mu * m + d
            u = d + mu * m1 if tr.nesterov else m1
            out = {"p": p - lr * u, "m": m1, "v": None, "ratio": lam}
    assert all(a is None or a.dtype == np.float32 for a in out.values())
    return out


KEYS = ("p", "m", "v")


def worst_ratios(got, want, tol):
    """{key: max |got - want| / tol} over p, m, the v the kind keeps, and "ratio" (adam_ref.worst_ratios: a non-finite value = inf, an
    error under a zero bound = inf)."""
    ks = [k for k in KEYS if want[k] is not None]
    r = AR.worst_ratios([got[k] for k in ks], [want[k] for k in ks], [tol[k] for k in ks])
    out = dict(zip(ks, r))
    out["ratio"] = AR.worst_ratios([np.array([got["ratio"]])], [np.array([want["ratio"]])], [np.array([tol["ratio"]])])[0]
    return out
