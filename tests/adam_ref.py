"""float64 numpy restatement of the optimizer update (clip_grad_norm_ + torch.optim.Adam, amsgrad off, L2 decay), with the
rounding-error bounds an fp32 evaluation of it must stay inside, written from the definition for the tests: it shares no code
with the kernels or the oracle.

  coef = min(1, max_norm / (sqrt(sum g^2) + 1e-6)), 1 when max_norm <= 0           (clip_coef32: the kernel's three fp32 operations)
  g' = g coef + wd p
  m' = b1 m + (1 - b1) g'
  v' = b2 v + (1 - b2) g'^2
  p' = p - lr / (1 - b1^t) m' / (sqrt(v') / sqrt(1 - b2^t) + eps)                  (adam_step64)

lr, wd, b1, b2, eps are the fp32 values the codae_hyper struct holds, widened to float64 (Hyper): 1 - float32(0.999) differs from
1e-3 by 1.3e-5 relative, far more than any bound below.

bounds(): per-element tolerances from operation counts, u = 2^-24 (half an fp32 ulp, relative).  With
  G = |g coef| + |wd p|,  A = |b1 m| + (1 - b1) G,  Bv = b2 v + (1 - b2) G^2
    m: 8 u A
    v: 16 u Bv + 1e-37                                (the constant: results below the smallest normal fp32 number)
    p: 2 u |p'| + (lr / bc1) / denom (8 u A) + |upd| d_denom / denom + 16 u |upd|
       upd = lr / bc1 m' / denom, denom = sqrt(v') / sqrt(bc2) + eps, d_denom = min(tol_v / (2 sqrt(v')), sqrt(tol_v)) / sqrt(bc2)
They are relative to the sums of magnitudes, not to the results: g coef and wd p can cancel, and so can b1 m and the new gradient.
Every fp32 operation of the update is counted once with u (a fused multiply-add rounds once instead of twice: less), the fp32
rounding of 1 - b1, 1 - b2, lr / bc1 and 1 / sqrt(bc2) likewise; the constants 8 and 16 leave about a factor two on top.  They
are measured against adam_step32_emulated (tests/test_adam_host.py asserts the worst |error| / bound <= 0.75), never against a
GPU run.

planted_state(): the state both test files update - magnitudes over thirteen decades, exact zeros, gradients the decay nearly
cancels, moments that the new gradient nearly cancels.
"""
import collections

import numpy as np

U = 2.0 ** -24

# the fp32 values of codae_hyper, widened; t = the step count (>= 1)
Hyper = collections.namedtuple("Hyper", "lr wd b1 b2 eps t")


def _w(x):
    return float(np.float32(x))


def hyper(lr, wd, betas=(0.9, 0.999), eps=1e-8, t=1):
    return Hyper(_w(lr), _w(wd), _w(betas[0]), _w(betas[1]), _w(eps), int(t))


def hyper_of_struct(hp):
    """From a codae.hip.Hyper (its c_float fields read back as the widened fp32 values)."""
    return Hyper(float(hp.lr), float(hp.weight_decay), float(hp.beta1), float(hp.beta2), float(hp.eps), int(hp.step))


def _f64(a):
    """Widened, never rounded: the callers hand over the fp32 arrays the update reads (or float64 state to carry on from)."""
    return np.asarray(a).astype(np.float64)


def bias_corrections(h):
    """(1 - b1^t, 1 - b2^t) in float64."""
    return 1.0 - h.b1 ** float(h.t), 1.0 - h.b2 ** float(h.t)


def clip_coef32(grad_sq, max_norm):
    """The kernel's coefficient from the float64 sum g^2: sqrt(float32(grad_sq)), max_norm / (total + 1e-6), clamped to 1 - three
    correctly rounded fp32 operations on both sides, so the same bits.  float32."""
    if not max_norm > 0:
        return np.float32(1.0)
    with np.errstate(all="ignore"):
        total = np.sqrt(np.float32(grad_sq))
        r = np.float32(max_norm) / np.float32(total + np.float32(1e-6))
    return np.float32(1.0) if r > np.float32(1.0) else np.float32(r)


def adam_step64(p, g, m, v, h, coef):
    """(p', m', v') in float64 from the inputs as given (fp32 arrays: what the kernel read, widened)."""
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    c = float(np.float32(coef))
    bc1, bc2 = bias_corrections(h)
    g1 = g * c + h.wd * p
    m1 = h.b1 * m + (1.0 - h.b1) * g1
    v1 = h.b2 * v + (1.0 - h.b2) * g1 * g1
    p1 = p - h.lr / bc1 * m1 / (np.sqrt(v1) / np.sqrt(bc2) + h.eps)
    return p1, m1, v1


def bounds(p, g, m, v, h, coef):
    """(tol_p, tol_m, tol_v): what |fp32 result - adam_step64| may reach, per element (module docstring)."""
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    c = float(np.float32(coef))
    bc1, bc2 = bias_corrections(h)
    p1, m1, v1 = adam_step64(p, g, m, v, h, coef)
    G = np.abs(g * c) + np.abs(h.wd * p)
    A = np.abs(h.b1 * m) + (1.0 - h.b1) * G
    Bv = h.b2 * v + (1.0 - h.b2) * G * G
    tol_m = 8.0 * U * A
    tol_v = 16.0 * U * Bv + 1e-37
    rv = np.sqrt(v1)
    denom = rv / np.sqrt(bc2) + h.eps
    upd = np.abs(h.lr / bc1 * m1 / denom)
    with np.errstate(divide="ignore"):
        d_denom = np.minimum(0.5 * tol_v / rv, np.sqrt(tol_v)) / np.sqrt(bc2)
    tol_p = 2.0 * U * np.abs(p1) + (h.lr / bc1) / denom * tol_m + upd * d_denom / denom + 16.0 * U * upd
    return tol_p, tol_m, tol_v


def adam_step32_emulated(p, g, m, v, h, coef):
    """The kernel's arithmetic in numpy float32, one operation at a time (no fused multiply-add); the two bias-correction
    factors are computed in float64 and cast, as the launcher does.  (p', m', v') float32."""
    f = np.float32
    p, g, m, v = (np.asarray(a, dtype=np.float32) for a in (p, g, m, v))
    bc1, bc2 = bias_corrections(h)
    lr_over_bc1 = f(h.lr / bc1)
    inv_sqrt_bc2 = f(1.0 / np.sqrt(bc2))
    b1, b2, eps, wd, c = f(h.b1), f(h.b2), f(h.eps), f(h.wd), f(coef)
    with np.errstate(under="ignore"):
        g1 = g * c + wd * p
        m1 = b1 * m + (f(1) - b1) * g1
        v1 = b2 * v + (f(1) - b2) * g1 * g1
        denom = np.sqrt(v1) * inv_sqrt_bc2 + eps
        p1 = p - lr_over_bc1 * (m1 / denom)
    assert p1.dtype == m1.dtype == v1.dtype == np.float32
    return p1, m1, v1


def worst_ratios(got, want, tol):
    """max |got - want| / tol per (p, m, v); a non-finite value counts as inf, and so does any error where the bound is 0 (m where
    gradient, decay and old moment are all zero: the result is exactly 0)."""
    out = []
    for a, b, t in zip(got, want, tol):
        a = np.asarray(a, dtype=np.float64)
        if a.size == 0:
            out.append(0.0)
            continue
        e = np.abs(a - b)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(e == 0, 0.0, e / t)
        out.append(float("inf") if not np.isfinite(a).all() else float(r.max()))
    return tuple(out)


def _magnitudes(rng, n, k_lo, k_hi):
    """10^k, k an integer drawn from k_lo..k_hi, times a mantissa factor in [1, 2)."""
    return 10.0 ** rng.integers(k_lo, k_hi + 1, n) * (1.0 + rng.random(n))


def planted_state(shape_list, seed, first_step, wd=0.0):
    """One dict per shape with float32 arrays p, g, m, v of that shape.
    g: magnitudes 10^k, k in -9..4, random sign; where wd > 0 every 11th element (of the tensor, flattened) is
       -wd p (1 + 1e-3 n), n = 0..7 in turn, so that the decay nearly (n = 0: all but) cancels it; every 7th element exactly 0.
    p: 10^k, k in -4..2, random sign.
    m: the magnitude of the element's gradient (before the zeros and the planted cancellations) times a factor in [0.5, 2),
       random sign; v = (such a value)^2 with a factor of its own; both zero when first_step."""
    rng = np.random.default_rng(seed)
    wd = _w(wd)
    out = []
    for shape in shape_list:
        n = int(np.prod(shape))
        sign = lambda: np.where(rng.random(n) < 0.5, -1.0, 1.0)
        p = (_magnitudes(rng, n, -4, 2) * sign()).astype(np.float32)
        mag = _magnitudes(rng, n, -9, 4)
        g = mag * sign()
        if wd > 0:
            i = np.arange(0, n, 11)
            g[i] = -wd * p[i].astype(np.float64) * (1.0 + 1e-3 * (np.arange(i.size) % 8))
        g[::7] = 0.0
        if first_step:
            m, v = np.zeros(n), np.zeros(n)
        else:
            m = mag * (0.5 + 1.5 * rng.random(n)) * sign()
            v = (mag * (0.5 + 1.5 * rng.random(n))) ** 2
        out.append({k: a.astype(np.float32).reshape(shape) for k, a in (("p", p), ("g", g), ("m", m), ("v", v))})
    return out
