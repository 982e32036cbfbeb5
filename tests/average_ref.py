"""Float64 restatement of the weight average (include/codae_hip.h, "Weight average") fed fp32 inputs, the bound the kernels are held
to, and a numpy fp32 emulation of the two orders a compiler may evaluate it in.  Shared by tests/test_weight_average_host.py (which
fixes the bound on the CPU) and tests/test_gpu_weight_average.py.

    t < start or (t - start) % every != 0: no sample.  n = (t - start) / every;
    swa w = 1 / (n + 1);  ema w = 1 if n == 0 else 1 - (debias ? min(decay, (1 + n) / (10 + n)) : decay);  w32 = float32(w)
    a' = p' when w32 == 1, else a + w32 (p' - a)

Bound per element: |a'_got - a'_64| <= 3 u (|a| + |p'|), u = 2^-24: one rounding each for the subtraction (relative to |p' - a| <=
|a| + |p'|), the product (w32 <= 1: the same size) and the sum (|a'| <= max(|a|, |p'|)); a contracted product-and-sum has one
rounding fewer, so the bound covers it too.
"""
import numpy as np

U = 2.0 ** -24
KINDS = ("ema", "swa")


class Setting:
    """kind "ema" | "swa", decay as the fp32 value the struct carries, debias, start, every."""

    def __init__(self, kind, decay=0.999, debias=True, start=1, every=1):
        assert kind in KINDS
        self.kind, self.decay, self.debias, self.start, self.every = kind, float(np.float32(decay)), bool(debias), int(start), int(every)

    def __repr__(self):
        return "%s(decay=%.6g, debias=%d, start=%d, every=%d)" % (self.kind, self.decay, self.debias, self.start, self.every)


def setting_of(tool):
    """Setting of a codae.tool.WeightAverage."""
    return Setting(tool.kind, tool.decay, tool.debias, tool.start, tool.every)


def weight32(s, t):
    """np.float32 w32 of the 1-based step t, or None when the step does not sample."""
    if t < s.start or (t - s.start) % s.every:
        return None
    n = (t - s.start) // s.every
    if s.kind == "swa":
        w = 1.0 / float(n + 1)
    elif n == 0:
        w = 1.0
    else:
        w = 1.0 - (min(s.decay, (1.0 + n) / (10.0 + n)) if s.debias else s.decay)
    return np.float32(w)


def step64(a, p, w32):
    """a' in float64 from fp32 arrays a, p (w32 None: a itself)."""
    a64, p64 = np.asarray(a, dtype=np.float32).astype(np.float64), np.asarray(p, dtype=np.float32).astype(np.float64)
    if w32 is None:
        return a64
    if np.float32(w32) == np.float32(1):
        return p64
    return a64 + np.float64(w32) * (p64 - a64)


def bound(a, p):
    return 3.0 * U * (np.abs(np.asarray(a, dtype=np.float64)) + np.abs(np.asarray(p, dtype=np.float64)))


def emulate32(a, p, w32, order):
    """fp32 a' as the hardware forms it: order "plain" = fl(a + fl(w fl(p - a))), "fma" = fl(a + w fl(p - a)) (the product of two
    fp32 values is exact in float64; the sum is rounded there once more before it is rounded to fp32 - a double rounding a real
    fma does not have, half a float64 ulp, far inside the bound)."""
    a, p = np.asarray(a, dtype=np.float32), np.asarray(p, dtype=np.float32)
    if w32 is None:
        return a.copy()
    w = np.float32(w32)
    if w == np.float32(1):
        return p.copy()
    d = (p - a).astype(np.float32)
    if order == "plain":
        return (a + (w * d).astype(np.float32)).astype(np.float32)
    assert order == "fma"
    return (a.astype(np.float64) + np.float64(w) * d.astype(np.float64)).astype(np.float32)


def worst_ratio(got, want64, tol):
    """max |got - want| / bound over the elements (0 where both error and bound are 0; inf where only the bound is)."""
    e = np.abs(np.asarray(got, dtype=np.float64) - want64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(e == 0, 0.0, e / tol)
    return float(r.max()) if r.size else 0.0


def swa_mean_bound(snapshots):
    """6 u N max|p| per element for the equal-weight mean of N snapshots (every step's local error is at most 3 u (|a| + |p'|) <= 6 u
    max|p|, and later steps contract it)."""
    n = len(snapshots)
    return 6.0 * U * n * np.max(np.abs(np.stack([np.asarray(x, dtype=np.float64) for x in snapshots])), axis=0)


def planted(n, seed):
    """(a, p): fp32 vectors of mixed sign and magnitude, some equal elements (p - a == 0) and some zeros."""
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 2, n)).astype(np.float32)
    p = (a + rng.standard_normal(n).astype(np.float32) * np.float32(0.05) * np.abs(a)).astype(np.float32)
    p[::7] = a[::7]
    a[3::11] = 0
    return a, p
