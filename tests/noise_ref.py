"""numpy restatement of the input-noise definition (include/codae_hip.h, "Input noise"), written from the definition
for the tests: it shares no code with codae.tool.noise or the kernels.

  words     Philox4x32-10, key = (seed & 0xffffffff, seed >> 32), counter = (column // 4, dataset row, step, 0); output
            word k of group g belongs to column 4 g + k
  MASKING   x <- 0 iff r < T, T = floor(p 2^32)
  SALT_PEPPER  r < T: x <- lo if r < T // 2 else hi
  GAUSSIAN  x <- x + sigma n; pairs (r0, r1), (r2, r3): u1 = ((ra >> 8) + 1) 2^-24, u2 = (rb >> 8) 2^-24,
            n_a = sqrt(-2 ln u1) cos(2 pi u2), n_b = sqrt(-2 ln u1) sin(2 pi u2)
  then the slot mask: keep == 0 -> exactly 0.
sigma, p, lo, hi are the fp32 values the C struct codae_noise carries; everything else is float64 / exact integers.
"""
import numpy as np

MUL_A, MUL_B = 0xD2511F53, 0xCD9E8D57
WEYL_A, WEYL_B = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def _mulhilo(m, x):
    """(high, low) 32-bit halves of m * x, x a uint64 array holding 32-bit values."""
    prod = np.uint64(m) * x
    return prod >> np.uint64(32), prod & np.uint64(MASK32)


def philox(counter, key):
    """counter: 4 broadcastable arrays / ints of 32-bit values, key: 2 ints -> list of 4 uint32 arrays."""
    x0, x1, x2, x3 = [np.array(v, dtype=np.uint64) for v in np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) for c in counter])]
    ka, kb = key[0] & MASK32, key[1] & MASK32
    for rnd in range(10):
        if rnd:
            ka, kb = (ka + WEYL_A) & MASK32, (kb + WEYL_B) & MASK32
        hi_a, lo_a = _mulhilo(MUL_A, x0)
        hi_b, lo_b = _mulhilo(MUL_B, x2)
        x0, x1, x2, x3 = hi_b ^ x1 ^ np.uint64(ka), lo_b, hi_a ^ x3 ^ np.uint64(kb), lo_a
    return [v.astype(np.uint32) for v in (x0, x1, x2, x3)]


def words(rows, io, step, seed):
    """uint32 [len(rows), io]"""
    rows = np.asarray(rows, dtype=np.uint64)
    out = np.empty((len(rows), io), dtype=np.uint32)
    n_groups = -(-io // 4)
    g = np.arange(n_groups, dtype=np.uint64)[None, :]
    r = philox((g, rows[:, None], step, 0), (seed & MASK32, seed >> 32))
    for k in range(4):
        cols = np.arange(k, io, 4)
        out[:, cols] = r[k][:, :len(cols)]
    return out


def unit_normals(rows, io, step, seed):
    """float64 [B, io]: generated at the padded width so that an odd io's last element still has its partner word."""
    io_pad = io + (io & 1)
    w = words(rows, io_pad, step, seed)
    u1 = ((w[:, 0::2] >> np.uint32(8)).astype(np.float64) + 1.0) / 16777216.0
    u2 = (w[:, 1::2] >> np.uint32(8)).astype(np.float64) / 16777216.0
    rho = np.sqrt(-2.0 * np.log(u1))
    n = np.empty((len(w), io_pad), dtype=np.float64)
    n[:, 0::2] = rho * np.cos(2.0 * np.pi * u2)
    n[:, 1::2] = rho * np.sin(2.0 * np.pi * u2)
    return n[:, :io]


def threshold(p):
    return int(np.floor(np.float64(np.float32(p)) * 4294967296.0))


def corrupt(x, rows, step, kind, seed=0, sigma=None, p=None, lo=None, hi=None, keep=None):
    """x float32 [B, io], rows [B] dataset rows, keep [B, io] (0 = blanked) or None.
    masking / salt_pepper: float32 result (exact).  gaussian: (float64 result, float64 tolerance scale |x| + sigma |n|)."""
    x = np.asarray(x, dtype=np.float32)
    B, io = x.shape
    if kind == "gaussian":
        s = np.float64(np.float32(sigma))
        n = unit_normals(rows, io, step, seed)
        out = x.astype(np.float64) + s * n
        mag = np.abs(x.astype(np.float64)) + s * np.abs(n)
        if keep is not None:
            out = np.where(np.asarray(keep) != 0, out, 0.0)
        return out, mag
    w = words(rows, io, step, seed).astype(np.uint64)
    T = threshold(p)
    if kind == "masking":
        out = np.where(w < np.uint64(T), np.float32(0), x)
    elif kind == "salt_pepper":
        out = np.where(w < np.uint64(T), np.where(w < np.uint64(T // 2), np.float32(lo), np.float32(hi)), x)
    else:
        raise ValueError(kind)
    if keep is not None:
        out = np.where(np.asarray(keep) != 0, out, np.float32(0))
    return out.astype(np.float32)


def ulp32(a):
    """fp32 unit in the last place at magnitude a (float64 array)."""
    return np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)


def gaussian_tol(mag, sigma, bf16_ref=None):
    """sigma 1e-5 (the device's unit normal is within 1e-5 of the formulas) + 2 fp32 ulps of |x| + sigma |n|; a bf16 output
    adds one bf16 ulp of the reference value, 2^-8 |c_ref|."""
    t = np.float64(np.float32(sigma)) * 1e-5 + 2.0 * ulp32(mag)
    if bf16_ref is not None:
        t = t + np.abs(bf16_ref) * 2.0 ** -8
    return t
