"""Swap noise written from its definition (include/codae_hip.h, "Swap noise"), as a plain-Python loop over (row, slot): the
reference the numpy statement of codae.tool.InputNoise and the HIP kernels are compared with, bit for bit - nothing is computed on
the values, so there is no tolerance.  Shares only the host Philox with the code under test.

The draw fixture of the tests: N = 64 rows, B = 64 (rows 0 .. 63), a pool of 8 rows, a presence table with about a quarter of the
slots absent, p = 0.4 (S = 2, 3) or 0.3 (S = 11), seed 7, steps 1 and 2.  Every definition test first asserts, on this reference
alone, that all four classes of a draw occur: not hit, rejected as the row itself, rejected by presence, accepted.
"""
import math

import numpy as np

from codae.tool.noise import philox4x32_10

STREAM = 512
SEED = 7
N_ROWS = 64


def draw(row, slot, step, seed):
    """(w0, w1) of one (dataset row, slot, step)."""
    w = philox4x32_10((slot, row, step, STREAM), (seed & 0xFFFFFFFF, seed >> 32))
    return int(w[0]), int(w[1])


def classify(rows, step, S, p, seed, n_rows, pool=None, present=None):
    """Per (batch row, slot): (cls int [B, S], source int [B, S]); cls 0 not hit, 1 rejected: the source is the row itself,
    2 rejected by presence, 3 accepted."""
    T = int(math.floor(float(np.float32(p)) * 4294967296.0))
    P = n_rows if pool is None else len(pool)
    cls = np.zeros((len(rows), S), dtype=np.int64)
    src = np.zeros((len(rows), S), dtype=np.int64)
    for b, r in enumerate(rows):
        r = int(r)
        for s in range(S):
            w0, w1 = draw(r, s, step, seed)
            j = (w1 * P) >> 32
            q = j if pool is None else int(pool[j])
            src[b, s] = q
            if not w0 < T:
                cls[b, s] = 0
            elif q == r:
                cls[b, s] = 1
            elif present is not None and not (present[r][s] and present[q][s]):
                cls[b, s] = 2
            else:
                cls[b, s] = 3
    return cls, src


def corrupt(x, data, rows, step, S, p, seed, pool=None, present=None, keep=None):
    """The training input of batch x [B, io] (x[b] = the clean row of dataset row rows[b]): swapped slots from `data`, then the
    blank (keep [B, io], 0 = blanked), then the presence rule.  Returns (out fp32 [B, io], cls [B, S])."""
    B, io = x.shape
    E = io // S
    cls, src = classify(rows, step, S, p, seed, data.shape[0], pool, present)
    out = np.array(x, dtype=np.float32, copy=True)
    for b in range(B):
        for s in range(S):
            if cls[b, s] == 3:
                out[b, s * E:(s + 1) * E] = data[src[b, s], s * E:(s + 1) * E]
    if keep is not None:
        out[np.asarray(keep) == 0] = np.float32(0)
    if present is not None:
        for b, r in enumerate(rows):
            for s in range(S):
                if not present[int(r)][s]:
                    out[b, s * E:(s + 1) * E] = np.float32(0)
    return out, cls


def fixture(S, p=None):
    """The issue's draw fixture for S slots: dict(pool, present, p, rows)."""
    rng = np.random.RandomState(1)
    pool = np.sort(rng.choice(N_ROWS, 8, replace=False))
    present = rng.rand(N_ROWS, S) > 0.25
    return dict(pool=pool, present=present, p=(0.3 if S == 11 else 0.4) if p is None else p, rows=np.arange(N_ROWS), S=S)


def assert_all_classes(cls):
    """Every definition test starts here: a test that swaps nothing or everything shows nothing."""
    counts = [int((cls == k).sum()) for k in range(4)]
    assert all(c > 0 for c in counts), counts
    return counts
