"""Per-pair numpy float64 reference of "Assembled outfits and compatibility" (include/codae_hip.h), written from the definitions with
plain loops - nothing of codae.tool is used.  Shared by tests/test_compat_host.py and tests/test_gpu_compat.py."""
import numpy as np

COS_EPS = 1e-8
WINS, TIES, PAIRS, PAIRED, STRIDE = 0, 1, 2, 3, 4


def present(items, q, s, n_rows, presence):
    r = int(items[q][s])
    return 0 <= r < n_rows and (presence is None or presence[r][s] != 0)


def assemble(src, items, S, blank=None, leave_one_out=False, presence=None):
    """src [N, io] of any dtype -> [Q (S)] rows of the same dtype: a copy, +0 where absent or blanked."""
    N, io = src.shape
    E = io // S
    Q = len(items)
    rows = Q * S if leave_one_out else Q
    out = np.zeros((rows, io), dtype=src.dtype)
    for row in range(rows):
        q, v = (row // S, row % S) if leave_one_out else (row, -1 if blank is None else int(blank[row]))
        for s in range(S):
            if s != v and present(items, q, s, N, presence):
                out[row, s * E:(s + 1) * E] = src[int(items[q][s]), s * E:(s + 1) * E]
    return out


def slot_scores(data, items, Y, S, presence=None):
    """float64 cos [Q, S], sq [Q, S], score [Q] (NaN with fewer than two present slots), n_present [Q] from Y [Q S, io]."""
    N, io = data.shape
    E = io // S
    Q = len(items)
    cos, sq = np.zeros((Q, S)), np.zeros((Q, S))
    score, n_present = np.full(Q, np.nan), np.zeros(Q, dtype=np.int64)
    for q in range(Q):
        acc, n = 0.0, 0
        for s in range(S):
            if not present(items, q, s, N, presence):
                continue
            x = data[int(items[q][s]), s * E:(s + 1) * E].astype(np.float64)
            y = Y[q * S + s, s * E:(s + 1) * E].astype(np.float64)
            nx, ny = np.sqrt((x * x).sum()), np.sqrt((y * y).sum())
            nx = COS_EPS if nx < COS_EPS else nx            # (a NaN norm stays NaN)
            ny = COS_EPS if ny < COS_EPS else ny
            cos[q, s] = (x * y).sum() / (nx * ny)
            sq[q, s] = ((x - y) ** 2).sum()
            acc += cos[q, s]
            n += 1
        n_present[q] = n
        if n >= 2:
            score[q] = acc / n
    return cos, sq, score, n_present


def auc_counts(pos, neg, neg_slot, S, neg_parent=None, pos_on=None):
    """int64 [S + 1, 4]: per swapped slot wins, ties, pairs, paired wins; row S = live positives, live negatives."""
    P, M = len(pos), len(neg)
    live_p = [pos_on is None or pos_on[i] != 0 for i in range(P)]
    c = np.zeros((S + 1, STRIDE), dtype=np.int64)
    n_pos = sum(live_p)
    for j in range(M):
        s = int(neg_slot[j])
        if not 0 <= s < S:
            continue
        if neg_parent is not None and pos_on is not None:
            par = int(neg_parent[j])
            if not (0 <= par < P and live_p[par]):
                continue
        c[S, 1] += 1
        c[s, PAIRS] += n_pos
        for i in range(P):
            if not live_p[i]:
                continue
            if pos[i] > neg[j]:
                c[s, WINS] += 1
            elif pos[i] == neg[j]:
                c[s, TIES] += 1
        if neg_parent is not None:
            par = int(neg_parent[j])
            if 0 <= par < P and live_p[par] and pos[par] > neg[j]:
                c[s, PAIRED] += 1
    c[S, 0] = n_pos
    return c


def auc_counts_fast(pos, neg, neg_slot, S, neg_parent=None, pos_on=None):
    """auc_counts with the comparisons as numpy array operations (the sizes the loops cannot do in a test's time);
    tests/test_compat_host.py holds it to the loops."""
    P = len(pos)
    live_p = np.ones(P, dtype=bool) if pos_on is None else np.asarray(pos_on) != 0
    sl = np.asarray(neg_slot).astype(np.int64)
    live_n = (sl >= 0) & (sl < S)
    if neg_parent is not None:
        par = np.asarray(neg_parent).astype(np.int64)
        par_ok = (par >= 0) & (par < P)
        par_live = par_ok & live_p[np.clip(par, 0, P - 1)]
        if pos_on is not None:
            live_n &= par_live
    c = np.zeros((S + 1, STRIDE), dtype=np.int64)
    p = np.asarray(pos)[live_p]
    with np.errstate(invalid="ignore"):
        for s in range(S):
            j = np.nonzero(live_n & (sl == s))[0]
            v = np.asarray(neg)[j]
            c[s, WINS] = int((p[:, None] > v[None, :]).sum())
            c[s, TIES] = int((p[:, None] == v[None, :]).sum())
            c[s, PAIRS] = len(p) * len(j)
            if neg_parent is not None:
                c[s, PAIRED] = int((par_live[j] & (np.asarray(pos)[np.clip(par[j], 0, P - 1)] > v)).sum())
    c[S, 0], c[S, 1] = len(p), int(live_n.sum())
    return c


def auc_of(c):
    """(auc, paired accuracy) in total from a counts block; NaN where there is no pair."""
    S = c.shape[0] - 1
    w, t, p, pw = (int(c[:S, f].sum()) for f in (WINS, TIES, PAIRS, PAIRED))
    return ((w + 0.5 * t) / p if p else float("nan")), (pw / int(c[S, 1]) if c[S, 1] else float("nan"))


def tricky_scores(P, M, S, seed, empty_slot=None):
    """fp32 score vectors with duplicates across the two sides, +-inf and NaN on both, slots in [0, S) except `empty_slot`."""
    rng = np.random.default_rng(seed)
    grid = np.linspace(-1, 1, 17).astype(np.float32)
    pos, neg = rng.choice(grid, P).astype(np.float32), rng.choice(grid, M).astype(np.float32)
    for v, special in ((pos, (np.inf, -np.inf, np.nan)), (neg, (np.nan, np.inf, -np.inf))):
        if len(v) >= 8:
            v[rng.choice(len(v), 3, replace=False)] = special
    slots = [s for s in range(S) if s != empty_slot]
    neg_slot = rng.choice(slots, M).astype(np.int32)
    neg_parent = rng.integers(0, P, M).astype(np.int32)
    return pos, neg, neg_slot, neg_parent


class Dataset:
    """data [N, S * E] in the shape ComplementRetriever / CompatibilityMetrics read."""

    def __init__(self, data, S):
        import torch
        self.nb_used_category, self.embedding_size = S, data.shape[1] // S
        t = torch.as_tensor(np.ascontiguousarray(data))
        self.data_per_category = {c: t[:, c * self.embedding_size:(c + 1) * self.embedding_size] for c in range(S)}


def orthogonal_design(seed=0, N=64, E=16):
    """S = 2: data[:, slot 1] = P data[:, slot 0] for a fixed orthogonal P, and the two-Linear stack W1 = [[0, P^T], [P, 0]], W2 = I
    without activation or bias, which reconstructs a blanked slot exactly from the other one.  float64 arrays; the tests cast."""
    rng = np.random.default_rng(seed)
    Pm, _ = np.linalg.qr(rng.standard_normal((E, E)))
    x0 = rng.standard_normal((N, E))
    data = np.concatenate([x0, x0 @ Pm.T], axis=1)
    W1 = np.zeros((2 * E, 2 * E))
    W1[:E, E:] = Pm.T
    W1[E:, :E] = Pm
    return {"S": 2, "E": E, "N": N, "P": Pm, "data": data, "W1": W1, "W2": np.eye(2 * E)}


def design_forward(d, X, sign=1.0):
    return (X.astype(np.float64) @ (sign * d["W1"]).T) @ d["W2"].T
