"""The float64 numpy restatement of "Code clusters" (include/codae_hip.h): nearest centroid, centroid update, fit - and the planted
data the host and the GPU tests share.  For the bf16 form the operands are rounded to bf16 (nearest even) first, so that what remains
between a kernel and this file is accumulation error only."""
import numpy as np

EPS = 1e-8


def bf16_round(a):
    """fp32 values rounded to bf16, nearest even, as fp32 (NaN stays NaN)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16).astype(np.uint32)
    out = r.view(np.float32).copy()
    out[np.isnan(a)] = np.nan
    return out


def op(a, bf16):
    return bf16_round(a) if bf16 else np.asarray(a, dtype=np.float32)


def scores(x, c, bf16):
    """d [M][K] in float64 from the operands as the product sees them"""
    with np.errstate(invalid="ignore", over="ignore"):
        return op(x, bf16).astype(np.float64) @ op(c, bf16).astype(np.float64).T


def nearest(x, c, norm=None, bf16=False):
    """(assign int64 [M], best float64 [M], d float64 [M][K])"""
    d = scores(x, c, bf16)
    M, K = d.shape
    assign = np.full(M, -1, dtype=np.int64)
    best = np.full(M, np.nan)
    for r in range(M):
        ok = ~np.isnan(d[r])
        if ok.any():
            top = d[r][ok].max()
            assign[r] = int(np.flatnonzero(ok & (d[r] == top))[0])           # -0 == +0; the lowest index of equal scores
            best[r] = d[r, assign[r]]
    if norm is not None:
        best = best / np.maximum(np.asarray(norm, dtype=np.float64), EPS)
    return assign, best, d


def top_two_gap(d):
    """per row the gap between the two largest scores (inf with one centroid)"""
    if d.shape[1] < 2:
        return np.full(d.shape[0], np.inf)
    s = np.sort(d, axis=1)
    return s[:, -1] - s[:, -2]


def update(x, norm, assign, c):
    """(c' float64 [K][Z], counts int64 [K], bound float64 [K][Z]): the update in float64 from the same assign, and per element the
    fp32 accumulation bound count_j 2^-24 sum|terms| / |sum_j| (0 for an empty cluster, which keeps c)"""
    x64 = np.asarray(x, dtype=np.float64)
    n = np.maximum(np.asarray(norm, dtype=np.float64), EPS)
    K = c.shape[0]
    out = np.asarray(c, dtype=np.float64).copy()
    counts = np.zeros(K, dtype=np.int64)
    bound = np.zeros_like(out)
    for j in range(K):
        mem = np.flatnonzero(assign == j)
        counts[j] = mem.size
        if mem.size:
            terms = x64[mem] / n[mem, None]
            s = terms.sum(axis=0)
            ns = max(np.sqrt((s * s).sum()), EPS)
            out[j] = s / ns
            bound[j] = mem.size * 2.0 ** -24 * np.abs(terms).sum(axis=0) / ns
    return out, counts, bound


def fit(x, norm, c0, iters, bf16=False):
    """the fit of the definition, centroids carried in fp32 between the iterations as the library carries them"""
    c = np.asarray(c0, dtype=np.float32)
    M = x.shape[0]
    changed, objective, prev = [], [], None
    for i in range(iters):
        a, best, _ = nearest(x, c, norm, bf16)
        changed.append(M if prev is None else int((a != prev).sum()))
        objective.append(best[a >= 0].mean() if (a >= 0).any() else np.nan)
        c = update(x, norm, a, c)[0].astype(np.float32)
        prev = a
    a, best, _ = nearest(x, c, norm, bf16)
    objective.append(best[a >= 0].mean() if (a >= 0).any() else np.nan)
    return dict(centroids=c, assign=a, score=best, counts=np.bincount(a[a >= 0], minlength=c.shape[0]),
                objective=np.array(objective), changed=np.array(changed, dtype=np.int64))


def planted(Z, K, M, seed=0, bf16=False):
    """c_true = K random unit directions; row r = (c_true[r % K] + 0.05 N(0, I)) * a factor in [0.5, 3] -> (x fp32 [M][Z], its fp32
    norms, c_true fp32, labels); bf16: the bank holds bf16 values, as one the bf16 engine exported"""
    rng = np.random.default_rng(seed)
    c_true = rng.standard_normal((K, Z))
    c_true /= np.linalg.norm(c_true, axis=1, keepdims=True)
    labels = np.arange(M) % K
    x = (c_true[labels] + 0.05 * rng.standard_normal((M, Z))) * rng.uniform(0.5, 3.0, size=(M, 1))
    x = op(x.astype(np.float32), bf16)
    norm = np.sqrt((x.astype(np.float64) ** 2).sum(axis=1)).astype(np.float32)
    return x, norm, c_true.astype(np.float32), labels


# ---- the update across sort chunks: assignment patterns and an exact design -----------------------------------------------------------

PATTERNS = ("round_robin", "blocked", "one", "singles", "nobody")


def nobody_values(K):
    """assign values that mean "nobody": -1 and everything else outside [0, K), 64-bit ones included"""
    return np.array([-1, -2, K, K + 5, 2 ** 40, -2 ** 40], dtype=np.int64)


def assign_pattern(kind, M, K, chunk, seed=0):
    """an int64 assign [M] laid out against sort chunks of `chunk` rows:
    round_robin  r % K: every cluster in every chunk (as far as K <= chunk allows)
    blocked      cluster j lives only in chunk j % n_chunks: some clusters are absent from chunk 0, others from the last
    one          cluster 1 % K holds every row
    singles      three single-member clusters at rows chunk - 1, chunk and M - 1 (M > chunk), everybody else nobody
    nobody       round_robin with 10 % of the rows, rows chunk - 1 and chunk among them, drawn from nobody_values(K)"""
    r = np.arange(M, dtype=np.int64)
    n_chunks = (M + chunk - 1) // chunk
    if kind == "round_robin":
        return r % K
    if kind == "blocked":
        c = r // chunk
        per = np.maximum((K - c + n_chunks - 1) // n_chunks, 1)              # clusters congruent to c that exist
        a = c + n_chunks * ((r % chunk) % per)
        return np.where(a < K, a, -1)                                         # (K < n_chunks: a chunk without a cluster)
    if kind == "one":
        return np.full(M, 1 % K, dtype=np.int64)
    if kind == "singles":
        a = np.full(M, -1, dtype=np.int64)
        a[chunk - 1], a[chunk], a[M - 1] = 0, K - 1, K // 2
        return a
    if kind == "nobody":
        rng = np.random.default_rng(seed)
        a = r % K
        out = rng.random(M) < 0.1
        out[[chunk - 1, chunk]] = True
        a[out] = rng.choice(nobody_values(K), size=int(out.sum()))
        return a
    raise ValueError(kind)


def exact_design(Z, M, seed=0):
    """x [M][Z] of small integers with norm 1 everywhere: column 0 is 1 (a member count), column 1 is r % 97 + 1 (which members), the
    rest are integers in [-2, 2].  Every member sum is an integer below 2^24: exact in fp32 in any order."""
    assert Z >= 2 and M * 97 < 2 ** 24
    x = np.random.default_rng(seed).integers(-2, 3, size=(M, Z)).astype(np.float32)
    x[:, 0] = 1.0
    x[:, 1] = np.arange(M) % 97 + 1
    return x, np.ones(M, dtype=np.float32)


def exact_update(x, assign, K):
    """(sums float64 [K][Z] - exact integers -, counts int64 [K]) of exact_design rows under assign"""
    live = (assign >= 0) & (assign < K)
    sums = np.zeros((K, x.shape[1]))
    np.add.at(sums, assign[live], x[live].astype(np.float64))
    return sums, np.bincount(assign[live], minlength=K).astype(np.int64)


def unit(sums):
    """sums / |sums| per row in float64 (rows of zeros stay zero)"""
    n = np.sqrt((sums * sums).sum(axis=1, keepdims=True))
    return sums / np.where(n > 0, n, 1.0)


def finish_bound(Z):
    """first-order relative error per element of c = s / sqrt(sum s_z^2) formed in fp32 from exact s, in the finish kernel's order: a
    lane's fma chain over ceil(Z / 64) columns (one rounding each), 6 butterfly additions, one square root, one division.  The sum of
    squares is a sum of non-negative terms, so its relative error is at most (ceil(Z/64) + 6) u; the root halves that and adds u, the
    division adds u: (ceil(Z/64) + 6) / 2 + 2 <= ceil(Z/64) + 8 roundings of u = 2^-24."""
    return ((Z + 63) // 64 + 8) * 2.0 ** -24
