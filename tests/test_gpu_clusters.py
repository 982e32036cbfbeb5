"""Code clusters on a real MI355X (include/codae_hip.h, "Code clusters"): the nearest-centroid kernel and the centroid update against
the float64 restatement (tests/clusters_ref.py), CodeClusters.fit on the device, and the trainer's code_index().cluster().

Shapes.  Z in {8, 40, 72, 100, 264}: whole and partial MFMA k-chunks (bf16: 32 columns, f32: 16); K in {1, 5, 16, 19, 300}: one
centroid, partial tiles, an exact tile, three groups of the kernel's 128 centroids; M in {1, 37, 70, 700}: a partial row tile, more
than one wave, more than one block (128 rows).  Dense operands take the 16-byte path, ld_x = Z + 3 / ld_c = Z + 1 the element path;
pad columns, two pad rows and the centroid rows past K hold NaN.  At the group edges: K 128 (the last centroid of a whole group), 129 (a
group of one tile) and 4096 (the most the entries take; Z 8 and 40 only).  The update also runs across its 1024-row sort chunks: M in
{1024, 1025, 2500} and K up to 4096 under five assignment patterns (clusters_ref.assign_pattern), see CHUNK_CASES.

Tolerances.  Exact tests: integers in [-2, 2] are exact in bf16 and in every fp32 partial sum (|d| <= 4 * 264), so assign and best
equal the integer reference.  Planted clusters: delta = 2 Z 2^-24, the fp32 accumulation bound for unit vectors (sum |a_z b_z| <= 1);
the reference alone first shows that no row's top-two gap is within delta, then assign must be equal for every row and best within
delta plus the project's rtol 1e-3 / atol 1e-5.  Update: per element count_j 2^-24 sum|terms| / |sum_j| (clusters_ref.update) plus
atol 1e-6.  Update of the exact integer design: twice clusters_ref.finish_bound, derived at the test."""
import numpy as np
import pytest

import clusters_ref as CR

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
ZS = (8, 40, 72, 100, 264)
KM = ((1, 1), (5, 37), (16, 70), (19, 700), (300, 70), (300, 700), (128, 70), (129, 70), (4096, 37))
MAX_K = 4096                        # the most centroids the entries take: checked at Z 8 and 40 only (the reference is [M][K])
ZKM = tuple((Z, K, M) for Z in ZS for K, M in KM if K < MAX_K or Z in (8, 40))
FORMS = (False, True)
FORM_IDS = ("f32", "bf16")
GROUP = 128                         # centroids per accumulator group of the kernel
SORT_CHUNK = 1024                   # rows per chunk of the update's counting sort
SCAN_CLUSTERS = 4                   # clusters per thread of its scan over the chunks
# the update across sort chunks: a whole chunk, one row more, two chunks and a ragged third; Z 72 is two column blocks of the member
# sum; K 1100 and MAX_K put clusters on the scan's threads 75 .. 1023
CHUNK_MS = (1024, 1025, 2500)
CHUNK_KZ = ((5, 8), (19, 40), (19, 72), (1100, 8))
CHUNK_CASES = tuple([(K, Z, M, "round_robin") for M in CHUNK_MS for K, Z in CHUNK_KZ] +
                    [(K, Z, CHUNK_MS[-1], kind) for kind in CR.PATTERNS[1:] for K, Z in CHUNK_KZ] + [(MAX_K, 8, 5000, "round_robin")])
CHUNK_IDS = ["k%d-z%d-m%d-%s" % c for c in CHUNK_CASES]
FIT_CHUNKED = (40, 19, 2500)


def _padded(a, ld, pad_rows=2):
    buf = np.full((a.shape[0] + pad_rows, ld), np.nan, dtype=np.float32)
    buf[:a.shape[0], :a.shape[1]] = a
    return torch.tensor(buf, device=DEV)


def _nearest(x, c, bf16, norm=None, padded=False, rows=None):
    """the kernel on x [M, Z] and c [K, Z]; padded: ld_x = Z + 3, ld_c = Z + 1 (the element path), else dense (16-byte where Z % 4 == 0).
    rows = (lo, hi): a call over that sub-range of the rows.  Pads hold NaN; the outputs' guard elements must stay."""
    from codae import hip
    lib = hip.lib()
    M, Z = x.shape
    K = c.shape[0]
    xb, cb = _padded(x, Z + 3 if padded else Z), _padded(c, Z + 1 if padded else Z)
    lo, hi = rows if rows is not None else (0, M)
    n = hi - lo
    assign = torch.full((n + 1,), -7, dtype=torch.long, device=DEV)
    best = torch.full((n + 1,), 7.0, dtype=torch.float32, device=DEV)
    nb = None if norm is None else torch.tensor(np.asarray(norm, dtype=np.float32)[lo:hi], device=DEV)
    ws = torch.empty(int(lib.codae_nearest_centroid_ws_bytes(Z, K, int(bf16))), dtype=torch.uint8, device=DEV)
    hip.check(lib.codae_nearest_centroid(hip.ptr(xb[lo:]), xb.stride(0), n, Z, hip.ptr(cb), cb.stride(0), K, int(bf16), hip.ptr(nb),
                                         hip.ptr(assign), hip.ptr(best), hip.ptr(ws), hip.current_stream()))
    torch.cuda.synchronize()
    assert assign[n] == -7 and best[n] == 7.0
    return assign[:n].cpu().numpy(), best[:n].cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- exact: small integers ------------------------------------------------------------------------------------------------------------

def _integers(Z, K, M, seed):
    """integer operands with planted exact ties: a duplicate of centroid 0 at K - 1 (K 128: the last centroid of a whole group, K 129:
    alone in a group of one tile), a +0 / -0 pair at 2 / 3, (K > 256) copies of centroid 127 at 128 and 256, across the group
    boundaries, and (K = MAX_K) one more at the first index of the last group; centroids 0 and 127 have no zero entry, so a row equal
    to one of them has its maximum exactly there and at the copies"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-2, 3, size=(M, Z)).astype(np.float32)
    c = rng.integers(-2, 3, size=(K, Z)).astype(np.float32)
    planted = []
    if K >= 5:
        c[0] = rng.choice([-2.0, 2.0], size=Z)
        c[K - 1] = c[0]
        c[2] = 0.0
        c[3] = -0.0
        if M >= 3:
            x[M // 2] = c[0]
            planted.append((M // 2, 0))
    if K > 2 * GROUP:
        c[GROUP - 1] = rng.choice([-2.0, 2.0], size=Z)
        c[GROUP - 1, 0] = -c[0, 0]                                            # (not centroid 0 again)
        c[GROUP], c[2 * GROUP] = c[GROUP - 1], c[GROUP - 1]
        if K == MAX_K:
            c[K - GROUP] = c[GROUP - 1]
        x[M // 3] = c[GROUP - 1]
        planted.append((M // 3, GROUP - 1))
    return x, c, planted


@pytest.mark.parametrize("bf16", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("Z,K,M", ZKM, ids=["%d-k%d-m%d" % s for s in ZKM])
def test_integer_operands_give_the_exact_assignment_and_score(Z, K, M, bf16):
    x, c, planted = _integers(Z, K, M, seed=Z * 1000 + K + M)
    ra, rb, d = CR.nearest(x, c, None, bf16)
    for r, j in planted:                                                      # the ties are really there, and the lower index is the answer
        assert ra[r] == j and (d[r] == d[r].max()).sum() >= 2
    if K >= 5 and M >= 37:
        zero_top = np.flatnonzero(d.max(axis=1) == 0)
        assert (ra[zero_top] <= 2).all()                                      # (the +0 / -0 pair: never index 3)
    for padded in (False, True):
        a, b = _nearest(x, c, bf16, padded=padded)
        assert np.array_equal(a, ra), (padded, np.flatnonzero(a != ra)[:8])
        assert np.array_equal(b, rb.astype(np.float32)), padded


@pytest.mark.parametrize("bf16", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("K", (1, 5, 19))
def test_all_negative_scores_keep_their_true_best_and_pads_never_win(K, bf16):
    rng = np.random.default_rng(K)
    Z, M = 40, 37
    c = rng.integers(1, 3, size=(K, Z)).astype(np.float32)
    x = -rng.integers(1, 3, size=(M, Z)).astype(np.float32)
    ra, rb, d = CR.nearest(x, c, None, bf16)
    assert (d < 0).all()
    for padded in (False, True):
        a, b = _nearest(x, c, bf16, padded=padded)
        assert np.array_equal(a, ra) and np.array_equal(b, rb.astype(np.float32)) and (b < 0).all()


# ---- planted clusters -------------------------------------------------------------------------------------------------------------------

PLANTED = ((8, 1, 37), (8, 5, 37), (40, 5, 70), (72, 19, 70), (264, 16, 700), (100, 300, 700))
_cache = {}


def _planted(Z, K, M, bf16):
    """the shared reference of a planted problem, computed once and never changed"""
    key = (Z, K, M, bf16)
    if key not in _cache:
        x, norm, c_true, labels = CR.planted(Z, K, M, seed=Z + K + M, bf16=bf16)
        a, best, d = CR.nearest(x, c_true, norm, bf16)
        for arr in (x, norm, c_true, labels, a, best, d):
            arr.setflags(write=False)
        _cache[key] = dict(x=x, norm=norm, c=c_true, labels=labels, assign=a, best=best, d=d)
    return _cache[key]


@pytest.mark.parametrize("bf16", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("Z,K,M", PLANTED, ids=["z%d-k%d-m%d" % s for s in PLANTED])
def test_planted_clusters_are_assigned_as_the_float64_statement_assigns_them(Z, K, M, bf16):
    p = _planted(Z, K, M, bf16)
    delta = 2 * Z * 2.0 ** -24
    gap = CR.top_two_gap(p["d"] / p["norm"][:, None].astype(np.float64))
    print("min top-two gap %.4f, delta %.3g" % (gap.min(), delta))
    assert (gap > delta).all()                                                # nobody is excused by a near-tie
    assert np.array_equal(p["assign"], p["labels"])
    for padded in (False, True):
        a, b = _nearest(p["x"], p["c"], bf16, norm=p["norm"], padded=padded)
        err = np.abs(b - p["best"])
        print("padded %d: max score error %.3g" % (padded, err.max()))
        assert np.array_equal(a, p["assign"])
        assert (err <= delta + 1e-5 + 1e-3 * np.abs(p["best"])).all()


# ---- non-finite and degenerate rows -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bf16", FORMS, ids=FORM_IDS)
def test_nan_rows_zero_rows_and_nan_centroids(bf16):
    p = _planted(40, 5, 70, bf16)
    x, c = p["x"].copy(), p["c"].copy()
    x[20, 7] = np.nan
    x[33] = 0.0
    norm = p["norm"].copy()
    norm[20], norm[33] = np.nan, 0.0
    for padded in (False, True):
        a, b = _nearest(x, c, bf16, norm=norm, padded=padded)
        a0, b0 = _nearest(p["x"], c, bf16, norm=p["norm"], padded=padded)
        assert a[20] == -1 and np.isnan(b[20])
        assert a[33] == 0 and _bits(b[33]) == 0                               # +0 exactly
        keep = np.ones(70, dtype=bool)
        keep[[20, 33]] = False
        assert np.array_equal(a[keep], a0[keep]) and np.array_equal(_bits(b[keep]), _bits(b0[keep]))     # the neighbours are untouched
    # a NaN centroid is never chosen: its rows go to their second best
    c[1, 3] = np.nan
    ra, rb, _ = CR.nearest(p["x"], c, p["norm"], bf16)
    assert (ra != 1).all() and (ra >= 0).all()
    a, b = _nearest(p["x"], c, bf16, norm=p["norm"])
    assert np.array_equal(a, ra) and np.allclose(b, rb, rtol=1e-3, atol=1e-5 + 80 * 2.0 ** -24)
    # all centroids NaN: nobody is assigned
    a, b = _nearest(p["x"], np.full_like(c, np.nan), bf16, norm=p["norm"])
    assert (a == -1).all() and np.isnan(b).all()


# ---- independence ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bf16", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("Z,K,M", ((100, 300, 700), (72, 19, 70)), ids=("z100-k300-m700", "z72-k19-m70"))
def test_a_rows_result_depends_on_the_row_and_the_centroids_alone(Z, K, M, bf16):
    p = _planted(Z, K, M, bf16)
    rng = np.random.default_rng(5)
    x = (p["x"] + 0.3 * rng.standard_normal(p["x"].shape).astype(np.float32)).astype(np.float32)     # (scores with many mantissa bits)
    a, b = _nearest(x, p["c"], bf16, norm=p["norm"])
    a2, b2 = _nearest(x, p["c"], bf16, norm=p["norm"])
    assert np.array_equal(a, a2) and np.array_equal(_bits(b), _bits(b2))                             # two calls
    ap, bp = _nearest(x, p["c"], bf16, norm=p["norm"], padded=True)
    assert np.array_equal(a, ap) and np.array_equal(_bits(b), _bits(bp))                             # the other access path
    lo, hi = M // 3 + 1, M // 3 + 1 + min(50, M // 2)
    asub, bsub = _nearest(x, p["c"], bf16, norm=p["norm"], rows=(lo, hi))
    assert np.array_equal(a[lo:hi], asub) and np.array_equal(_bits(b[lo:hi]), _bits(bsub))           # a sub-range of the rows
    for r in (0, M // 2, M - 1):                                                                     # a row alone, at another position
        for padded in (False, True):
            a1, b1 = _nearest(x[r:r + 1], p["c"], bf16, norm=p["norm"][r:r + 1], padded=padded)
            assert a1[0] == a[r] and _bits(b1)[0] == _bits(b)[r]
            other = np.concatenate([x[:5], x[r:r + 1], x[:3]])
            a3, b3 = _nearest(other, p["c"], bf16, norm=np.concatenate([p["norm"][:5], p["norm"][r:r + 1], p["norm"][:3]]), padded=padded)
            assert a3[5] == a[r] and _bits(b3)[5] == _bits(b)[r]


# ---- the update ---------------------------------------------------------------------------------------------------------------------------------

def _update(x, norm, assign, c_in, padded=False, alias=False):
    from codae import hip
    lib = hip.lib()
    M, Z = x.shape
    K = c_in.shape[0]
    xb, cb = _padded(x, Z + 3 if padded else Z), _padded(c_in, Z + 1 if padded else Z)
    out = cb if alias else torch.full_like(cb, 7.0)
    nb = torch.tensor(np.asarray(norm, dtype=np.float32), device=DEV)
    ab = torch.tensor(np.asarray(assign, dtype=np.int64), device=DEV)
    counts = torch.full((K + 1,), -7, dtype=torch.long, device=DEV)
    ws = torch.empty(int(lib.codae_centroid_update_ws_bytes(M, Z, K)), dtype=torch.uint8, device=DEV)
    hip.check(lib.codae_centroid_update(hip.ptr(xb), xb.stride(0), M, Z, hip.ptr(nb), hip.ptr(ab), hip.ptr(cb), hip.ptr(out), out.stride(0), K,
                                        hip.ptr(counts), hip.ptr(ws), hip.current_stream()))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert counts[K] == -7
    if not alias:
        assert (got[K:] == 7.0).all() and (got[:, Z:] == 7.0).all()          # pads are never written
    return got[:K, :Z].copy(), counts[:K].cpu().numpy()


@pytest.mark.parametrize("Z,K,M", PLANTED[1:], ids=["z%d-k%d-m%d" % s for s in PLANTED[1:]])
def test_update_is_the_float64_statement_within_the_derived_bound(Z, K, M):
    p = _planted(Z, K, M, False)
    rng = np.random.default_rng(Z)
    assign = p["labels"].copy()
    assign[rng.random(M) < 0.1] = -1                                          # rows that belong to nobody
    assign[assign == 2] = 0                                                   # an empty cluster (2), a larger one (0)
    c_in = p["c"].copy()
    c_in[2, 1] = np.array([0x7FC12345], dtype=np.uint32).view(np.float32)[0]  # a NaN payload: copied, not recomputed
    want, counts, bound = CR.update(p["x"], p["norm"], assign, c_in)
    assert counts[2] == 0 and counts.sum() == (assign >= 0).sum()
    got, gc = _update(p["x"], p["norm"], assign, c_in)
    assert np.array_equal(gc, counts)
    assert np.array_equal(_bits(got[2]), _bits(c_in[2]))                      # the empty cluster keeps c_in's bits
    live = counts > 0
    err = np.abs(got[live] - want[live])
    print("max error %.3g, max bound %.3g" % (err.max(), bound[live].max()))
    assert (err <= bound[live] + 1e-6).all()
    # twice, on the other access path and in place: the same bits
    for kw in (dict(), dict(padded=True), dict(alias=True), dict(padded=True, alias=True)):
        g2, c2 = _update(p["x"], p["norm"], assign, c_in, **kw)
        assert np.array_equal(_bits(g2), _bits(got)) and np.array_equal(c2, counts), kw


def test_update_of_one_member_and_of_one_cluster_that_holds_every_row():
    p = _planted(72, 19, 700, False)
    x, norm = p["x"], p["norm"]
    # a cluster of one member is that row's unit vector
    assign = np.full(700, -1, dtype=np.int64)
    assign[123] = 4
    want, counts, bound = CR.update(x, norm, assign, p["c"])
    got, gc = _update(x, norm, assign, p["c"])
    unit = x[123].astype(np.float64) / np.linalg.norm(x[123].astype(np.float64))
    assert gc.tolist() == counts.tolist() and gc[4] == 1 and gc.sum() == 1
    assert (np.abs(got[4] - unit) <= bound[4] + 1e-6).all()
    others = np.arange(19) != 4
    assert np.array_equal(_bits(got[others]), _bits(p["c"][others]))
    # the imbalanced case: all 700 rows in one of the 19 clusters
    assign = np.full(700, 7, dtype=np.int64)
    want, counts, bound = CR.update(x, norm, assign, p["c"])
    got, gc = _update(x, norm, assign, p["c"])
    assert gc.tolist() == counts.tolist() and gc[7] == 700
    err = np.abs(got[7] - want[7])
    print("max error %.3g, max bound %.3g" % (err.max(), bound[7].max()))
    assert (err <= bound[7] + 1e-6).all()
    g2, _ = _update(x, norm, assign, p["c"], padded=True)
    assert np.array_equal(_bits(g2), _bits(got))


# ---- the update across sort chunks ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,Z,M,kind", CHUNK_CASES, ids=CHUNK_IDS)
def test_chunked_update_of_an_exact_design_counts_exactly_and_normalises_within_the_finish_bound(K, Z, M, kind):
    """x is clusters_ref.exact_design: integers with norm 1, so every member sum is exact in fp32 whatever the order, and what is left
    between c_out and float64 sums / |sums| is the finish kernel alone: per lane an fma chain over ceil(Z / 64) squares, 6 butterfly
    additions (all terms non-negative: relative error <= (ceil(Z/64) + 6) u, u = 2^-24), a square root (halves it, adds u) and one
    division (adds u): to first order (ceil(Z/64) + 6) / 2 + 2 <= ceil(Z/64) + 8 roundings per element (clusters_ref.finish_bound).
    Asserted at twice that.  Column 0 counts the members and column 1 tells them apart, so a lost, duplicated or foreign member
    moves an element by >= 1 / (2 count) relative: tests/test_clusters_host.py shows it for every member of every design."""
    x, norm = CR.exact_design(Z, M, seed=K + Z)
    assign = CR.assign_pattern(kind, M, K, SORT_CHUNK, seed=K)
    sums, counts = CR.exact_update(x, assign, K)
    want = CR.unit(sums)
    c_in = np.random.default_rng(1).standard_normal((K, Z)).astype(np.float32)
    got, gc = _update(x, norm, assign, c_in)
    assert np.array_equal(gc, counts)
    live = counts > 0
    assert np.array_equal(_bits(got[~live]), _bits(c_in[~live]))
    bound = CR.finish_bound(Z)
    ratio = np.abs(got[live] - want[live]) / (bound * np.abs(want[live]) + 1e-300)
    ratio[(want[live] == 0) & (got[live] == 0)] = 0.0
    print("MEASURE chunked update exact k%d z%d m%d %s: worst error / bound %.3f" % (K, Z, M, kind, ratio.max() if live.any() else 0.0))
    assert (ratio <= 2.0).all()


def _member_list_bits(x, norm, assign, c_in, clusters):
    """row j of c_out from a call that holds only the members of j, in their order: a single-chunk call, for each j in clusters"""
    from codae import hip
    lib = hip.lib()
    M, Z = x.shape
    K = c_in.shape[0]
    xd, nd, cb = torch.tensor(x, device=DEV), torch.tensor(norm, device=DEV), torch.tensor(c_in, device=DEV)
    out = torch.full((K + 1, Z), 7.0, device=DEV)
    counts = torch.full((K + 1,), -7, dtype=torch.long, device=DEV)
    res = torch.zeros((len(clusters), Z), device=DEV)
    ws = torch.empty(int(lib.codae_centroid_update_ws_bytes(SORT_CHUNK, Z, K)), dtype=torch.uint8, device=DEV)
    for i, j in enumerate(clusters):
        mem = torch.tensor(np.flatnonzero(assign == j), device=DEV)
        n = int(mem.numel())
        assert 1 <= n <= SORT_CHUNK
        xs, ns = xd[mem].contiguous(), nd[mem].contiguous()
        ab = torch.full((n,), int(j), dtype=torch.long, device=DEV)
        hip.check(lib.codae_centroid_update(hip.ptr(xs), Z, n, Z, hip.ptr(ns), hip.ptr(ab), hip.ptr(cb), hip.ptr(out), Z, K, hip.ptr(counts),
                                            hip.ptr(ws), hip.current_stream()))
        res[i] = out[j]
    torch.cuda.synchronize()
    assert counts[K] == -7 and (out[K] == 7.0).all()
    return res.cpu().numpy()


@pytest.mark.parametrize("K,Z,M,kind", CHUNK_CASES, ids=CHUNK_IDS)
def test_chunked_update_of_planted_rows_has_the_bits_of_each_member_list_alone(K, Z, M, kind):
    """non-integer rows with their own norms.  "Every fp32 sum runs in an order fixed by the member list alone": a live cluster of at
    most SORT_CHUNK members has the bits of a call that holds only its members (one chunk: the path the small tests cover); a larger
    one is held to clusters_ref.update's float64 bound.  Cluster 3 is emptied and keeps c_in's bits, a NaN payload included; the
    padded (ld_x = Z + 3, ld_c = Z + 1) and the in-place forms give the bits of the dense out-of-place one."""
    x, norm, c_true, _ = CR.planted(Z, K, M, seed=Z + K + M)
    assign = CR.assign_pattern(kind, M, K, SORT_CHUNK, seed=K)
    assign[assign == 3] = -1
    c_in = c_true.copy()
    c_in[3, 1] = np.array([0x7FC12345], dtype=np.uint32).view(np.float32)[0]
    want, counts, bound = CR.update(x, norm, assign, c_in)
    assert counts[3] == 0
    got, gc = _update(x, norm, assign, c_in)
    assert np.array_equal(gc, counts)
    live = np.flatnonzero(counts > 0)
    assert np.array_equal(_bits(got[counts == 0]), _bits(c_in[counts == 0]))
    small = [j for j in live if counts[j] <= SORT_CHUNK]
    alone = _member_list_bits(x, norm, assign, c_in, small)
    differ = [j for i, j in enumerate(small) if not np.array_equal(_bits(alone[i]), _bits(got[j]))]
    assert not differ, (len(differ), differ[:8])
    err = np.abs(got[live] - want[live])
    assert (err <= bound[live] + 1e-6).all()
    for kw in (dict(padded=True), dict(alias=True), dict(padded=True, alias=True)):
        g2, c2 = _update(x, norm, assign, c_in, **kw)
        assert np.array_equal(_bits(g2), _bits(got)) and np.array_equal(c2, counts), kw


def test_the_entries_refuse_bad_arguments_before_any_launch():
    from codae import hip
    lib = hip.lib()
    x = torch.ones((8, 8), device=DEV)
    c = torch.ones((4, 8), device=DEV)
    n = torch.ones(8, device=DEV)
    a = torch.full((8,), -7, dtype=torch.long, device=DEV)
    b = torch.full((8,), 7.0, device=DEV)
    cnt = torch.full((4,), -7, dtype=torch.long, device=DEV)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    s = hip.current_stream()

    def near(M=8, Z=8, K=4, ld_x=8, ld_c=8, op=0, xp=x):
        rc = lib.codae_nearest_centroid(hip.ptr(xp), ld_x, M, Z, hip.ptr(c), ld_c, K, op, hip.ptr(n), hip.ptr(a), hip.ptr(b), hip.ptr(ws), s)
        return rc, lib.codae_last_error().decode()

    def upd(M=8, Z=8, K=4, ld_x=8, ld_c=8):
        rc = lib.codae_centroid_update(hip.ptr(x), ld_x, M, Z, hip.ptr(n), hip.ptr(a), hip.ptr(c), hip.ptr(c), ld_c, K, hip.ptr(cnt), hip.ptr(ws), s)
        return rc, lib.codae_last_error().decode()
    for call in (near, upd):
        for kw, word in ((dict(K=0), "K 0"), (dict(K=4097), "K 4097"), (dict(M=0), "M 0"), (dict(Z=0), "Z 0"), (dict(ld_x=7), "ld_x 7"),
                         (dict(ld_c=5), "ld_c 5")):
            rc, msg = call(**kw)
            assert rc == -1 and word in msg, (kw, rc, msg)
    rc, msg = near(op=2)
    assert rc == -1 and "op_bf16 2" in msg
    rc, msg = near(xp=None)
    assert rc == -1 and "NULL" in msg
    assert lib.codae_nearest_centroid_ws_bytes(8, 0, 0) == -1 and lib.codae_nearest_centroid_ws_bytes(8, 4097, 1) == -1
    assert lib.codae_centroid_update_ws_bytes(0, 8, 4) == -1 and lib.codae_centroid_update_ws_bytes(8, 8, 4097) == -1
    torch.cuda.synchronize()
    assert (a == -7).all() and (b == 7.0).all() and (cnt == -7).all() and (c == 1).all()            # a refusal launches nothing


# ---- fit ----------------------------------------------------------------------------------------------------------------------------------------

def _perturbed(c_true, seed):
    c = c_true + 0.02 * np.random.default_rng(seed).standard_normal(c_true.shape).astype(np.float32)
    return (c / np.linalg.norm(c, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("bf16", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("Z,K,M", ((40, 5, 70), (100, 300, 700), FIT_CHUNKED), ids=("z40-k5-m70", "z100-k300-m700", "z40-k19-m2500"))
def test_fit_recovers_the_planted_labels_and_stays_at_its_fixed_point(Z, K, M, bf16):
    from codae.tool import CodeClusters
    p = _planted(Z, K, M, bf16)
    precision = "bf16" if bf16 else "f32"
    delta = 2 * Z * 2.0 ** -24
    c0 = torch.tensor(_perturbed(p["c"], 3))
    xd, nd = torch.tensor(p["x"], device=DEV), torch.tensor(p["norm"], device=DEV)
    fit = CodeClusters.fit(xd, K, norm=nd, iters=4, init=c0.to(DEV), precision=precision)
    assert fit.centroids.device.type == "cuda" and fit.assign.dtype == torch.long
    assert np.array_equal(fit.assign.cpu().numpy(), p["labels"])
    changed, objective = fit.changed.cpu().numpy(), fit.objective.cpu().numpy()
    assert changed[0] == M and fit.converged_at is not None and (changed[fit.converged_at:] == 0).all()
    assert tuple(objective.shape) == (5,) and (np.diff(objective) >= -delta).all()
    assert np.array_equal(fit.counts.cpu().numpy(), np.bincount(p["labels"], minlength=K))
    # assign belongs to the returned centroids
    cl, sc = fit.predict(xd)                                                  # (predict divides by norms it forms itself: an ulp apart)
    assert torch.equal(cl, fit.assign) and np.allclose(sc.cpu().numpy(), fit.score.cpu().numpy(), rtol=1e-6, atol=0)
    # further iterations past convergence change no bit of any output
    more = CodeClusters.fit(xd, K, norm=nd, iters=7, init=c0.to(DEV), precision=precision)
    assert torch.equal(more.centroids.view(torch.int32), fit.centroids.view(torch.int32))
    assert torch.equal(more.assign, fit.assign) and torch.equal(more.score.view(torch.int32), fit.score.view(torch.int32))
    assert torch.equal(more.counts, fit.counts) and more.converged_at == fit.converged_at
    assert more.objective[-1] == fit.objective[-1] and (more.changed[4:] == 0).all()
    # the host route: the same assignment, the centroids within the update bound
    host = CodeClusters.fit(torch.tensor(p["x"]), K, norm=torch.tensor(p["norm"]), iters=4, init=c0, precision=precision)
    assert np.array_equal(host.assign.numpy(), fit.assign.cpu().numpy())
    assert np.array_equal(host.changed.numpy(), changed)
    want, _, bound = CR.update(p["x"], p["norm"], p["labels"], host.centroids.numpy())
    assert (np.abs(fit.centroids.cpu().numpy() - want) <= bound + 1e-6).all()
    assert (np.abs(host.centroids.numpy() - want) <= bound + 1e-6).all()
    assert np.allclose(host.objective.numpy(), objective, rtol=1e-3, atol=1e-5 + delta)


def test_fit_seeds_from_rows_on_the_device_as_on_the_host():
    from codae.tool import CodeClusters
    p = _planted(40, 5, 70, False)
    dev = CodeClusters.fit(torch.tensor(p["x"], device=DEV), 5, iters=0, seed=11)
    host = CodeClusters.fit(torch.tensor(p["x"]), 5, iters=0, seed=11)
    assert np.allclose(dev.centroids.cpu().numpy(), host.centroids.numpy(), rtol=0, atol=1e-6)
    assert np.array_equal(dev.assign.cpu().numpy(), host.assign.numpy())


# ---- the trainer ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ("f32", "bf16"))
def test_code_index_cluster_on_the_fixture_trainer_leaves_its_state_alone(precision):
    from codae.hip import HipError
    from test_gpu_codes import _kw
    from test_gpu_norm import _idx, _square, _trainer
    p = _square(5, 24, 70, "relu", seed=121)
    t = _trainer(p, precision, **_kw("layer", "hidden"))
    t.train_batch(_idx(p, 0), run=0)
    t.eval_batch(_idx(p, 1), run=0)                                           # (the metric sums hold something)
    dig, scal, sums = t.state_digest(), t.engine.scalars.clone(), t.epoch_sums(reset=False)
    index = t.code_index(layer=2)
    assert index.precision == precision
    fit = index.cluster(k=4, iters=5)
    N = p["N"]
    assert fit.precision == precision and fit.rows is None
    assert tuple(fit.centroids.shape) == (4, 24) and tuple(fit.assign.shape) == (N,) and tuple(fit.score.shape) == (N,)
    assert tuple(fit.counts.shape) == (4,) and tuple(fit.objective.shape) == (6,) and tuple(fit.changed.shape) == (5,)
    a = fit.assign.cpu().numpy()
    assert ((a >= 0) & (a < 4)).all() and np.array_equal(fit.counts.cpu().numpy(), np.bincount(a, minlength=4))
    assert int(fit.changed[0]) == N and np.isfinite(fit.objective.cpu().numpy()).all()
    # the returned assignment is that of the float64 statement on the returned centroids, wherever the top-two gap is not a near-tie
    bank, norm = index.bank.cpu().numpy(), index.norm.cpu().numpy()
    ra, rb, d = CR.nearest(bank, fit.centroids.cpu().numpy(), norm, precision == "bf16")
    clear = CR.top_two_gap(d / np.maximum(norm, 1e-8)[:, None].astype(np.float64)) > 2 * 24 * 2.0 ** -24
    assert clear.mean() > 0.9 and np.array_equal(a[clear], ra[clear])
    assert np.allclose(fit.score.cpu().numpy()[clear], rb[clear], rtol=1e-3, atol=1e-5 + 2 * 24 * 2.0 ** -24)
    # a partial outfit's code finds a cluster
    cl, sc = fit.predict(t.encode(_idx(p, 1)[:9], blank=0, layer=2))
    assert tuple(cl.shape) == (9,) and ((cl >= 0) & (cl < 4)).all() and torch.isfinite(sc).all()
    # an index over a subset answers in dataset rows
    sub = t.code_index(rows=[50, 7, 99, 3, 20, 31], layer=2).cluster(k=2, iters=3)
    assert sub.rows.tolist() == [3, 7, 20, 31, 50, 99]
    both = torch.cat([sub.members(0), sub.members(1)]).tolist()
    assert sorted(both) == [3, 7, 20, 31, 50, 99] and sub.members(0).tolist() == sorted(sub.members(0).tolist())
    rep = sub.representatives().tolist()
    assert all(r == -1 or r in sub.members(j).tolist() for j, r in enumerate(rep))
    # nothing of the trainer moved
    torch.cuda.synchronize()
    assert t.state_digest() == dig
    assert torch.equal(t.engine.scalars.view(torch.int64), scal.view(torch.int64)) and t.epoch_sums(reset=False) == sums
    # refusals name the value
    with pytest.raises(HipError, match="k 7 exceeds the bank's 6"):
        t.code_index(rows=[50, 7, 99, 3, 20, 31], layer=2).cluster(k=7)
    for bad in (0, 4097):
        with pytest.raises(HipError, match=r"k must be an int in \[1, 4096\], got %d" % bad):
            index.cluster(k=bad)
    with pytest.raises(HipError, match="the query is on cpu"):
        fit.predict(torch.zeros((2, 24)))
    with pytest.raises(HipError, match=r"\[Q, 24\].*25"):
        fit.predict(torch.zeros((2, 25), device=DEV))
    assert t.state_digest() == dig
