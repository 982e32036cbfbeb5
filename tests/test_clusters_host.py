"""Code clusters on the host (no GPU): the whole-tensor torch route of CodeClusters.fit / predict / members / representatives against
the float64 restatement (tests/clusters_ref.py) on planted clusters, an empty cluster, the row seeding, refusals, the config block,
the header and the binding.

Tolerances.  Scores: delta = 2 Z 2^-24, the fp32 accumulation bound for unit vectors (sum |a_z b_z| <= 1), plus the project's rtol
1e-3 / atol 1e-5; assignments exactly, after the reference alone has shown that no row's top-two gap is within delta.  Centroids:
the per-element bound clusters_ref.update derives, plus atol 1e-6."""
import os

import numpy as np
import pytest

import clusters_ref as CR

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("codae_nearest_centroid", "codae_nearest_centroid_ws_bytes", "codae_centroid_update", "codae_centroid_update_ws_bytes")


def _tools():
    from codae.hip import HipError
    from codae.tool import CodeClusters, clusters_from_config
    return CodeClusters, clusters_from_config, HipError


def _perturbed(c_true, seed):
    c = c_true + 0.02 * np.random.default_rng(seed).standard_normal(c_true.shape).astype(np.float32)
    return (c / np.linalg.norm(c, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("Z,K,M,precision", [(40, 5, 70, "f32"), (8, 3, 37, "f32"), (72, 19, 150, "bf16")])
def test_host_fit_is_the_float64_statement_on_planted_clusters(Z, K, M, precision):
    CodeClusters, _, _ = _tools()
    bf16 = precision == "bf16"
    x, norm, c_true, labels = CR.planted(Z, K, M, seed=Z + K, bf16=bf16)
    c0 = _perturbed(c_true, 1)
    delta = 2 * Z * 2.0 ** -24
    ref = CR.fit(x, norm, c0, 4, bf16)
    # the reference alone: nobody is excused by a near-tie
    gap = CR.top_two_gap(CR.nearest(x, ref["centroids"], norm, bf16)[2] / norm[:, None].astype(np.float64))
    assert gap.min() > 0.1 > delta, gap.min()
    assert np.array_equal(ref["assign"], labels)
    rows = torch.arange(1000, 1000 + M).flip(0)
    fit = CodeClusters.fit(torch.tensor(x), K, norm=torch.tensor(norm), rows=rows, iters=4, init=torch.tensor(c0), precision=precision)
    assert fit.assign.dtype == torch.long and fit.counts.dtype == torch.long and fit.objective.dtype == torch.float64
    assert tuple(fit.centroids.shape) == (K, Z) and tuple(fit.objective.shape) == (5,) and tuple(fit.changed.shape) == (4,)
    assert np.array_equal(fit.assign.numpy(), ref["assign"])
    assert np.allclose(fit.score.numpy(), ref["score"], rtol=1e-3, atol=1e-5 + delta)
    assert np.array_equal(fit.counts.numpy(), ref["counts"]) and np.array_equal(fit.changed.numpy(), ref["changed"])
    assert fit.changed[0] == M and fit.changed[-1] == 0 and fit.converged_at == int(np.flatnonzero(ref["changed"] == 0)[0])
    assert np.allclose(fit.objective.numpy(), ref["objective"], rtol=1e-3, atol=1e-5 + delta)
    assert (np.diff(fit.objective.numpy()) >= -delta).all()
    want, _, bound = CR.update(x, norm, ref["assign"], ref["centroids"])
    assert (np.abs(fit.centroids.numpy() - want) <= bound + 1e-6).all()
    # predict: the bank's own rows come back, in cluster and score
    cl, sc = fit.predict(torch.tensor(x))
    assert torch.equal(cl, fit.assign) and np.allclose(sc.numpy(), fit.score.numpy(), rtol=1e-3, atol=1e-5 + delta)
    # members and representatives speak dataset rows
    rn = rows.numpy()
    for j in range(K):
        assert np.array_equal(fit.members(j).numpy(), np.sort(rn[ref["assign"] == j]))
    rep = fit.representatives().numpy()
    score = fit.score.numpy()
    for j in range(K):
        mem = np.flatnonzero(ref["assign"] == j)
        top = mem[score[mem] == score[mem].max()]
        assert rep[j] == rn[top].min()


def test_an_empty_cluster_keeps_its_centroid_and_ties_go_to_the_lower_index():
    CodeClusters, _, _ = _tools()
    x, norm, c_true, _ = CR.planted(16, 3, 30, seed=4)
    dup = np.concatenate([c_true[:1], c_true[:1], c_true[1:]])               # centroid 1 duplicates 0: the lower index takes the rows
    assert CodeClusters.fit(torch.tensor(x), 4, iters=0, init=torch.tensor(dup)).counts.tolist() == [10, 0, 10, 10]
    far = -c_true.sum(axis=0)
    far = (far / np.linalg.norm(far)).astype(np.float32)                      # behind every row: never the nearest
    nan = far.copy()
    nan[3] = np.float32(np.nan)                                               # never chosen either, and copied as it is
    c0 = np.concatenate([c_true[:1], far[None], nan[None], c_true[1:]])
    fit = CodeClusters.fit(torch.tensor(x), 5, iters=3, init=torch.tensor(c0))
    assert fit.counts.tolist() == [10, 0, 0, 10, 10]
    assert np.array_equal(fit.centroids.numpy()[1].view(np.uint32), c0[1].view(np.uint32))
    assert np.array_equal(fit.centroids.numpy()[2].view(np.uint32), c0[2].view(np.uint32))
    assert fit.representatives()[1] == -1 and fit.members(1).numel() == 0
    # a row holding a NaN belongs to nobody; an all-zero row goes to centroid 0 with score +0
    y = x.copy()
    y[4, 2] = np.nan
    y[7] = 0.0
    fit = CodeClusters.fit(torch.tensor(y), 3, iters=2, init=torch.tensor(c_true))
    assert fit.assign[4] == -1 and torch.isnan(fit.score[4]) and fit.assign[7] == 0 and fit.score[7] == 0
    assert int(fit.counts.sum()) == 29 and not torch.isnan(fit.centroids).any()


def test_row_seeding_takes_k_distinct_rows_and_repeats_under_the_seed():
    CodeClusters, _, _ = _tools()
    x, norm, _, _ = CR.planted(12, 4, 50, seed=9)
    tx = torch.tensor(x)
    a = CodeClusters.fit(tx, 7, iters=0, seed=3)
    b = CodeClusters.fit(tx, 7, iters=0, seed=3)
    c = CodeClusters.fit(tx, 7, iters=0, seed=4)
    assert torch.equal(a.centroids, b.centroids) and not torch.equal(a.centroids, c.centroids)
    pick = torch.randperm(50, generator=torch.Generator().manual_seed(3))[:7].numpy()
    assert len(set(pick.tolist())) == 7
    unit = x[pick].astype(np.float64) / np.linalg.norm(x[pick].astype(np.float64), axis=1, keepdims=True)
    assert np.allclose(a.centroids.numpy(), unit, rtol=0, atol=1e-6)
    assert tuple(a.changed.shape) == (0,) and tuple(a.objective.shape) == (1,) and a.converged_at is None
    assert int(a.counts.sum()) == 50


def test_refusals_name_the_value():
    CodeClusters, _, HipError = _tools()
    tx = torch.tensor(CR.planted(12, 4, 20, seed=2)[0])
    with pytest.raises(HipError, match="k 21 exceeds the bank's 20"):
        CodeClusters.fit(tx, 21)
    for bad in (0, 4097, -1, 2.0, True):
        with pytest.raises(HipError, match=r"k must be an int in \[1, 4096\]"):
            CodeClusters.fit(tx, bad)
    with pytest.raises(HipError, match="iters"):
        CodeClusters.fit(tx, 3, iters=-1)
    with pytest.raises(HipError, match="precision"):
        CodeClusters.fit(tx, 3, precision="fp16")
    with pytest.raises(HipError, match="init"):
        CodeClusters.fit(tx, 3, init="kmeans++")
    with pytest.raises(HipError, match="init"):
        CodeClusters.fit(tx, 3, init=torch.zeros((3, 11)))
    with pytest.raises(HipError, match="norm"):
        CodeClusters.fit(tx, 3, norm=torch.ones(19))
    with pytest.raises(HipError, match="rows"):
        CodeClusters.fit(tx, 3, rows=[1, 2])
    with pytest.raises(HipError, match="bank"):
        CodeClusters.fit(tx.double(), 3)
    fit = CodeClusters.fit(tx, 3, iters=1)
    with pytest.raises(HipError, match=r"\[Q, 12\]"):
        fit.predict(torch.zeros((2, 13)))
    with pytest.raises(HipError, match="cluster must be an int"):
        fit.members(3)


def test_config_block():
    _, clusters_from_config, HipError = _tools()
    assert clusters_from_config(None) is None and clusters_from_config({}) is None
    assert clusters_from_config({"K": 8}) == {"k": 8, "iters": 25, "seed": 0, "layer": None}
    assert clusters_from_config({"ITERS": 3}) == {"k": 64, "iters": 3, "seed": 0, "layer": None}
    assert clusters_from_config({"K": 4, "ITERS": 5, "SEED": 7, "LAYER": 3}) == {"k": 4, "iters": 5, "seed": 7, "layer": 3}
    with pytest.raises(HipError, match=r"CODE_CLUSTERS: unknown key\(s\) RESTARTS"):
        clusters_from_config({"K": 4, "RESTARTS": 2})
    with pytest.raises(HipError, match="must be a mapping"):
        clusters_from_config(8)
    for bad in (0, 4097, 2.5, True, "8"):
        with pytest.raises(HipError, match="CODE_CLUSTERS: K"):
            clusters_from_config({"K": bad})
    for bad in (-1, 1.0, False):
        with pytest.raises(HipError, match="CODE_CLUSTERS: ITERS"):
            clusters_from_config({"ITERS": bad, "K": 2})
    with pytest.raises(HipError, match="CODE_CLUSTERS: SEED"):
        clusters_from_config({"SEED": "x"})
    with pytest.raises(HipError, match="CODE_CLUSTERS: LAYER"):
        clusters_from_config({"K": 2, "LAYER": 0})


def test_the_header_has_the_section_and_keeps_its_abi_and_the_binding_declares_the_entries():
    text = open(os.path.join(ROOT, "include", "codae_hip.h")).read()
    assert "#define CODAE_ABI_VERSION 11" in text and "CODAE_K_COUNT = 11" in text
    assert "---- Code clusters ----" in text
    for name in ENTRIES:
        assert ("%s(" % name) in text
    from codae import hip
    assert hip.ABI_VERSION == 11 and len(hip.KERNEL_CLASSES) == 11
    for name in ENTRIES:
        assert name in hip.PROTOTYPES
    assert len(hip.PROTOTYPES["codae_nearest_centroid"][1]) == 13 and len(hip.PROTOTYPES["codae_centroid_update"][1]) == 13


def test_the_exact_design_notices_any_one_lost_member_of_any_cluster():
    """the reference alone, for every case of the chunked-update test on the GPU (tests/test_gpu_clusters.py): take any one member out
    of any cluster and either its count changes with the cluster gone, or float64 sums / |sums| moves some element by more than the
    test's bound (twice clusters_ref.finish_bound) - so a sort that loses one row, and with it one that duplicates a row or files it
    under another cluster, cannot pass.  The patterns are also what they claim to be."""
    from test_gpu_clusters import CHUNK_CASES, SORT_CHUNK
    for K, Z, M, kind in CHUNK_CASES:
        x, _ = CR.exact_design(Z, M, seed=K + Z)
        assert np.abs(x).max() * M < 2 ** 24                                  # every partial sum is an exact fp32 integer
        assign = CR.assign_pattern(kind, M, K, SORT_CHUNK, seed=K)
        sums, counts = CR.exact_update(x, assign, K)
        want = CR.unit(sums)
        tol = 2 * CR.finish_bound(Z)
        worst = np.inf
        for j in np.flatnonzero(counts > 1):
            mem = np.flatnonzero(assign == j)
            less = CR.unit(sums[j][None] - x[mem].astype(np.float64))
            moved = (np.abs(less - want[j][None]) / (tol * np.abs(want[j][None]) + 1e-300)).max(axis=1)
            worst = min(worst, moved.min())
        assert worst > 100, (K, Z, M, kind, worst)                            # far outside the bound, not just outside
        chunk_of = np.arange(M) // SORT_CHUNK
        n_chunks = chunk_of[-1] + 1
        valid = (assign >= 0) & (assign < K)
        if kind == "round_robin" and K <= SORT_CHUNK and M % SORT_CHUNK == 0:
            assert all(np.unique(assign[chunk_of == c]).size == K for c in range(n_chunks))
        if kind == "blocked":
            assert (assign[valid] % n_chunks == chunk_of[valid]).all() and n_chunks == 3
            if K >= n_chunks:
                assert valid.all() and (counts > 0).all()
        if kind == "one":
            assert counts.max() == M and (counts > 0).sum() == 1
        if kind == "singles":
            assert counts.sum() == 3 and counts.max() == 1 and (assign[[SORT_CHUNK - 1, SORT_CHUNK, M - 1]] >= 0).all()
        if kind == "nobody":
            out = assign[~valid]
            assert not valid[SORT_CHUNK - 1] and not valid[SORT_CHUNK] and 0.05 * M < out.size < 0.15 * M
            assert set(out.tolist()) == set(CR.nobody_values(K).tolist())
