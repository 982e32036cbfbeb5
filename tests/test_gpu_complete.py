"""Complementarity inference on a real MI355X: the top-k selection kernel bit for bit against numpy, the end-to-end entry
(codae_complete_topk: fp32 GEMM per candidate chunk + selection) against float64 in both CODAE_F32_GEMM modes, device =
host, determinism, agreement with the rank metric, and HipEmbeddingTrainer.complete."""
import types

import numpy as np
import pytest

from complete_ref import check_topk, ref_ranked

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    from codae import hip as H
    H.lib()
    return H


@pytest.fixture
def f32_gemm_mode(hip, monkeypatch):
    """CODAE_F32_GEMM for one test (native = fp32 MFMA, x3 = three bf16 planes per operand), restored afterwards"""
    def set_mode(mode):
        monkeypatch.setenv("CODAE_F32_GEMM", mode)
        hip.check(hip.lib().codae_reload_env())
    yield set_mode
    monkeypatch.delenv("CODAE_F32_GEMM", raising=False)
    hip.check(hip.lib().codae_reload_env())


# ---- the selection primitive -----------------------------------------------------------------------------------------
def adversarial_scores(B, n, seed):
    """heavy ties, +-0, +-inf, NaN and ordinary floats"""
    rng = np.random.default_rng(seed)
    pool = np.array([1.0, 0.5, 0.0, -0.0, -0.5, -1.0, np.inf, -np.inf, np.nan, 0.25, 0.25, 0.0], dtype=np.float32)
    s = pool[rng.integers(0, len(pool), (B, n))]
    mix = rng.random((B, n)) < 0.4
    s[mix] = rng.standard_normal(int(mix.sum())).astype(np.float32)
    if B > 1:
        s[0] = np.nan                         # a row with nothing to return
        s[1, :] = -0.0                        # all ties at zero
    return s


def ref_select(s, k, skip):
    """(positions, scores) [B, k]: score descending (-0 == +0), position ascending among equals, no NaN, no skip_col."""
    B, n = s.shape
    idx = np.full((B, k), -1, dtype=np.int32)
    sc = np.full((B, k), -np.inf, dtype=np.float32)
    cols = np.arange(n)
    for b in range(B):
        v = s[b] + np.float32(0.0)
        ok = ~np.isnan(v)
        if skip is not None and skip[b] >= 0:
            ok &= cols != skip[b]
        c, x = cols[ok], v[ok]
        o = np.lexsort((c, -x))[:k]
        idx[b, :len(o)] = c[o]
        sc[b, :len(o)] = x[o]
    return idx, sc


def run_select(hip, s, k, chunk, skip=None, row_id=None):
    B, n = s.shape
    L = hip.lib()
    st = hip.current_stream()
    sd = torch.from_numpy(s).to(DEV)
    state = torch.empty(B * k, dtype=torch.int64, device=DEV)
    skip_d = None if skip is None else torch.from_numpy(skip.astype(np.int32)).to(DEV)
    rid = None if row_id is None else torch.from_numpy(row_id.astype(np.int32)).to(DEV)
    oi = torch.empty((B, k), dtype=torch.int32, device=DEV)
    os_ = torch.empty((B, k), dtype=torch.float32, device=DEV)
    hip.check(L.codae_topk_init(hip.ptr(state), B, k, st))
    for c0 in range(0, n, chunk):
        m = min(chunk, n - c0)
        # each chunk is a view of the whole matrix (ld = n): columns c0 .. c0 + m - 1
        hip.check(L.codae_topk_merge(hip.ptr(sd[:, c0:]), n, B, m, c0, k, None, hip.ptr(skip_d), hip.ptr(state), st))
    hip.check(L.codae_topk_finish(hip.ptr(state), B, k, hip.ptr(rid), hip.ptr(oi), hip.ptr(os_), st))
    torch.cuda.synchronize()
    return oi.cpu().numpy(), os_.cpu().numpy()


@pytest.mark.parametrize("k", [1, 10, 64, 100, 256])
@pytest.mark.parametrize("B,n,chunk", [(1, 1000, 1000), (37, 1000, 333), (5, 70, 64), (300, 2500, 1024)])
def test_selection_kernel_is_exact(hip, k, B, n, chunk):
    s = adversarial_scores(B, n, seed=k * 1000 + n)
    idx, sc = run_select(hip, s, k, chunk)
    ri, rs = ref_select(s, k, None)
    assert np.array_equal(idx, ri)
    assert np.array_equal(sc.view(np.uint32), rs.view(np.uint32))        # bit for bit (-0 comes back as +0)


@pytest.mark.parametrize("k", [10, 256])
def test_selection_kernel_skip_col_row_ids_and_many_rows(hip, k):
    B, n = 8192, 700
    s = adversarial_scores(B, n, seed=k)
    rng = np.random.default_rng(k)
    skip = rng.integers(-1, n, B)
    row_id = rng.permutation(10 * n)[:n]
    idx, sc = run_select(hip, s, k, 256, skip=skip, row_id=row_id)
    ri, rs = ref_select(s, k, skip)
    assert np.array_equal(idx, np.where(ri >= 0, row_id[np.maximum(ri, 0)], -1))
    assert np.array_equal(sc.view(np.uint32), rs.view(np.uint32))


def test_selection_kernel_worst_case_order(hip):
    """ascending scores: every element beats the running threshold, the survivor buffer fills and merges over and over"""
    B, n = 8, 5000
    s = np.tile(np.arange(n, dtype=np.float32), (B, 1))
    s[1] = s[1][::-1].copy()
    for k in (1, 100, 256):
        idx, sc = run_select(hip, s, k, 1111)
        ri, rs = ref_select(s, k, None)
        assert np.array_equal(idx, ri) and np.array_equal(sc.view(np.uint32), rs.view(np.uint32))


def test_selection_argument_errors(hip):
    L = hip.lib()
    st = hip.current_stream()
    state = torch.empty(64, dtype=torch.int64, device=DEV)
    s = torch.zeros(4, 16, device=DEV)
    assert L.codae_topk_init(hip.ptr(state), 4, 0, st) != 0
    assert L.codae_topk_init(hip.ptr(state), 4, 257, st) != 0
    assert L.codae_topk_merge(hip.ptr(s), 16, 4, 16, 0, 300, None, None, hip.ptr(state), st) != 0
    assert L.codae_topk_merge(hip.ptr(s), 8, 4, 16, 0, 4, None, None, hip.ptr(state), st) != 0     # ld < n
    assert L.codae_topk_merge(hip.ptr(s), 16, 0, 16, 0, 4, None, None, hip.ptr(state), st) != 0


# ---- end to end -------------------------------------------------------------------------------------------------------
def dataset(S, E, N, seed):
    rng = np.random.default_rng(seed)
    blocks = [rng.standard_normal((N, E)).astype(np.float32) for _ in range(S)]
    ds = types.SimpleNamespace(nb_used_category=S, embedding_size=E,
                               data_per_category={c: torch.from_numpy(blocks[c].copy()) for c in range(S)})
    return ds, blocks


def near_queries(blocks, S, E, B, seed, noise=0.3):
    """queries near inventory rows (a realistic score spread: a few close items, many far ones)"""
    rng = np.random.default_rng(seed)
    q = np.concatenate([blocks[c][rng.integers(0, blocks[c].shape[0], B)] for c in range(S)], axis=1)
    return (q + noise * rng.standard_normal(q.shape)).astype(np.float32)


def same_up_to_ties(a_idx, a_sc, b_idx, b_sc, tol=1e-5):
    """two results agree: equal (-1, -inf) tails, scores of shared items within tol, differing items only within tol of the k-th"""
    for b in range(a_idx.shape[0]):
        A = dict(zip(a_idx[b].tolist(), a_sc[b].tolist()))
        Bm = dict(zip(b_idx[b].tolist(), b_sc[b].tolist()))
        assert (a_idx[b] == -1).sum() == (b_idx[b] == -1).sum(), b
        for i in set(A) & set(Bm) - {-1}:
            assert abs(A[i] - Bm[i]) <= tol, (b, i)
        kth = min(a_sc[b][a_idx[b] >= 0].min(initial=np.inf), b_sc[b][b_idx[b] >= 0].min(initial=np.inf))
        for i in (set(A) ^ set(Bm)) - {-1}:
            v = A[i] if i in A else Bm[i]
            assert abs(v - kth) <= 2 * tol, (b, i, v, kth)


@pytest.mark.parametrize("mode", ["x3", "native"])
@pytest.mark.parametrize("S,E,N,B,chunk", [(3, 64, 3000, 96, 1024), (3, 512, 20480, 512, 8192)])
def test_end_to_end_matches_float64_and_host(hip, f32_gemm_mode, mode, S, E, N, B, chunk):
    from codae.tool import ComplementRetriever
    f32_gemm_mode(mode)
    ds, blocks = dataset(S, E, N, seed=E)
    pred = near_queries(blocks, S, E, B, seed=E + 1)
    rng = np.random.default_rng(7)
    slots = rng.integers(0, S, B)
    exclude = rng.integers(0, N, B)
    dev_r = ComplementRetriever(ds, DEV)
    host_r = ComplementRetriever(ds, "cpu")
    pd = torch.from_numpy(pred).to(DEV)
    for k in (10, 100):
        for ex in (None, exclude):
            ex_t = None if ex is None else torch.from_numpy(ex)
            idx, sc = dev_r.topk(pd, torch.from_numpy(slots).to(DEV), k, exclude=None if ex is None else ex_t.to(DEV), chunk=chunk)
            idx, sc = idx.cpu().numpy(), sc.cpu().numpy()
            check_topk(idx, sc, ref_ranked(pred, slots, blocks, E, k, exclude=ex), k)
            hi, hs = host_r.topk(torch.from_numpy(pred), torch.from_numpy(slots), k, exclude=ex_t)
            same_up_to_ties(idx, sc, hi.numpy(), hs.numpy())


def test_end_to_end_edge_cases(hip):
    """candidate subset + distinct with planted duplicates, k beyond the candidate count, NaN and zero queries, int slot,
    a device slot outside [0, S) (its row comes back empty)"""
    from codae.tool import ComplementRetriever
    S, E, N, B = 3, 64, 500, 40
    ds, blocks = dataset(S, E, N, seed=3)
    for c in range(S):
        ds.data_per_category[c][100:110] = ds.data_per_category[c][105]
        blocks[c][100:110] = blocks[c][105]
    pred = near_queries(blocks, S, E, B, seed=4)
    pred[0, :] = np.nan
    pred[1, :] = 0.0
    cands = list(range(90, 130)) + [7, 400]
    for distinct in (True, False):
        r = ComplementRetriever(ds, DEV, candidates=cands, distinct=distinct)
        n_items = len(cands) - (9 if distinct else 0)
        for k in (5, 64):
            slots = np.arange(B) % S
            ex = np.full(B, 103)
            idx, sc = r.topk(torch.from_numpy(pred).to(DEV), torch.from_numpy(slots).to(DEV), k, exclude=torch.from_numpy(ex).to(DEV))
            idx, sc = idx.cpu().numpy(), sc.cpu().numpy()
            check_topk(idx, sc, ref_ranked(pred, slots, blocks, E, k, candidates=cands, distinct=distinct, exclude=ex), k)
            assert (idx[0] == -1).all()
            assert (sc[1, :min(k, n_items - 1)] == 0).all()
            hi, hs = ComplementRetriever(ds, "cpu", candidates=cands, distinct=distinct).topk(
                torch.from_numpy(pred), torch.from_numpy(slots), k, exclude=torch.from_numpy(ex))
            same_up_to_ties(idx, sc, hi.numpy(), hs.numpy())
        idx, _ = r.topk(torch.from_numpy(pred).to(DEV), 2, 3)
        assert idx.shape == (B, 3)
        bad = torch.tensor([0, 5] + [1] * (B - 2), dtype=torch.int32, device=DEV)
        idx, sc = r.topk(torch.from_numpy(pred).to(DEV), bad, 3)
        assert (idx[1] == -1).all().item() and torch.isneginf(sc[1]).all().item() and (idx[2] >= 0).all().item()


def test_end_to_end_is_deterministic(hip):
    from codae.tool import ComplementRetriever
    S, E, N, B = 3, 512, 20480, 1024
    ds, blocks = dataset(S, E, N, seed=11)
    pd = torch.from_numpy(near_queries(blocks, S, E, B, seed=12)).to(DEV)
    slots = torch.arange(B, device=DEV) % S
    r = ComplementRetriever(ds, DEV, distinct=False)
    a = r.topk(pd, slots, 100, chunk=4096)
    b = r.topk(pd, slots, 100, chunk=4096)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_position_of_own_row_matches_the_rank_metric(hip):
    """candidates = the validation rows, k = their count, distinct=False: query b's own row sits at n_val - 1 - rank_b,
    rank_b as codae_ranking_loss_batched counts it (one query per call, so its sum is the row's rank); a query with
    another candidate within 1e-6 of its own score may differ by one"""
    from codae.tool import ComplementRetriever, Corrupter, RankingLoss
    S, E, N = 3, 64, 600
    ds, blocks = dataset(S, E, N, seed=21)
    ds.nb_predictor = S * E
    rng = np.random.default_rng(22)
    val = sorted(rng.choice(N, 200, replace=False).tolist())
    V = len(val)
    arch = [{"name": str(s), "size": E, "position": s * E, "type": "regression", "lambda": 1} for s in range(S)]
    cor = Corrupter(N, arch, 1, DEV)
    rl = RankingLoss(ds, val, DEV)
    r = ComplementRetriever(ds, DEV, candidates=val, distinct=False)
    rows = rng.choice(val, 24, replace=False)
    pred = near_queries(blocks, S, E, len(rows), seed=23)
    slot_of = cor.mask_to_use_i32[torch.from_numpy(rows).to(DEV), 0].cpu().numpy()     # mask id c = the 1-subset {c}
    idx, sc = r.topk(torch.from_numpy(pred).to(DEV), torch.from_numpy(slot_of.astype(np.int64)).to(DEV), V)
    idx = idx.cpu().numpy()
    for b, row in enumerate(rows):
        rl.add(torch.from_numpy(pred[b:b + 1]).to(DEV), torch.tensor([row], dtype=torch.int32, device=DEV), cor, run=0)
        rank = round((1.0 - rl.total()) * (V - 1))
        pos = int(np.nonzero(idx[b] == row)[0][0])
        c = int(slot_of[b])
        q = pred[b, c * E:(c + 1) * E].astype(np.float64)
        X = blocks[c][val].astype(np.float64)
        s = X @ q / (np.linalg.norm(q) * np.linalg.norm(X, axis=1))
        own = s[val.index(row)]
        near = int((np.abs(s - own) <= 1e-6).sum()) - 1
        assert abs(pos - (V - 1 - rank)) <= near, (b, pos, V - 1 - rank, near)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_trainer_complete_matches_its_eval_output(hip, precision):
    from golden_util import Golden
    from codae.train import HipEmbeddingTrainer
    from codae.tool import ComplementRetriever
    g = Golden("embedding_square")
    m = g.meta
    S, E = m["S"], m["E"]
    sched = [(w.shape[1], w.shape[0], r) for (w, _), r in zip(g.params("init"), g.relu_flags())]
    tr = HipEmbeddingTrainer(sched, torch.tensor(g["data"]), torch.tensor(g["binary_masks"]).to(torch.uint8),
                             torch.tensor(g["mask_to_use"]).to(torch.int32), m["lr"], m["weight_decay"], clip=1.0,
                             max_batch=m["batch"], precision=precision, device=DEV)
    tr.load_params(g.params("init"))
    for idx, run in g.calls()[:4]:
        tr.train_batch(torch.tensor(idx, dtype=torch.int32, device=DEV), run=run)
    rows = torch.tensor(g["validation_indices"][:48], dtype=torch.int32, device=DEV)
    sums = tr.engine.scalars[:2].clone()
    data = torch.tensor(g["data"])
    inv = types.SimpleNamespace(nb_used_category=S, embedding_size=E,
                                data_per_category={c: data[:, c * E:(c + 1) * E].contiguous() for c in range(S)})
    for c in range(S):
        for exclude_self, distinct in ((False, True), (True, False)):
            idx, sc = tr.complete(rows, c, 10, exclude_self=exclude_self, distinct=distinct)
            # the expected answer: the trainer's own eval forward with slot c blanked, fed to the host retriever
            mid = torch.full((rows.numel(),), c, dtype=torch.int32, device=DEV)
            y = torch.empty((rows.numel(), S * E), dtype=torch.float32, device=DEV)
            tr.engine.eval_step(tr.engine.make_batch(tr.data, rows, mid, tr.mask_table), y)
            hi, hs = ComplementRetriever(inv, "cpu", distinct=distinct).topk(
                y.cpu(), c, 10, exclude=rows.cpu().long() if exclude_self else None)
            same_up_to_ties(idx.cpu().numpy(), sc.cpu().numpy(), hi.numpy(), hs.numpy())
            if exclude_self:
                assert not (idx.cpu() == rows.cpu().long()[:, None]).any()
    tr.engine.scalars[:2].copy_(sums)
    # complete() leaves the metric sums alone, and does not depend on the mask run
    before = tr.engine.scalars.clone()
    a = tr.complete(rows, 1, 5)
    assert torch.equal(tr.engine.scalars, before)
    b = tr.complete(rows, 1, 5)
    assert torch.equal(a[0], b[0])
