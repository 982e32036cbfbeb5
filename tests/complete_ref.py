"""float64 numpy brute force of complementarity inference (codae.tool.ComplementRetriever) and the checks the
test files share."""
import numpy as np


def ref_ranked(pred, slots, inv, E, k, candidates=None, distinct=True, exclude=None):
    """Per query row: (ids, s64) of EVERY valid candidate, score descending then id ascending, float64 cosine.
    inv: {slot: [n_obs, E] array}."""
    out = []
    n_obs = inv[0].shape[0]
    rows = np.arange(n_obs) if candidates is None else np.unique(np.asarray(candidates, dtype=np.int64))
    items = {}
    for c in set(int(s) for s in slots):
        X = np.asarray(inv[c], dtype=np.float32)
        if distinct:
            first, item_of = {}, {}
            for r in rows:
                key = X[r].tobytes()
                first.setdefault(key, r)
                item_of[r] = first[key]
            reps = np.array(sorted(set(first.values())), dtype=np.int64)
        else:
            item_of = {r: r for r in rows}
            reps = rows
        items[c] = (reps, item_of)
    for b, c in enumerate(slots):
        c = int(c)
        reps, item_of = items[c]
        q = np.asarray(pred[b, c * E:(c + 1) * E], dtype=np.float64)
        V = np.asarray(inv[c], dtype=np.float64)[reps]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            s = (V @ q) / (max(np.linalg.norm(q), 1e-8) * np.maximum(np.linalg.norm(V, axis=1), 1e-8))
        ok = ~np.isnan(s)
        if exclude is not None and int(exclude[b]) in item_of:
            ok &= reps != item_of[int(exclude[b])]
        ids, s = reps[ok], s[ok]
        o = np.lexsort((ids, -s))
        out.append((ids[o], s[o]))
    return out


def check_topk(idx, score, ranked, k, tol=1e-5):
    """idx / score [B, k] against ranked (ref_ranked): scores within tol of float64, the returned set = the float64 top-k
    except items within tol of the k-th score, contract order (score descending, equal scores by ascending id), the
    (-1, -inf) tail exactly where fewer than k candidates exist."""
    idx = np.asarray(idx)
    score = np.asarray(score)
    assert idx.shape == score.shape == (len(ranked), k)
    for b, (ids, s64) in enumerate(ranked):
        kk = min(k, len(ids))
        got, gs = idx[b, :kk], score[b, :kk]
        assert (idx[b, kk:] == -1).all() and np.isneginf(score[b, kk:]).all(), (b, idx[b], score[b])
        assert (got >= 0).all() and len(set(got.tolist())) == kk, (b, got)
        if kk == 0:
            continue
        lookup = dict(zip(ids.tolist(), s64.tolist()))
        assert all(g in lookup for g in got.tolist()), (b, got)
        ref_s = np.array([lookup[g] for g in got.tolist()])
        finite = np.isfinite(ref_s)
        assert np.all(np.abs(gs[finite] - ref_s[finite]) <= tol), (b, np.abs(gs - ref_s).max())
        assert np.array_equal(np.isfinite(gs), finite), b
        thr = s64[kk - 1]
        must = set(ids[s64 > thr + tol].tolist())
        assert must <= set(got.tolist()), (b, must - set(got.tolist()))
        assert (ref_s >= thr - tol).all(), b
        for i in range(kk - 1):
            assert gs[i] > gs[i + 1] or (gs[i] == gs[i + 1] and got[i] < got[i + 1]), (b, i, gs[i:i + 2], got[i:i + 2])
