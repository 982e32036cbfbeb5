"""Reference for the retrieval metrics (include/codae_hip.h, "Retrieval metrics"): a plain numpy loop over the definition, one
query pair at a time, evaluated in the floating-point type it is given (float64 or float32) - and the two designs the host and
GPU tests share (an exact one whose cosine ORDER does not depend on the summation order, and a gaussian one)."""
import numpy as np

PAIRS, RRE, RR, HIT, MAX_KS, HIST, STRIDE = 0, 1, 2, 3, 8, 16, 48


def items_of_slot(X, rows, distinct):
    """(first [n_items] dataset rows ascending, item_of [N] item position or -1): candidates `rows` of inventory X [N, E] with
    identical BYTES folded into one item, represented by its lowest row."""
    item_of = np.full(X.shape[0], -1, dtype=np.int64)
    first, seen = [], {}
    for r in sorted(set(int(r) for r in rows)):
        key = X[r].astype(np.float32).tobytes() if distinct else r
        if key not in seen:
            seen[key] = len(first)
            first.append(r)
        item_of[r] = seen[key]
    return np.asarray(first, dtype=np.int64), item_of


def reference(inv, val, presence, distinct, mask_table, mask_ids, idx, pred, ks, dtype):
    """inv [S, N, E], val: validation rows, presence uint8 [N, S] or None, mask_table [n_masks, S*E] (0 = blanked), mask_ids [B],
    idx [B] dataset rows, pred [B, S*E].  Returns (sums float64 [S, STRIDE], pairs: list of (b, c, p, n))."""
    S, N, E = inv.shape
    T = np.dtype(dtype).type
    inv, pred = inv.astype(dtype), pred.astype(dtype)
    sums = np.zeros((S, STRIDE), dtype=np.float64)
    out = []
    eps = T(1e-8)
    for c in range(S):
        rows = [r for r in val if presence is None or presence[r, c]]
        first, item_of = items_of_slot(inv[c], rows, distinct)
        V = inv[c][first] if len(first) else np.zeros((0, E), dtype=dtype)
        vn = np.maximum(np.sqrt((V * V).sum(axis=1, dtype=dtype)), eps)
        for b in range(len(idx)):
            r = int(idx[b])
            if mask_table[int(mask_ids[b]), c * E] != 0 or (presence is not None and not presence[r, c]):
                continue
            keep = np.ones(len(first), dtype=bool)
            if item_of[r] >= 0:
                keep[item_of[r]] = False
            n = int(keep.sum())
            if n < 1:
                continue
            q = pred[b, c * E:(c + 1) * E]
            qn = max(np.sqrt((q * q).sum(dtype=dtype)), eps)
            o = inv[c][r]
            with np.errstate(invalid="ignore"):
                own = (q * o).sum(dtype=dtype) / (qn * max(np.sqrt((o * o).sum(dtype=dtype)), eps))
                s = (V @ q) / (qn * vn)
                beaten = int((own > s[keep]).sum())                 # (a NaN on either side compares False)
            p = 1 + n - beaten
            out.append((b, c, p, n))
            sums[c, PAIRS] += 1
            sums[c, RRE] += (p - 1) / n
            sums[c, RR] += 1.0 / p
            for i, k in enumerate(ks):
                sums[c, HIT + i] += p <= k
            sums[c, HIST + int(np.floor(np.log2(p)))] += 1
    return sums, out


def mask_table_for(S, E, nb_missing):
    """uint8 [n_masks, S*E]: the 1-subsets {c} in slot order, then (nb_missing = 2) the 2-subsets."""
    subsets = [(c,) for c in range(S)]
    if nb_missing == 2:
        subsets += [(a, b) for a in range(S) for b in range(a + 1, S)]
    t = np.ones((len(subsets), S * E), dtype=np.uint8)
    for i, sub in enumerate(subsets):
        for c in sub:
            t[i, c * E:(c + 1) * E] = 0
    return t


class Dataset:
    """what RankingLoss / ComplementRetriever / RetrievalMetrics read of a dataset"""

    def __init__(self, inv):
        import torch
        S, N, E = inv.shape
        self.nb_used_category, self.embedding_size, self.nb_predictor = S, E, S * E
        self.data_per_category = {c: torch.tensor(inv[c]) for c in range(S)}


def exact_design(nb_missing=1, nan_row=True):
    """S = 3, E = 8, N = 96, V = 53, B = 37.  Inventory rows: exactly four entries of +-1 (every norm exactly 2, every dot product
    a small integer); rows 48..95 of slot 1 copy rows 0..47; presence drawn at 75 %; predictions integers in [-2, 2]; one prediction
    row NaN; the last batch row is no validation row.  Equal dot products give equal cosines in any precision and summation order, and
    unequal ones differ by far more than rounding: the positions are exact, ties and all."""
    S, E, N, V, B = 3, 8, 96, 53, 37
    rng = np.random.default_rng(7)
    inv = np.zeros((S, N, E), dtype=np.float32)
    for c in range(S):
        for r in range(N):
            inv[c, r, rng.permutation(E)[:4]] = rng.choice([-1.0, 1.0], 4)
    inv[1, 48:] = inv[1, :48]
    presence = (rng.random((N, S)) < 0.75).astype(np.uint8)
    perm = rng.permutation(N)
    val = sorted(int(v) for v in perm[:V])
    idx = np.concatenate([rng.permutation(val)[:B - 1], perm[V:V + 1]]).astype(np.int32)
    pred = rng.integers(-2, 3, (B, S * E)).astype(np.float32)
    if nan_row:
        pred[5] = np.nan
        presence[idx[5]] = 1                     # (the NaN row has every slot: whatever its mask blanks is a pair)
    table = mask_table_for(S, E, nb_missing)
    mask_to_use = rng.integers(0, len(table), (N, 2)).astype(np.int32)
    return dict(S=S, E=E, N=N, V=V, B=B, inv=inv, presence=presence, val=val, idx=idx, pred=pred, table=table, mask_to_use=mask_to_use)


def gaussian_design(S=3, E=64, N=3000, V=700, B=500, seed=7, signal=(0.0, 0.2, 0.4, 0.8)):
    """Gaussian inventory without duplicates, complete rows, one blanked slot per row, every batch row a validation row.  The
    prediction of row b is signal[b % len] times its own row plus unit noise, so that the positions spread from 1 to mid-field."""
    rng = np.random.default_rng(seed)
    inv = rng.standard_normal((S, N, E)).astype(np.float32)
    val = sorted(int(v) for v in rng.permutation(N)[:V])
    idx = rng.permutation(val)[:B].astype(np.int32)
    own = np.concatenate([inv[c][idx] for c in range(S)], axis=1)
    pred = (np.asarray(signal, dtype=np.float32)[np.arange(B) % len(signal)][:, None] * own
            + rng.standard_normal((B, S * E)).astype(np.float32)).astype(np.float32)
    table = mask_table_for(S, E, 1)
    mask_to_use = rng.integers(0, S, (N, 2)).astype(np.int32)
    return dict(S=S, E=E, N=N, V=V, B=B, inv=inv, presence=None, val=val, idx=idx, pred=pred, table=table, mask_to_use=mask_to_use)
