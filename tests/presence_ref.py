"""float64 numpy statement of per-row slot presence (include/codae_hip.h, "Slot presence"), built on the statements the other
definitions already have - emphasis_ref (weights, corrupted), recon_loss_ref (every criterion's terms), contrast_ref (the pair
terms and the candidate draw), noise_ref (the gather) - by import: presence only SELECTS what those see.

  present [N, S] uint8, keyed by the DATASET row;  pm [B, io] = present[rows] repeated over each slot's E columns
  gather      where(pm, blank(noise(x)), 0)
  loss        the criterion's terms of (where(pm, x, 0), where(pm, y, 0)) under the weight where(pm, w, 0): an absent element has
              d = 0 and weight 0, so its term is 0 whatever x and y hold (a NaN included), and an absent pair of slot_cosine has
              W = 0; dy is then SET to +0 there
  sums        sum d^2 over present elements, over present and blanked elements
  contrast    an absent pair has x = 0: no positive.  An absent candidate is left out of every pair: contrast_ref leaves out by
              identity, so each batch row is scored with an id table in which every row that lacks the slot carries the batch
              row's own id (the data handed over has zeros in absent slots, so nothing non-finite is multiplied by p = 0)
"""
import numpy as np

import contrast_ref as CR
import emphasis_ref as ER
import noise_ref as R
import recon_loss_ref as RR

SEED = 20261019


def make_table(N, S, seed=SEED, p_absent=0.3, min_keep=2):
    """uint8 [N, S], about 30 % absent, repaired so that every row keeps at least `min_keep` present slots, with row 0 complete.
    (min_keep = 2 is what training needs: one slot to blank, one to see.  The S = 2 kernel fixtures pass 1: two of two would be
    a table without an absence.)"""
    rng = np.random.default_rng(seed + 1000 * S + N)
    t = (rng.random((N, S)) >= p_absent).astype(np.uint8)
    for r in range(N):
        while t[r].sum() < min_keep:
            t[r, rng.integers(0, S)] = 1
    t[0] = 1
    return t


def pmask(present, rows, E):
    """bool [B, S * E]"""
    return np.repeat(np.asarray(present)[np.asarray(rows, dtype=np.int64)] != 0, E, axis=1)


def gather(x, rows, keep, present, step=0, noise=None):
    """What the gather writes for clean rows x [B, io] (dataset rows `rows`), keep [B, io] (0 = blanked) or None, noise None or
    (kind, kwargs, seed).  float32 for no noise / masking / salt_pepper (exact); gaussian: (float64 values, float64 scale)."""
    x = np.asarray(x, dtype=np.float32)
    B, io = x.shape
    pm = pmask(present, rows, io // np.asarray(present).shape[1])
    xs = np.where(pm, x, np.float32(0))                  # (what is under an absent slot is never used: not even by the noise)
    if noise is None:
        out = xs if keep is None else np.where(np.asarray(keep) != 0, xs, np.float32(0))
        return np.where(pm, out, np.float32(0)).astype(np.float32)
    kind, kw, seed = noise
    out = R.corrupt(xs, rows, step, kind, seed=seed, keep=keep, **kw)
    if kind == "gaussian":
        return np.where(pm, out[0], 0.0), np.where(pm, out[1], 0.0)
    return np.where(pm, out, np.float32(0)).astype(np.float32)


def loss_terms(kind, x, y, keep, w, inv_n, present, rows, param=None, mse_weight=0.0, S=None):
    """recon_loss_ref.loss_terms (kind "mse" included) under the presence rule.  -> its dict, with dy exactly +0 in absent
    elements, `pm`, and for kind "mse" also `wsum` (= crit), emphasis_ref's name for the weighted sum."""
    x = np.asarray(x, dtype=np.float32)
    y = np.asarray(y, dtype=np.float32)
    B, io = x.shape
    pm = pmask(present, rows, io // np.asarray(present).shape[1])
    w = np.ones((B, io)) if w is None else np.asarray(w, dtype=np.float64)
    keep = np.ones((B, io), np.uint8) if keep is None else np.asarray(keep)
    xs, ys, ws = np.where(pm, x, np.float32(0)), np.where(pm, y, np.float32(0)), np.where(pm, w, 0.0)
    t = RR.loss_terms(kind, xs, ys, keep, ws, inv_n, param, mse_weight, S)
    dy = np.where(pm, t["dy"], 0.0)
    t.update(dy=dy, colsum=dy.sum(axis=0), colsum_abs=np.abs(dy).sum(axis=0), pm=pm)
    if kind == "mse":
        t["wsum"] = t["crit"]
    return t


def contrast_terms(data, present, x, y, rows, step, S, K, tau, scale, seed, W=None, item_id=None, pool=None, dy_in=None):
    """contrast_ref.terms under the presence rule -> dict(dy [B, io], own, parts [blocks], loss, l [B, S], left_out [B, S, K],
    cand [S, K], plus the bound scales k, ny, bs, bsn, yh, W of contrast_ref for the rows as a batch)."""
    data = np.asarray(data, dtype=np.float32)
    present = np.asarray(present)
    rows = np.asarray(rows, dtype=np.int64)
    N, io = data.shape
    E = io // S
    B = len(rows)
    data0 = np.where(np.repeat(present != 0, E, axis=1), data, np.float32(0))
    x0 = np.where(pmask(present, rows, E), np.asarray(x, dtype=np.float32), np.float32(0))
    base = np.tile(np.arange(N, dtype=np.int64), (S, 1)) if item_id is None else np.asarray(item_id, dtype=np.int64)
    W = np.ones((B, S)) if W is None else np.asarray(W, dtype=np.float64)
    dy_in = np.zeros((B, io)) if dy_in is None else np.asarray(dy_in, dtype=np.float64)
    keys = ("dy", "own", "l", "left_out", "k", "ny", "bs", "bsn", "yh", "W")
    per = {k: [] for k in keys}
    cand = None
    for b in range(B):
        ids = base.copy()
        for s in range(S):
            ids[s, present[:, s] == 0] = base[s, rows[b]]          # rows that lack slot s: "the same item" as this batch row's
        t = CR.terms(data0, x0[b:b + 1], np.asarray(y)[b:b + 1], rows[b:b + 1], step, S, K, tau, scale, seed, W=W[b:b + 1], item_id=ids,
                     pool=pool, dy_in=dy_in[b:b + 1])
        for k in keys:
            per[k].append(t[k])
        cand = t["cand"]
    out = {k: np.concatenate(per[k], axis=0) for k in keys}
    with np.errstate(all="ignore"):
        Wl = np.where(np.isnan(out["l"]), np.nan, out["W"] * out["l"])
        blocks = (B + CR.BLOCK - 1) // CR.BLOCK
        out["parts"] = np.array([Wl[i * CR.BLOCK:(i + 1) * CR.BLOCK].sum() for i in range(blocks)])
        out["colsum"] = np.stack([out["dy"][i * CR.BLOCK:(i + 1) * CR.BLOCK].sum(axis=0) for i in range(blocks)])
        out["loss"] = float(np.float64(np.float32(scale)) * Wl.sum())
    out["cand"] = cand
    out["absent_cand"] = np.stack([present[cand[s], s] == 0 for s in range(S)])        # [S, K]
    return out


class PresenceOracle:
    """recon_loss_ref.CriterionOracle's step under a presence table, optionally with the slot contrast on top: the input is the
    presence-aware gather, dy and the sums come from loss_terms / contrast_terms above, everything else is the oracle's."""

    def __init__(self, params, relu_flags, lr, weight_decay, present, data=None, kind="mse", param=None, mse_weight=0.0, S=None,
                 alpha=1.0, beta=1.0, col_weight=None, noise=None, quant=None, contrast=None):
        """contrast: None or dict(K=, tau=, weight=, seed=, item_id=None, pool=None); data: the whole dataset (contrast only)."""
        from oracle import dae_oracle as O
        self.O = O
        self.params = [(w.astype(np.float32).copy(), b.astype(np.float32).copy()) for w, b in params]
        self.relu, self.lr, self.wd, self.quant = list(relu_flags), lr, weight_decay, quant
        self.present, self.data = np.asarray(present), data
        self.kind, self.param, self.mse_weight, self.S = kind, param, mse_weight, S
        self.alpha, self.beta, self.col_weight, self.noise, self.contrast = alpha, beta, col_weight, noise, contrast
        self.adam = O.adam_init(self.params)
        self.last_grads = None
        self.last_dy = None
        self.steps = 0

    def step(self, x, rows, fmask, global_rows=None):
        O = self.O
        self.steps += 1
        x = np.asarray(x, dtype=np.float32)
        B, io = x.shape
        c = gather(x, rows, fmask, self.present, self.steps, self.noise)
        if self.noise is not None and self.noise[0] == "gaussian":
            c = c[0]
        c = np.asarray(c, dtype=np.float32)
        y, acts = O.forward(self.params, self.relu, c, keep=True, quant=self.quant)
        w = ER.weights(ER.corrupted(fmask, rows, self.steps, self.noise), self.alpha, self.beta, self.col_weight)
        n_rows = B if global_rows is None else global_rows
        t = loss_terms(self.kind, x, y, fmask, w, 1.0 / (float(n_rows) * io), self.present, rows, self.param, self.mse_weight, self.S)
        dy, loss = t["dy"], t["loss"]
        if self.contrast is not None:
            cc = self.contrast
            S = self.S
            Wp = np.where(t["pm"], w, 0.0).reshape(B, S, io // S).mean(-1)
            scale = np.float32(np.float64(np.float32(cc["weight"])) / (float(n_rows) * S))
            ct = contrast_terms(self.data, self.present, x, y, rows, self.steps, S, cc["K"], cc["tau"], scale, cc["seed"], W=Wp,
                                item_id=cc.get("item_id"), pool=cc.get("pool"), dy_in=dy)
            dy, loss = ct["dy"], loss + ct["loss"]
        self.last_dy = dy
        grads = O.backward(self.params, self.relu, acts, dy.astype(np.float32), quant=self.quant)
        self.last_grads = grads
        clipped, gnorm = O.clip_grad_norm(grads, 1.0)
        self.params = O.adam_step(self.params, clipped, self.adam, self.lr, self.wd)
        return {"loss": loss, "grad_norm": float(gnorm), "sq_full": t["sq"], "sq_partial": t["sqp"], "y": y}


def eval_sums(params, relu_flags, x, rows, fmask, present, quant=None):
    """(sum d^2 over present, over present and blanked, y) of an evaluation step."""
    from oracle import dae_oracle as O
    x = np.asarray(x, dtype=np.float32)
    c = gather(x, rows, fmask, present)
    y, _ = O.forward([(w.astype(np.float32), b.astype(np.float32)) for w, b in params], list(relu_flags), c, keep=True, quant=quant)
    t = loss_terms("mse", x, y, fmask, None, 1.0, present, rows)
    return t["sq"], t["sqp"], y
