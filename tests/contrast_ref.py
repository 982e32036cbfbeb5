"""float64 numpy restatement of the slot contrast (include/codae_hip.h, "Slot contrast"), written from the definition for the
tests: it shares no code with codae.tool.contrast or the kernels.  Philox comes from tests/noise_ref.py.

  candidates  step t, slot s, k in 0 .. K-1: r = word k % 4 of Philox(counter (k // 4, s, t, 256), key (seed lo, seed hi)),
              j = (r * P) >> 32, row_k = pool[j] (or j), c_k = slot s of data[row_k]
  left out    item_id[s][row_k] == item_id[s][row_b]  (item_id None: row_k == row_b)
  pair        z_0 = x^ . y^ / tau, z_k = c_k^ . y^ / tau; l = logsumexp(z_0, z_kept) - z_0; p = softmax
              g = sum_kept p_k c_k^ - (1 - p_0) x^;  dl/dy = [|y| > eps] (g - (g . y^) y^) / (tau |y|)
              |x| <= eps: l = 0, dl = 0;  a NaN / Inf in the y slot: l = NaN, dy = NaN (whatever else holds)
  dy          dy_in + scale W dl, scale = weight / (rows S) as the fp32 value handed to the kernel
  parts       per block of 32 batch rows: sum W l
tau and scale are the fp32 values the C side carries; everything else is float64 from the fp32 inputs.
"""
import numpy as np

import noise_ref as R

EPS = 1e-8
BLOCK = 32


def candidate_rows(step, slot, K, seed, n_rows, pool=None):
    """int64 [K] dataset rows of the candidates of (step, slot)."""
    k = np.arange(K)
    w = R.philox((k // 4, slot, step, 256), (seed & R.MASK32, seed >> 32))
    r = np.stack(w, axis=-1)[k, k % 4].astype(np.uint64)
    P = len(pool) if pool is not None else n_rows
    j = ((r * np.uint64(P)) >> np.uint64(32)).astype(np.int64)
    return j if pool is None else np.asarray(pool, dtype=np.int64)[j]


def item_ids(data, S):
    """int64 [S, N]: index of every row's slot among the slot's distinct embeddings (np.unique over rows)."""
    N, io = data.shape
    E = io // S
    return np.stack([np.unique(data[:, s * E:(s + 1) * E], axis=0, return_inverse=True)[1].reshape(-1) for s in range(S)])


def _unit(v):
    n = np.sqrt((v * v).sum(axis=-1, keepdims=True))
    return v / np.maximum(n, EPS), n[..., 0]


def terms(data, x, y, rows, step, S, K, tau, scale, seed, W=None, item_id=None, pool=None, dy_in=None):
    """data [N, io] the dataset; x [B, io] the clean batch rows (data[rows]); y [B, io]; rows [B] dataset rows; W [B, S] or None (1);
    item_id [S, N] or None; dy_in [B, io] (what the criterion left; default 0).
    -> dict: dy, colsum, colsum_abs (of the contrast's own contribution, plus |dy_in|), parts [blocks], loss (scale * sum W l),
       l [B, S], left_out [B, S, K] bool, cand [S, K] rows, k [B, S] = scale W, ny [B, S],
       bs [B, io] = sum_kept p_k (|c_k^| + |x^|) per column and bsn [B, S] its 2-norm over the slot, yh [B, io] = |y^|
       (the scales of the fp32 error bound in tests/test_gpu_slot_contrast.py)."""
    data64 = np.asarray(data, dtype=np.float32).astype(np.float64)
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    y64 = np.asarray(y).astype(np.float64)       # (fp32 from the tests; a float64 y is taken as it is: the finite difference)
    rows = np.asarray(rows, dtype=np.int64)
    B, io = x64.shape
    N = data64.shape[0]
    E = io // S
    tau = np.float64(np.float32(tau))
    scale = np.float64(np.float32(scale))
    W = np.ones((B, S)) if W is None else np.asarray(W, dtype=np.float64)
    dy = np.zeros((B, io)) if dy_in is None else np.asarray(dy_in, dtype=np.float64).copy()
    own = np.zeros((B, io))
    l_all = np.zeros((B, S))
    left = np.zeros((B, S, K), dtype=bool)
    cand = np.zeros((S, K), dtype=np.int64)
    ny_all = np.zeros((B, S))
    bs = np.zeros((B, io))
    bsn = np.zeros((B, S))
    yh_abs = np.zeros((B, io))
    with np.errstate(all="ignore"):
        for s in range(S):
            sl = slice(s * E, (s + 1) * E)
            ck = candidate_rows(step, s, K, seed, N, pool)
            cand[s] = ck
            ch, _ = _unit(data64[ck, sl])                                           # [K, E]
            xh, nx = _unit(x64[:, sl])
            yh, ny = _unit(y64[:, sl])
            ny_all[:, s] = ny
            yh_abs[:, sl] = np.abs(yh)
            if item_id is not None:
                out = item_id[s][ck][None, :] == item_id[s][rows][:, None]
            else:
                out = ck[None, :] == rows[:, None]
            left[:, s] = out
            z0 = (xh * yh).sum(axis=-1) / tau                                       # [B]
            z = (yh @ ch.T) / tau                                                   # [B, K]
            z = np.where(out, -np.inf, z)
            m = np.maximum(z0, z.max(axis=1))
            tot = np.exp(z0 - m) + np.exp(z - m[:, None]).sum(axis=1)
            lse = m + np.log(tot)
            l = lse - z0
            p0 = np.exp(z0 - lse)
            p = np.exp(z - lse[:, None])                                            # [B, K], 0 where left out
            g = p @ ch - (1.0 - p0)[:, None] * xh
            gy = (g * yh).sum(axis=-1)
            live = (ny > EPS)[:, None]
            dl = np.where(live, (g - gy[:, None] * yh) / (tau * np.maximum(ny, 1e-300))[:, None], 0.0)
            nopos = ~(nx > EPS)
            l = np.where(nopos, 0.0, l)
            dl = np.where(nopos[:, None], 0.0, dl)
            bad = ~np.isfinite(y64[:, sl]).all(axis=1)
            l = np.where(bad, np.nan, l)
            dl = np.where(bad[:, None], np.nan, dl)
            k = scale * W[:, s]
            c = k[:, None] * dl
            c = np.where(bad[:, None], np.nan, c)                                   # (under W = 0 too)
            own[:, sl] = c
            dy[:, sl] = dy[:, sl] + c
            l_all[:, s] = l
            b = p @ np.abs(ch) + (1.0 - p0)[:, None] * np.abs(xh)
            b = np.where(nopos[:, None], 0.0, b)
            bs[:, sl] = b
            bsn[:, s] = np.sqrt((b * b).sum(axis=-1))
        Wl = np.where(np.isnan(l_all), np.nan, W * l_all)
        blocks = (B + BLOCK - 1) // BLOCK
        parts = np.array([Wl[i * BLOCK:(i + 1) * BLOCK].sum() for i in range(blocks)])
        colsum = np.stack([dy[i * BLOCK:(i + 1) * BLOCK].sum(axis=0) for i in range(blocks)])
    return dict(dy=dy, own=own, colsum=colsum, colsum_abs=np.abs(dy).sum(axis=0), parts=parts, loss=float(scale * Wl.sum()), l=l_all,
                left_out=left, cand=cand, k=scale * W, ny=ny_all, bs=bs, bsn=bsn, yh=yh_abs, W=W)


def loss_value(data, x, y, rows, step, S, K, tau, scale, seed, W=None, item_id=None, pool=None):
    return terms(data, x, y, rows, step, S, K, tau, scale, seed, W, item_id, pool)["loss"]


class ContrastOracle:
    """recon_loss_ref.CriterionOracle's step with the slot contrast on top: dy = the criterion's dy + the term's, loss = the sum.
    data: the whole dataset the candidates are drawn from; item_id [S, N] or None; emphasis / noise as CriterionOracle."""

    def __init__(self, params, relu_flags, lr, weight_decay, data, S, K, tau, weight, seed, item_id=None, pool=None, kind="mse", param=None,
                 mse_weight=0.0, alpha=1.0, beta=1.0, col_weight=None, noise=None, quant=None):
        from oracle import dae_oracle as O
        self.O = O
        self.params = [(w.astype(np.float32).copy(), b.astype(np.float32).copy()) for w, b in params]
        self.relu, self.lr, self.wd, self.quant = list(relu_flags), lr, weight_decay, quant
        self.data, self.S, self.K, self.tau, self.weight, self.seed, self.item_id, self.pool = data, S, K, tau, weight, seed, item_id, pool
        self.kind, self.param, self.mse_weight = kind, param, mse_weight
        self.alpha, self.beta, self.col_weight, self.noise = alpha, beta, col_weight, noise
        self.adam = O.adam_init(self.params)
        self.last_grads = None
        self.last_terms = None
        self.steps = 0

    def step(self, x, rows, fmask, global_rows=None, update=True):
        import emphasis_ref as ER
        import recon_loss_ref as RR
        O = self.O
        self.steps += 1
        x = np.asarray(x, dtype=np.float32)
        c = x * fmask
        if self.noise is not None:
            kind, kw, seed = self.noise
            c = R.corrupt(x, rows, self.steps, kind, seed=seed, keep=fmask, **kw)
            if kind == "gaussian":
                c = c[0]
        c = np.asarray(c, dtype=np.float32)
        y, acts = O.forward(self.params, self.relu, c, keep=True, quant=self.quant)
        w = ER.weights(ER.corrupted(fmask, rows, self.steps, self.noise), self.alpha, self.beta, self.col_weight)
        n_rows = len(x) if global_rows is None else global_rows
        io = x.shape[1]
        t = RR.loss_terms(self.kind, x, y, fmask, w, 1.0 / (float(n_rows) * io), self.param, self.mse_weight, self.S)
        W = w.reshape(len(x), self.S, io // self.S).mean(-1)
        scale = np.float32(np.float64(np.float32(self.weight)) / (float(n_rows) * self.S))
        ct = terms(self.data, x, y, rows, self.steps, self.S, self.K, self.tau, scale, self.seed, W=W, item_id=self.item_id, pool=self.pool,
                   dy_in=t["dy"])
        self.last_terms = ct
        grads = O.backward(self.params, self.relu, acts, ct["dy"].astype(np.float32), quant=self.quant)
        self.last_grads = grads
        clipped, gnorm = O.clip_grad_norm(grads, 1.0)
        if update:
            self.params = O.adam_step(self.params, clipped, self.adam, self.lr, self.wd)
        return {"loss": t["loss"] + ct["loss"], "criterion": t["loss"], "contrast": ct["loss"], "grad_norm": float(gnorm),
                "sq_full": t["sq"], "sq_partial": t["sqp"]}
