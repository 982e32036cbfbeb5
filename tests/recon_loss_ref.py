"""float64 numpy restatement of the training criterion (include/codae_hip.h, "Training criterion"), written from the definition
for the tests: it shares no code with codae.tool.recon_loss or the kernels.  The emphasis weight w comes from
tests/emphasis_ref.py (weights / corrupted), a whole optimizer step from the oracle's forward / backward / clip_grad_norm /
adam_step fed this dy.

  d = x - y, inv_n = 1 / (rows io), w = 1 without emphasis
  mse        rho = d^2                                                 rho' = 2 d
  l1         rho = |d|                                                 rho' = sign(d), sign(0) = 0
  smooth_l1  rho = |d| < beta ? d^2 / (2 beta) : |d| - beta / 2        rho' = d / beta or sign(d)
  huber      rho = |d| <= delta ? d^2 / 2 : delta (|d| - delta / 2)    rho' = d or delta sign(d)
  L = sum w rho inv_n, dL/dy = -w rho' inv_n
  slot_cosine  per (row, slot) over its E columns: dot = sum x y, nx = max(|x|, eps), ny = max(|y|, eps), cos = dot / (nx ny),
             W = mean of w over the slot;  L = sum W (1 - cos) / (rows S) + mse_weight sum w d^2 inv_n
             dL/dy_c = -W / (rows S) (x_c / (nx ny) - [|y| > eps] cos y_c / |y|^2) + mse_weight 2 w (y_c - x_c) inv_n
             with 1 / (rows S) = E inv_n
  the metric sums sum d^2 and sum (1 - fmask) d^2 never change
"""
import numpy as np

import emphasis_ref as ER
import noise_ref as R

EPS = 1e-8
KINDS = ("l1", "smooth_l1", "huber", "slot_cosine")


def _f64(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def rho(kind, d, param=None):
    """(rho(d), rho'(d)) in float64."""
    a = np.abs(d)
    sg = np.sign(d)
    if kind == "mse":
        return d * d, 2.0 * d
    if kind == "l1":
        return a, sg
    p = float(np.float32(param))
    if kind == "smooth_l1":
        q = a < p
        return np.where(q, 0.5 * d * d / p, a - 0.5 * p), np.where(q, d / p, sg)
    if kind == "huber":
        q = a <= p
        return np.where(q, 0.5 * d * d, p * (a - 0.5 * p)), np.where(q, d, p * sg)
    raise ValueError(kind)


def loss_terms(kind, x, y, keep, w, inv_n, param=None, mse_weight=0.0, S=None):
    """Everything one launch of a criterion kernel produces, in float64 from the fp32 inputs: dy [B, io], its column sums, the
    criterion's sum (times inv_n = the loss), the two squared-error sums; for slot_cosine also cos, W, the norms [B, S],
    bound_scale [B, io] = k (|x_c| / (nx ny) + |y_c| / |y|^2), what the fp32 error bound of dy in tests/test_gpu_recon_loss.py
    scales with, and mse_part [B, io], the magnitude of the mse_weight term."""
    with np.errstate(all="ignore"):
        x64, y64 = _f64(x), _f64(y)
        B, io = x64.shape
        w = np.ones((B, io)) if w is None else np.asarray(w, dtype=np.float64)
        inv = np.float64(np.float32(inv_n))
        d = x64 - y64
        se = d * d
        out = dict(sq=float(np.sum(se)), sqp=float(np.sum(se[np.asarray(keep) == 0])))
        if kind != "slot_cosine":
            r, dr = rho(kind, d, param)
            dy = -w * dr * inv
            out.update(dy=dy, crit=float(np.sum(w * r)))
        else:
            E = io // S
            mw = np.float64(np.float32(mse_weight))
            x3, y3, w3 = x64.reshape(B, S, E), y64.reshape(B, S, E), w.reshape(B, S, E)
            dot = (x3 * y3).sum(-1)
            nyr = np.sqrt((y3 * y3).sum(-1))
            nx, ny = np.maximum(np.sqrt((x3 * x3).sum(-1)), EPS), np.maximum(nyr, EPS)
            cos = dot / (nx * ny)
            W = w3.sum(-1) / E
            k = W * (E * inv)
            a = (k / (nx * ny))[:, :, None]
            bq = np.where(nyr > EPS, k * cos / np.where(nyr > EPS, nyr * nyr, 1.0), 0.0)[:, :, None]
            dy = (-(a * x3 - bq * y3)).reshape(B, io) + mw * 2.0 * w * (y64 - x64) * inv
            cos_sum = float(np.sum(W * (1.0 - cos)))
            out.update(dy=dy, crit=float(mw * np.sum(w * se) + E * cos_sum), cos=cos, W=W, nx=nx, ny=ny, nyr=nyr,
                       bound_scale=(k[:, :, None] * (np.abs(x3) / (nx * ny)[:, :, None]
                                                     + np.where(nyr > EPS, 1.0 / np.where(nyr > EPS, nyr * nyr, 1.0), 0.0)[:, :, None] * np.abs(y3))
                                    ).reshape(B, io), mse_part=np.abs(mw * 2.0 * w * d * inv))
        out.update(colsum=out["dy"].sum(axis=0), colsum_abs=np.abs(out["dy"]).sum(axis=0), loss=out["crit"] * float(inv))
        return out


class CriterionOracle:
    """emphasis_ref.EmphasisOracle's step with the criterion's dy: the input is the reference-noised and blanked row, the target
    the clean row.  alpha = beta = 1 and col_weight None: no emphasis."""

    def __init__(self, params, relu_flags, lr, weight_decay, kind, param=None, mse_weight=0.0, S=None, alpha=1.0, beta=1.0,
                 col_weight=None, noise=None, quant=None):
        from oracle import dae_oracle as O
        self.O = O
        self.params = [(w.astype(np.float32).copy(), b.astype(np.float32).copy()) for w, b in params]
        self.relu, self.lr, self.wd, self.quant = list(relu_flags), lr, weight_decay, quant
        self.kind, self.param, self.mse_weight, self.S = kind, param, mse_weight, S
        self.alpha, self.beta, self.col_weight, self.noise = alpha, beta, col_weight, noise
        self.adam = O.adam_init(self.params)
        self.last_grads = None
        self.steps = 0

    def step(self, x, rows, fmask, global_rows=None):
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
        t = loss_terms(self.kind, x, y, fmask, w, 1.0 / (float(n_rows) * x.shape[1]), self.param, self.mse_weight, self.S)
        grads = O.backward(self.params, self.relu, acts, t["dy"].astype(np.float32), quant=self.quant)
        self.last_grads = grads
        clipped, gnorm = O.clip_grad_norm(grads, 1.0)
        self.params = O.adam_step(self.params, clipped, self.adam, self.lr, self.wd)
        return {"loss": t["loss"], "grad_norm": float(gnorm), "sq_full": t["sq"], "sq_partial": t["sqp"],
                "mse": t["sq"] / (float(n_rows) * x.shape[1]), "min_abs_d": float(np.abs(x.astype(np.float64) - y).min())}
