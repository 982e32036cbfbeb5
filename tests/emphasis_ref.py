"""float64 numpy restatement of the emphasised denoising loss (include/codae_hip.h, "Emphasised denoising loss"), written from
the definition for the tests: it shares no code with codae.tool.emphasis or the kernels.  `replaced` comes from
tests/noise_ref.py (words, threshold), a whole optimizer step from the oracle's forward / backward / clip_grad_norm /
adam_step with the weighted dy.

  blank      keep == 0 (the row's mask blanks the column)
  replaced   MASKING / SALT_PEPPER: word < T; GAUSSIAN and no noise: nothing
  corrupted  blank or replaced
  w          col_weight[c] * (alpha if corrupted else beta)      (alpha, beta, col_weight: the fp32 values the C struct carries)
  L          sum w (x - y)^2 * inv_n;   dL/dy = 2 w (y - x) inv_n
  the metric sums sum (x - y)^2 and sum (1 - fmask)(x - y)^2 stay unweighted
"""
import numpy as np

import noise_ref as R

SEED = 0x0123456789ABCDEF


def replaced(rows, io, step, noise):
    """bool [B, io]; noise: None or (kind, dict(p=.., ..), seed)."""
    rows = np.asarray(rows)
    if noise is None or noise[0] not in ("masking", "salt_pepper"):
        return np.zeros((len(rows), io), dtype=bool)
    kind, kw, seed = noise
    return R.words(rows, io, step, seed).astype(np.uint64) < np.uint64(R.threshold(kw["p"]))


def corrupted(keep, rows, step, noise):
    keep = np.asarray(keep)
    return (keep == 0) | replaced(rows, keep.shape[1], step, noise)


def weights(corr, alpha, beta, col_weight=None):
    """float64 [B, io] from the fp32 parameters."""
    w = np.where(corr, np.float64(np.float32(alpha)), np.float64(np.float32(beta)))
    if col_weight is not None:
        w = w * np.asarray(col_weight, dtype=np.float32).astype(np.float64)[None, :]
    return w


def loss_terms(x, y, keep, w, inv_n):
    """Everything one launch of the loss kernel produces, in float64 from the fp32 inputs: dy [B, io], its column sums, the
    three sums, and the loss."""
    with np.errstate(all="ignore"):
        x64, y64 = np.asarray(x, dtype=np.float32).astype(np.float64), np.asarray(y, dtype=np.float32).astype(np.float64)
        inv = np.float64(np.float32(inv_n))
        se = (x64 - y64) ** 2
        dy = 2.0 * w * (y64 - x64) * inv
        wsum = float(np.sum(w * se))
        return dict(dy=dy, colsum=dy.sum(axis=0), colsum_abs=np.abs(dy).sum(axis=0), wsum=wsum, sq=float(np.sum(se)),
                    sqp=float(np.sum(se[np.asarray(keep) == 0])), loss=wsum * float(inv))


class EmphasisOracle:
    """oracle.EmbeddingTrainer.step composed from the oracle's public functions with the weighted loss: the input is the
    reference-noised and blanked row, the target the clean row, dy = 2 w (y - x) / (rows * io)."""

    def __init__(self, params, relu_flags, lr, weight_decay, alpha, beta, col_weight=None, noise=None, quant=None):
        from oracle import dae_oracle as O
        self.O = O
        self.params = [(w.astype(np.float32).copy(), b.astype(np.float32).copy()) for w, b in params]
        self.relu, self.lr, self.wd, self.quant = list(relu_flags), lr, weight_decay, quant
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
        w = weights(corrupted(fmask, rows, self.steps, self.noise), self.alpha, self.beta, self.col_weight)
        n_rows = len(x) if global_rows is None else global_rows
        t = loss_terms(x, y, fmask, w, 1.0 / (float(n_rows) * x.shape[1]))
        grads = O.backward(self.params, self.relu, acts, t["dy"].astype(np.float32), quant=self.quant)
        self.last_grads = grads
        clipped, gnorm = O.clip_grad_norm(grads, 1.0)
        self.params = O.adam_step(self.params, clipped, self.adam, self.lr, self.wd)
        return {"loss": t["loss"], "grad_norm": float(gnorm), "sq_full": t["sq"], "sq_partial": t["sqp"],
                "unweighted_loss": t["sq"] / (float(n_rows) * x.shape[1])}


def problem(io, S=3, N=120, B=33, seed=0):
    """The shared kernel-level fixture: N dataset rows, B batch rows (two 32-row blocks, the second with one live row), S
    one-slot masks, a mask_to_use table of 3 runs, a prediction y."""
    rng = np.random.default_rng(7000 + io + seed)
    E = io // S
    data = rng.standard_normal((N, io)).astype(np.float32)
    table = np.ones((S, io), dtype=np.uint8)
    for s in range(S):
        table[s, s * E:(s + 1) * E] = 0
    return dict(N=N, B=B, io=io, S=S, data=data, table=table, rows=rng.permutation(N)[:B].astype(np.int32),
                mask_id=rng.integers(0, S, B).astype(np.int32), mtu=rng.integers(0, S, (N, 3)).astype(np.int32),
                y=rng.standard_normal((B, io)).astype(np.float32))
