"""Independent numpy statement of hidden dropout (include/codae_hip.h, "Hidden dropout"), written from the definition for the
tests: it carries its own Philox4x32-10 and shares no code with codae.tool or tests/noise_ref.py.

  word     Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter (c // 4, dataset row, step, 1 + layer), word c % 4
  T        floor(p 2^32) of the fp32 probability; dropped iff word < T
  f        0 when dropped, else float32(1 / (1 - p))
  forward  a <- a * f (one fp32 product; bf16: widened, multiplied, rounded to nearest even); backward d <- d * f likewise

Step references: the chain h = act(h W^T + b) * f in torch float64 autograd on the CPU from the fp32 parameters (StepRef), and a
restatement with a bf16 rounding wherever the bf16 engine stores (StepRefBf16: after the activation and again after * f, forward
and backward).  Both hand their gradients to the oracle's clip_grad_norm / adam_step.
"""
import math

import numpy as np

MASK32 = (1 << 32) - 1
MUL_A, MUL_B = 0xD2511F53, 0xCD9E8D57
WEYL_A, WEYL_B = 0x9E3779B9, 0xBB67AE85


def _words_of_group(group, row, step, word3, seed):
    """The four 32-bit words of one counter, in plain Python integers."""
    c = [group & MASK32, row & MASK32, step & MASK32, word3 & MASK32]
    k = [seed & MASK32, (seed >> 32) & MASK32]
    for _ in range(10):
        pa, pb = MUL_A * c[0], MUL_B * c[2]
        c = [(pb >> 32) ^ c[1] ^ k[0], pb & MASK32, (pa >> 32) ^ c[3] ^ k[1], pa & MASK32]
        k = [(k[0] + WEYL_A) & MASK32, (k[1] + WEYL_B) & MASK32]
    return c


def words(rows, layer, width, step, seed):
    """uint32 [B, width]: the word of every element of layer `layer`'s output."""
    rows = [int(r) for r in np.asarray(rows).reshape(-1)]
    out = np.zeros((len(rows), width), dtype=np.uint32)
    for i, r in enumerate(rows):
        for g in range((width + 3) // 4):
            w = _words_of_group(g, r, int(step), 1 + int(layer), int(seed))
            for k in range(4):
                if 4 * g + k < width:
                    out[i, 4 * g + k] = w[k]
    return out


def words_vec(rows, layer, width, step, seed):
    """words() in whole-array uint64 arithmetic, for matrices of millions of elements (the tests compare the two on a few rows)"""
    m = np.uint64(MASK32)
    rows = np.asarray(rows).reshape(-1).astype(np.int64).astype(np.uint64) & m
    B, G = rows.size, (width + 3) // 4
    c0 = np.repeat(np.arange(G, dtype=np.uint64)[None, :], B, axis=0)
    c1 = np.repeat(rows[:, None], G, axis=1)
    c2 = np.full((B, G), int(step) & MASK32, dtype=np.uint64)
    c3 = np.full((B, G), (1 + int(layer)) & MASK32, dtype=np.uint64)
    k0, k1 = int(seed) & MASK32, (int(seed) >> 32) & MASK32
    for _ in range(10):
        pa, pb = np.uint64(MUL_A) * c0, np.uint64(MUL_B) * c2
        c0, c1, c2, c3 = (pb >> np.uint64(32)) ^ c1 ^ np.uint64(k0), pb & m, (pa >> np.uint64(32)) ^ c3 ^ np.uint64(k1), pa & m
        k0, k1 = (k0 + WEYL_A) & MASK32, (k1 + WEYL_B) & MASK32
    return np.stack([c0, c1, c2, c3], axis=2).reshape(B, 4 * G)[:, :width].astype(np.uint32)


def threshold(p):
    return int(math.floor(float(np.float32(p)) * 2.0 ** 32))


def scale(p):
    return np.float32(1.0 / (1.0 - float(np.float32(p))))


def dropped(rows, layer, width, step, seed, p):
    return words(rows, layer, width, step, seed).astype(np.uint64) < np.uint64(threshold(p))


def factor(rows, layer, width, step, seed, p):
    """float32 [B, width]"""
    return np.where(dropped(rows, layer, width, step, seed, p), np.float32(0), scale(p)).astype(np.float32)


def bf16_round(a):
    """fp32 -> bf16 (nearest even) -> fp32; a NaN stays a NaN."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(np.float32)
    return np.where(np.isnan(a), np.float32(np.nan), r).astype(np.float32)


def apply(a, f, bf16=False):
    """The stored values after a <- a * f: fp32 product (of the widened bf16 value), rounded to bf16 again when bf16."""
    with np.errstate(invalid="ignore"):
        out = (np.asarray(a, dtype=np.float32) * np.asarray(f, dtype=np.float32)).astype(np.float32)
    return bf16_round(out) if bf16 else out


# ---- whole steps ------------------------------------------------------------------------------------------------------------
# acts: per layer None, "relu" or ("leaky", slope); p: per hidden output (L - 1 values)

def _act_t(torch, kind, z):
    if kind is None:
        return z
    if kind == "relu":
        return torch.relu(z)
    return torch.where(z > 0, z, z * float(np.float32(kind[1])))


class StepRef:
    """float64 autograd.  step(c, x, rows, w=None): c the (corrupted) input, x the clean target, rows the dataset rows, w
    [B, io] loss weights (None: the plain mean squared error); loss = sum w (x - y)^2 / (B io)."""

    def __init__(self, params, acts, p, seed, lr, weight_decay):
        from oracle import dae_oracle as O
        self.O = O
        self.params = [(w.astype(np.float32).copy(), b.astype(np.float32).copy()) for w, b in params]
        self.acts, self.p, self.seed, self.lr, self.wd = list(acts), [float(np.float32(v)) for v in p], int(seed), lr, weight_decay
        self.adam = O.adam_init(self.params)
        self.steps = 0
        self.last_grads = None

    def factors(self, rows, step):
        return [factor(rows, l, self.params[l][0].shape[0], step, self.seed, self.p[l]) if self.p[l] > 0 else None
                for l in range(len(self.params) - 1)]

    def step(self, c, x, rows, w=None, drop=True):
        import torch
        O = self.O
        self.steps += 1
        L = len(self.params)
        fs = self.factors(rows, self.steps) if drop else [None] * (L - 1)
        ps = [(torch.tensor(wt.astype(np.float64), requires_grad=True), torch.tensor(b.astype(np.float64), requires_grad=True))
              for wt, b in self.params]
        h = torch.tensor(np.asarray(c, dtype=np.float32).astype(np.float64))
        for l, (wt, b) in enumerate(ps):
            h = _act_t(torch, self.acts[l], h @ wt.T + b)
            if l < L - 1 and fs[l] is not None:
                h = h * torch.tensor(fs[l].astype(np.float64))
        xt = torch.tensor(np.asarray(x, dtype=np.float32).astype(np.float64))
        se = (xt - h) ** 2
        wt_ = 1.0 if w is None else torch.tensor(np.asarray(w, dtype=np.float64))
        loss = (wt_ * se).sum() / float(xt.numel())
        loss.backward()
        grads = [(wt.grad.numpy().astype(np.float32), b.grad.numpy().astype(np.float32)) for wt, b in ps]
        self.last_grads = grads
        clipped, gnorm = O.clip_grad_norm(grads, 1.0)
        self.params = O.adam_step(self.params, clipped, self.adam, self.lr, self.wd)
        return {"loss": float(loss.detach()), "grad_norm": float(gnorm), "sq_full": float(se.detach().sum())}


def _act_np(kind, z):
    if kind is None:
        return z
    if kind == "relu":
        return np.maximum(z, 0)
    return np.where(z > 0, z, z * np.float32(kind[1]))


def _dact_np(kind, saved):
    """act'(.) from the SAVED output, as the engine's backward takes it."""
    if kind is None:
        return 1.0
    if kind == "relu":
        return (saved > 0).astype(np.float64)
    return np.where(saved > 0, 1.0, np.float64(np.float32(kind[1])))


class StepRefBf16(StepRef):
    """The same step with the bf16 engine's roundings: the input, the weights and every hidden activation are bf16 (rounded after
    the activation and again after * f), every stored activation gradient is bf16 (rounded after the activation derivative and
    again after * f); products and sums in float64; the last layer's output and dy stay fp32, and its bias gradient sums the
    unrounded dy.  Plain mean squared error only."""

    def step(self, c, x, rows, w=None, drop=True):
        assert w is None
        O = self.O
        q = O.bf16_round
        self.steps += 1
        L = len(self.params)
        fs = self.factors(rows, self.steps) if drop else [None] * (L - 1)
        h = q(np.asarray(c, dtype=np.float32))
        saved = [h]
        for l, (wt, b) in enumerate(self.params):
            z = (h.astype(np.float64) @ q(wt).astype(np.float64).T + b.astype(np.float64)).astype(np.float32)
            h = _act_np(self.acts[l], z).astype(np.float32)
            if l < L - 1:
                h = q(h)
                if fs[l] is not None:
                    h = apply(h, fs[l], bf16=True)
            saved.append(h)
        x = np.asarray(x, dtype=np.float32)
        se = (x.astype(np.float64) - h.astype(np.float64)) ** 2
        dy = ((h.astype(np.float64) - x.astype(np.float64)) * (2.0 / x.size)).astype(np.float32)
        grads = [None] * L
        db = dy.astype(np.float64).sum(axis=0)
        d = q(dy)
        for l in range(L - 1, -1, -1):
            grads[l] = ((d.astype(np.float64).T @ saved[l].astype(np.float64)).astype(np.float32), db.astype(np.float32))
            if l > 0:
                g = d.astype(np.float64) @ q(self.params[l][0]).astype(np.float64)
                d = q((g * _dact_np(self.acts[l - 1], saved[l])).astype(np.float32))
                if fs[l - 1] is not None:
                    d = apply(d, fs[l - 1], bf16=True)
                db = d.astype(np.float64).sum(axis=0)
        self.last_grads = grads
        clipped, gnorm = O.clip_grad_norm(grads, 1.0)
        self.params = O.adam_step(self.params, clipped, self.adam, self.lr, self.wd)
        return {"loss": float(se.sum() / x.size), "grad_norm": float(gnorm), "sq_full": float(se.sum())}
