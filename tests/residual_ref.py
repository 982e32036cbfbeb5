"""float64 statement of a training step with residual connections (include/codae_hip.h, "Residual connections"), written from
the definition in plain numpy for the tests: forward, loss and every gradient by hand, no autograd, no code of codae.tool.

  z_l = W_l h_l + b_l      a_l = act_l(z_l) (* f_l)      h_{l+1} = a_l + skip_l h_l      loss on h_L
  U_l = W_l^T D_l          G_l = U_l + skip_l G_{l+1}    D_{l-1} = G_l * act'_{l-1} (* f_{l-1})      db_{l-1} = column sums of D_{l-1}

acts: per layer None, "relu" or ("leaky", slope); the last layer has none.  The derivative of ReLU / LeakyReLU is taken from
the sign of a_l (after the dropout factor, as the engine's 1-bit mask and its saved activations are): where f_l = 0 it is
multiplied by f_l = 0 anyway.  factors: None, or per hidden layer None / a float32 [B, out[l]] array (HiddenDropout.factor).

bf16=True rounds to bf16 (nearest even) exactly where the bf16 engine stores bf16: the input, the weights, every a_l, a_l f_l
and h_{l+1}; every U_l and every D_l.  G stays fp32 (one fp32 add per level), the last layer's output and dy stay fp32, and the
last bias gradient sums the unrounded dy.  A data gradient with no skip on either side is rounded once, behind the derivative,
as the GEMM epilogue does.

tied=True: layer L-1-l uses the transpose of layer l < L // 2; the decoder matrices' gradients are folded into the encoder's
and left zero, and the update moves the free tensors only (oracle.dae_oracle.clip_grad_norm / adam_step on them), then mirrors.
"""
import numpy as np


def bf16_round(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(np.float32)
    return np.where(np.isnan(a), np.float32(np.nan), r).astype(np.float32)


def positive(a):
    """The engine's mask predicate on a stored value: sign clear and not zero (a NaN with a clear sign counts)."""
    a32 = np.ascontiguousarray(a, dtype=np.float32)
    u = a32.view(np.uint32)
    return ((u >> np.uint32(31)) == 0) & ((u & np.uint32(0x7FFFFFFF)) != 0)


def packed_mask(a, bf16=False):
    """uint8 [B, ceil(width / 8)]: the 1-bit mask of a [B, width] as the forward kernel writes it (column 8 j + k in bit k)."""
    a = bf16_round(a) if bf16 else np.asarray(a, dtype=np.float32)
    return np.packbits(positive(a), axis=1, bitorder="little")


def colsum_parts_fixed_order(stored_f32, B):
    """The partial column sums a backward streaming kernel (dropout, residual, norm) leaves, from the values it STORED, in the
    order its sweep adds them: per block of 64 batch rows, wave w of 16 adds its rows 4 w .. 4 w + 3 that are < B in row order
    to a zero, (((0 + r0) + r1) + r2) + r3, then wave 0's sum takes the sums of waves 1 .. 15 in order.  Every step is one IEEE
    fp32 addition, so float32 numpy gives the kernel's bits.  -> float32 [ceil(B / 64), width]"""
    d = np.ascontiguousarray(stored_f32, dtype=np.float32)[:B]
    blocks = (B + 63) // 64
    out = np.zeros((blocks, d.shape[1]), dtype=np.float32)
    for k in range(blocks):
        total = None
        for w in range(16):
            s = np.zeros(d.shape[1], dtype=np.float32)
            for b in range(64 * k + 4 * w, min(64 * k + 4 * w + 4, B)):
                s = s + d[b]
            total = s if total is None else total + s
        out[k] = total
    return out


def _act(kind, z):
    if kind is None:
        return z
    if kind == "relu":
        return np.where(np.isnan(z), z, np.maximum(z, 0))
    return np.where(z > 0, z, z * np.float64(np.float32(kind[1])))


def _dact(kind, a):
    if kind is None:
        return 1.0
    if kind == "relu":
        return (a > 0).astype(np.float64)
    return np.where(a > 0, 1.0, np.float64(np.float32(kind[1])))


def mse(x, w=None):
    """dy_of for the (weighted) mean squared error against the clean rows x: loss = sum w (x - y)^2 / (B io)."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)

    def dy_of(y):
        ww = 1.0 if w is None else np.asarray(w, dtype=np.float64)
        d = y.astype(np.float64) - x64
        return ww * d * (2.0 / x64.size), float((ww * d * d).sum() / x64.size)
    return dy_of


def forward(params, acts, skips, c, factors=None, bf16=False):
    """-> (y, hs, a_s): y = h_L (float64; bf16: the fp32 output), hs[l] = h_l as stored, a_s[l] = a_l (* f_l) as stored."""
    q = bf16_round if bf16 else (lambda t: t)
    L = len(params)
    assert acts[L - 1] is None and not skips[L - 1]
    h = q(np.asarray(c, dtype=np.float32)).astype(np.float64)
    hs, a_s = [h], []
    with np.errstate(invalid="ignore", over="ignore"):
        for l, (W, b) in enumerate(params):
            Wq = q(np.asarray(W, dtype=np.float32)).astype(np.float64)
            z = h @ Wq.T + np.asarray(b, dtype=np.float32).astype(np.float64)
            if bf16:
                z = z.astype(np.float32).astype(np.float64)
            a = _act(acts[l], z)
            if l < L - 1:
                a = q(a).astype(np.float64)
                f = None if factors is None else factors[l]
                if f is not None:
                    a = a * np.asarray(f, dtype=np.float32).astype(np.float64)
                    a = q(a.astype(np.float32) if bf16 else a).astype(np.float64)
                h = a + h if skips[l] else a
                if skips[l]:
                    h = q(h.astype(np.float32) if bf16 else h).astype(np.float64)
            else:
                h = a
            a_s.append(a)
            hs.append(h)
    return h, hs, a_s


def gradients(params, acts, skips, c, dy_of, factors=None, bf16=False):
    """-> (grads [(dW, db)] float64, loss, y)"""
    q = bf16_round if bf16 else (lambda t: t)
    r32 = (lambda t: t.astype(np.float32).astype(np.float64)) if bf16 else (lambda t: t)
    L = len(params)
    y, hs, a_s = forward(params, acts, skips, c, factors, bf16)
    dy, loss = dy_of(y)
    if bf16:
        dy = dy.astype(np.float32).astype(np.float64)
    grads = [None] * L
    db = dy.sum(axis=0)
    D = q(dy.astype(np.float32)).astype(np.float64) if bf16 else dy
    G_next = None
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(L - 1, -1, -1):
            grads[l] = (D.T @ hs[l], db)
            if l == 0:
                break
            Wq = q(np.asarray(params[l][0], dtype=np.float32)).astype(np.float64)
            U = D @ Wq
            m = l - 1
            if skips[l] or skips[m]:
                U = q(U.astype(np.float32)).astype(np.float64) if bf16 else U
                G = r32(U + G_next) if skips[l] else U
                G_next = G if skips[m] else None
            else:
                G = U
                G_next = None
            D = G * _dact(acts[m], a_s[m])
            D = q(D.astype(np.float32)).astype(np.float64) if bf16 else D
            f = None if factors is None else factors[m]
            if f is not None:
                D = D * np.asarray(f, dtype=np.float32).astype(np.float64)
                D = q(D.astype(np.float32)).astype(np.float64) if bf16 else D
            db = D.sum(axis=0)
    return grads, loss, y


class StepRef:
    """Steps of the reference: step(c, dy_of, factors) -> {"loss", "grad_norm"}; last_grads (fp32, folded when tied), params."""

    def __init__(self, params, acts, skips, lr, weight_decay, bf16=False, tied=False, clip=1.0):
        from oracle import dae_oracle as O
        self.O = O
        self.params = [(w.astype(np.float32).copy(), b.astype(np.float32).copy()) for w, b in params]
        self.acts, self.skips, self.lr, self.wd, self.bf16, self.tied, self.clip = list(acts), list(skips), lr, weight_decay, bf16, tied, clip
        L = len(params)
        self.free = [l for l in range(L) if not tied or l < (L + 1) // 2]
        self.adam = None
        self.last_grads = None
        if tied:
            self._mirror()

    def _mirror(self):
        L = len(self.params)
        for l in range(L // 2):
            self.params[L - 1 - l] = (self.params[l][0].T.copy(), self.params[L - 1 - l][1])

    def step(self, c, dy_of, factors=None):
        O = self.O
        L = len(self.params)
        g64, loss, _ = gradients(self.params, self.acts, self.skips, c, dy_of, factors, self.bf16)
        gw = [g[0].astype(np.float32) for g in g64]
        gb = [g[1].astype(np.float32) for g in g64]
        if self.tied:
            for l in range(L // 2):
                gw[l] = (gw[l].astype(np.float64) + gw[L - 1 - l].astype(np.float64).T).astype(np.float32)
                gw[L - 1 - l] = np.zeros_like(gw[L - 1 - l])
        self.last_grads = list(zip(gw, gb))
        # the update sees the free tensors: every bias, and the matrices the stack owns
        none = np.zeros((0, 0), dtype=np.float32)
        tensors = [(self.params[l][0] if l in self.free else none, self.params[l][1]) for l in range(L)]
        grads = [(gw[l] if l in self.free else none, gb[l]) for l in range(L)]
        if self.adam is None:
            self.adam = O.adam_init(tensors)
        clipped, gnorm = O.clip_grad_norm(grads, self.clip)
        new = O.adam_step(tensors, clipped, self.adam, self.lr, self.wd)
        self.params = [(new[l][0] if l in self.free else self.params[l][0], new[l][1]) for l in range(L)]
        if self.tied:
            self._mirror()
        return {"loss": loss, "grad_norm": float(gnorm)}
