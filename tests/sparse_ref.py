"""Restatement of the sparse code (include/codae_hip.h, "Sparse code") in plain numpy for the tests: the key, the selection by a
brute-force ranking, and the float64 statement of a training step with a sparse layer.  No code of codae.tool.  It extends
tests/norm_ref.py (skips, norms, dropout factors, tied weights) by the layer m whose output is sparsified:

  a_l = f_l act_l(W_l h_l + b_l)    s_l = a_l + skip_l h_l    h_{l+1} = norm_l ? N(s_l) : s_l    h_{m+1} <- kept ? h_{m+1} : +0
  D_m = (Gs_m act'_m, rounded), then kept ? D_m : +0, then the dropout factor

key(v) = the stored bits with the sign cleared, as an unsigned integer; columns ranked by (key descending, column ascending), the
first `keep` are kept.  The network functions take the mask as GIVEN (the engine's own, read back from its work space) when one is
passed, so that a summation-order difference at the threshold does not turn into a different network; mask=None selects from the
restatement's own stored values.
"""
import numpy as np

import norm_ref as NR
from residual_ref import _act, _dact, bf16_round, mse  # noqa: F401  (re-exported for the tests)


def key(a, bf16=False):
    """int64 keys of fp32 values (bf16: the values are bf16 numbers held in fp32; their 15 magnitude bits)"""
    u = np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32).astype(np.int64)
    return (u >> 16) & 0x7FFF if bf16 else u & 0x7FFFFFFF


def ranking(a, bf16=False):
    """int [B, Z]: the columns of every row in rank order, by sorting them in plain Python"""
    k = key(a, bf16)
    B, Z = k.shape
    return np.array([sorted(range(Z), key=lambda j: (-int(k[b, j]), j)) for b in range(B)], dtype=np.int64).reshape(B, Z)


def select(a, keep, bf16=False, order=None):
    """bool [B, Z]: the kept columns of every row - the first `keep` of the ranking (order: a ranking computed before)"""
    order = ranking(a, bf16) if order is None else order
    B, Z = order.shape
    assert 1 <= keep <= Z
    mask = np.zeros((B, Z), dtype=bool)
    np.put_along_axis(mask, order[:, :keep], True, axis=1)
    return mask


def _f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def planted_rows(Z, keep, rng):
    """fp32 rows [n, Z] that pin the edge cases of the ranking (Z >= 8)"""
    rows = []
    r = np.full(Z, 1.5, dtype=np.float32)                          # all magnitudes equal, mixed signs: the lowest columns win
    r[::2] *= -1
    rows.append(r)
    r = np.zeros(Z, dtype=np.float32)                              # all +-0
    r[1::2] = -0.0
    rows.append(r)
    r = rng.permutation(np.arange(1, Z + 1)).astype(np.float32)    # the keep-th and the (keep+1)-th equal (when there are two)
    order = np.argsort(-r, kind="stable")
    if keep < Z:
        r[order[keep]] = r[order[keep - 1]]
        r[order[keep]] *= -1
    rows.append(r)
    r = rng.standard_normal(Z).astype(np.float32)                  # NaN of both signs and two payloads, +-Inf
    r[Z - 1] = _f32([0x7FC00000])[0]
    r[Z - 2] = _f32([0xFFC00000])[0]
    r[1] = _f32([0x7FC10000])[0]
    r[0] = np.inf
    r[2] = -np.inf
    rows.append(r)
    r = rng.standard_normal(Z).astype(np.float32) * np.float32(1e-3)   # subnormals among small values and zeros
    r[::3] = _f32([0x00010000])[0]
    r[1::3] = 0.0
    r[Z - 1] = _f32([0x80020000])[0]
    rows.append(r)
    return np.stack(rows)


def apply_bits(a, mask):
    """fp32 [B, Z]: the bits of a where mask, +0 elsewhere"""
    u = np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)
    return np.where(mask, u, np.uint32(0)).astype(np.uint32).view(np.float32)


def packed(mask):
    """uint8 [B, ceil(Z / 8)]: column 8 j + i in bit i of byte j, pad bits 0"""
    return np.packbits(mask, axis=1, bitorder="little")


def unpacked(bits, Z):
    return np.unpackbits(np.asarray(bits, dtype=np.uint8), axis=1, bitorder="little")[:, :Z].astype(bool)


def forward(params, acts, skips, norms, kind, eps, c, m, keep, mask=None, factors=None, bf16=False):
    """-> (y, hs, a_s, rs, pre, mask): norm_ref.forward's outputs with h_{m+1} sparsified; pre = h_{m+1} before the selection (as
    stored), mask = the selection used"""
    q = bf16_round if bf16 else (lambda t: t)
    L = len(params)
    assert acts[L - 1] is None and not skips[L - 1] and not norms[L - 1] and 0 <= m < L - 1 and not skips[m] and not norms[m]
    h = q(np.asarray(c, dtype=np.float32)).astype(np.float64)
    hs, a_s, rs = [h], [], []
    pre = None
    with np.errstate(invalid="ignore", over="ignore"):
        for l, (W, b) in enumerate(params):
            Wq = q(np.asarray(W, dtype=np.float32)).astype(np.float64)
            z = h @ Wq.T + np.asarray(b, dtype=np.float32).astype(np.float64)
            if bf16:
                z = z.astype(np.float32).astype(np.float64)
            a = _act(acts[l], z)
            r = None
            if l < L - 1:
                a = q(a).astype(np.float64)
                f = None if factors is None else factors[l]
                if f is not None:
                    a = a * np.asarray(f, dtype=np.float32).astype(np.float64)
                    a = q(a.astype(np.float32) if bf16 else a).astype(np.float64)
                h = a + h if skips[l] else a
                if skips[l]:
                    h = q(h.astype(np.float32) if bf16 else h).astype(np.float64)
                if norms[l]:
                    h, r = NR.normalise_engine(h, kind, eps, True) if bf16 else NR.normalise64(h, kind, eps)
                if l == m:
                    pre = h
                    if mask is None:
                        mask = select(h.astype(np.float32), keep, bf16)
                    assert mask.shape == h.shape
                    h = np.where(mask, h, 0.0)
            else:
                h = a
            a_s.append(a)
            rs.append(r)
            hs.append(h)
    return h, hs, a_s, rs, pre, mask


def gradients(params, acts, skips, norms, kind, eps, c, dy_of, m, keep, mask=None, factors=None, bf16=False):
    """-> (grads [(dW, db)] float64, loss, y, pre, mask)"""
    q = bf16_round if bf16 else (lambda t: t)
    r32 = (lambda t: t.astype(np.float32).astype(np.float64)) if bf16 else (lambda t: t)
    L = len(params)
    y, hs, a_s, rs, pre, mask = forward(params, acts, skips, norms, kind, eps, c, m, keep, mask, factors, bf16)
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
            j = l - 1
            if skips[l] or skips[j] or norms[j]:
                U = q(U.astype(np.float32)).astype(np.float64) if bf16 else U
                Gh = r32(U + G_next) if skips[l] else U
                Gs = r32(NR.backward_rows(Gh, hs[l], rs[j], kind)) if norms[j] else Gh
                G_next = Gs if skips[j] else None
            else:
                Gs = U
                G_next = None
            D = Gs * _dact(acts[j], a_s[j])
            D = q(D.astype(np.float32)).astype(np.float64) if bf16 else D
            if j == m:
                D = np.where(mask, D, 0.0)                      # a selection: +0 under a dropped column whatever D held
            f = None if factors is None else factors[j]
            if f is not None:
                D = D * np.asarray(f, dtype=np.float32).astype(np.float64)
                D = q(D.astype(np.float32)).astype(np.float64) if bf16 else D
            db = D.sum(axis=0)
    return grads, loss, y, pre, mask


class StepRef(NR.StepRef):
    """norm_ref.StepRef with the sparse layer: step(c, dy_of, factors, mask) - mask: the engine's own selection of this step, or
    None for the restatement's"""

    def __init__(self, params, acts, skips, norms, kind, eps, lr, weight_decay, m, keep, bf16=False, tied=False, clip=1.0):
        super().__init__(params, acts, skips, norms, kind, eps, lr, weight_decay, bf16=bf16, tied=tied, clip=clip)
        self.m, self.keep = m, keep
        self.last_pre = self.last_mask = None

    def grads_of(self, c, dy_of, factors=None, mask=None):
        g64, loss, _, self.last_pre, self.last_mask = gradients(self.params, self.acts, self.skips, self.norms, self.kind, self.eps, c, dy_of,
                                                                self.m, self.keep, mask, factors, self.bf16)
        return g64, loss

    def step(self, c, dy_of, factors=None, mask=None):
        O = self.O
        L = len(self.params)
        g64, loss = self.grads_of(c, dy_of, factors, mask)
        gw = [g[0].astype(np.float32) for g in g64]
        gb = [g[1].astype(np.float32) for g in g64]
        if self.tied:
            for l in range(L // 2):
                gw[l] = (gw[l].astype(np.float64) + gw[L - 1 - l].astype(np.float64).T).astype(np.float32)
                gw[L - 1 - l] = np.zeros_like(gw[L - 1 - l])
        self.last_grads = list(zip(gw, gb))
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


def selection_is_valid(pre, mask, keep, bf16):
    """The engine's selection `mask` against the restatement's pre-selection magnitudes `pre`: every row keeps exactly `keep`
    columns, and no kept column's magnitude lies below a dropped column's by more than 4 units in the last place of the threshold
    value (2^-8 relative in bf16, 2^-23 in fp32: the activations of two summation orders differ by that much, not by more).
    -> (ok, worst excess in units of the allowance)"""
    mag = np.abs(np.asarray(pre, dtype=np.float64))
    if not (mask.sum(axis=1) == keep).all():
        return False, float("inf")
    lowest_kept = np.where(mask, mag, np.inf).min(axis=1)
    highest_dropped = np.where(mask, -np.inf, mag).max(axis=1)
    ulp = 2.0 ** -8 if bf16 else 2.0 ** -23
    allow = 4 * ulp * np.maximum(highest_dropped, 0.0)
    gap = highest_dropped - lowest_kept
    worst = float(np.max(np.where(allow > 0, gap / np.maximum(allow, 1e-300), np.where(gap > 0, np.inf, 0.0))))
    return bool((gap <= allow).all()), worst
