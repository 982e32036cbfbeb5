"""float64 statement of a training step with normalised hidden layers (include/codae_hip.h, "Normalisation"), written from the
definition in plain numpy for the tests: forward, loss and every gradient by hand, no autograd, no code of codae.tool.  It extends
tests/residual_ref.py (skips, dropout factors, tied weights) by norm_l:

  a_l = f_l act_l(W_l h_l + b_l)      s_l = a_l + skip_l h_l      h_{l+1} = norm_l ? N(s_l) : s_l      loss on h_L
  layer: mu = sum x / w, v = sum (x - mu)^2 / w, r = 1 / sqrt(v + eps), xhat = (x - mu) r        rms: r = 1 / sqrt(sum x^2 / w + eps), xhat = x r
  Gh_l = D_l W_l + skip_l Gs_l        c1 = sum Gh / w (layer)     c2 = sum (Gh xhat) / w
  Gs_{l-1} = r (Gh_l - c1 - xhat c2)  (rms: no c1; norm_{l-1} = 0: Gh_l)                  D_{l-1} = Gs_{l-1} act'_{l-1} (* f_{l-1})

xhat in the backward is the STORED activation, act' comes from the sign of the value before the skip and the norm.

bf16=True is the restatement with the engine's roundings: everything residual_ref rounds, and the statistics in fp32 from the stored
s_l, xhat rounded to bf16 on store, every U in bf16 behind a norm, Gs in fp32, D rounded once.
"""
import numpy as np

from residual_ref import _act, _dact, bf16_round, mse, packed_mask, positive  # noqa: F401  (re-exported for the tests)


def normalise64(s, kind, eps):
    """-> (xhat, r) in float64 of the rows of s, straight from the definition"""
    s = np.asarray(s, dtype=np.float64)
    w = s.shape[-1]
    with np.errstate(invalid="ignore", over="ignore"):
        if kind == "layer":
            mu = s.sum(axis=-1, keepdims=True) / w
            c = s - mu
            r = 1.0 / np.sqrt((c * c).sum(axis=-1, keepdims=True) / w + np.float64(np.float32(eps)))
            return c * r, r[..., 0]
        r = 1.0 / np.sqrt((s * s).sum(axis=-1, keepdims=True) / w + np.float64(np.float32(eps)))
        return s * r, r[..., 0]


def normalise_engine(s, kind, eps, bf16):
    """-> (xhat as stored widened to float64, r fp32): the statistics in fp32 from the stored s, xhat rounded on store"""
    s = np.asarray(s, dtype=np.float32)
    w = np.float32(s.shape[-1])
    with np.errstate(invalid="ignore", over="ignore"):
        if kind == "layer":
            mu = (s.sum(axis=-1, keepdims=True, dtype=np.float32) / w).astype(np.float32)
            c = (s - mu).astype(np.float32)
            v = ((c * c).sum(axis=-1, keepdims=True, dtype=np.float32) / w).astype(np.float32)
        else:
            c = s
            v = ((s * s).sum(axis=-1, keepdims=True, dtype=np.float32) / w).astype(np.float32)
        r = (np.float32(1) / np.sqrt(v + np.float32(eps), dtype=np.float32)).astype(np.float32)
        xh = (c * r).astype(np.float32)
    return (bf16_round(xh) if bf16 else xh).astype(np.float64), r[..., 0]


def backward_rows(gh, xhat, r, kind):
    """Gs of the definition in float64: gh, xhat [B, w], r [B]"""
    gh, xhat = np.asarray(gh, dtype=np.float64), np.asarray(xhat, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)[:, None]
    w = gh.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        c2 = (gh * xhat).sum(axis=1, keepdims=True) / w
        c1 = gh.sum(axis=1, keepdims=True) / w if kind == "layer" else 0.0
        return r * (gh - c1 - xhat * c2)


def forward(params, acts, skips, norms, kind, eps, c, factors=None, bf16=False):
    """-> (y, hs, a_s, rs): y = h_L, hs[l] = h_l as stored (xhat behind a norm), a_s[l] = a_l (* f_l) as stored, rs[l] = r of a
    normalised layer (else None)"""
    q = bf16_round if bf16 else (lambda t: t)
    L = len(params)
    assert acts[L - 1] is None and not skips[L - 1] and not norms[L - 1]
    h = q(np.asarray(c, dtype=np.float32)).astype(np.float64)
    hs, a_s, rs = [h], [], []
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
                    h, r = normalise_engine(h, kind, eps, True) if bf16 else normalise64(h, kind, eps)
            else:
                h = a
            a_s.append(a)
            rs.append(r)
            hs.append(h)
    return h, hs, a_s, rs


def gradients(params, acts, skips, norms, kind, eps, c, dy_of, factors=None, bf16=False):
    """-> (grads [(dW, db)] float64, loss, y)"""
    q = bf16_round if bf16 else (lambda t: t)
    r32 = (lambda t: t.astype(np.float32).astype(np.float64)) if bf16 else (lambda t: t)
    L = len(params)
    y, hs, a_s, rs = forward(params, acts, skips, norms, kind, eps, c, factors, bf16)
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
            if skips[l] or skips[m] or norms[m]:
                U = q(U.astype(np.float32)).astype(np.float64) if bf16 else U
                Gh = r32(U + G_next) if skips[l] else U
                Gs = r32(backward_rows(Gh, hs[l], rs[m], kind)) if norms[m] else Gh
                G_next = Gs if skips[m] else None
            else:
                Gs = U
                G_next = None
            D = Gs * _dact(acts[m], a_s[m])
            D = q(D.astype(np.float32)).astype(np.float64) if bf16 else D
            f = None if factors is None else factors[m]
            if f is not None:
                D = D * np.asarray(f, dtype=np.float32).astype(np.float64)
                D = q(D.astype(np.float32)).astype(np.float64) if bf16 else D
            db = D.sum(axis=0)
    return grads, loss, y


class StepRef:
    """Steps of the reference: step(c, dy_of, factors) -> {"loss", "grad_norm"}; last_grads (fp32, folded when tied), params."""

    def __init__(self, params, acts, skips, norms, kind, eps, lr, weight_decay, bf16=False, tied=False, clip=1.0):
        from oracle import dae_oracle as O
        self.O = O
        self.params = [(w.astype(np.float32).copy(), b.astype(np.float32).copy()) for w, b in params]
        self.acts, self.skips, self.norms, self.kind, self.eps = list(acts), list(skips), list(norms), kind, eps
        self.lr, self.wd, self.bf16, self.tied, self.clip = lr, weight_decay, bf16, tied, clip
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
        g64, loss, _ = gradients(self.params, self.acts, self.skips, self.norms, self.kind, self.eps, c, dy_of, factors, self.bf16)
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
