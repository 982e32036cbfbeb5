"""A denoising autoencoder with tied weights in plain torch, written from the definition (include/codae_hip.h, "Tied weights")
for the tests: it shares no code with the library or with codae.tool.tied.

  layer l < ceil(L / 2) owns W_l:  F.linear(x, W_l);   layer l' = L-1-l uses F.linear(x, W_l.t());   every layer owns its bias.
  One nn.Parameter per free tensor, so autograd adds the two uses of W_l, clip_grad_norm_ counts it once and a torch optimizer
  decays and updates it once.

TiedModel(tied=False) is the same stack with one parameter per layer (what the engine computes before its fold).  It keeps each
decoder matrix in the encoder's layout, V_l' = W_l'^T, and multiplies by V_l'.t() - the transposed view the tied model multiplies by -
so the two models issue the same matrix products on the same strides and float64 sums run in the same order whichever BLAS path a
host takes for a transposed operand; flat_grads transposes that gradient back into the decoder's own layout.  bf16=True
rounds where the bf16 engine rounds (oracle/dae_oracle.py's `quant`, DESIGN.md section 3, layer 2): the corrupted input, the weight
operands, every hidden activation and every activation gradient to bf16; accumulation, biases, the last layer's output, the
last bias gradient (sums of the unrounded dL/dy) and the weight gradients stay wide.

flat_layout / flatten restate the engine's flat parameter vector: [W_0 | .. | W_{L-1} | b_0 | ..], every tensor padded to 64 floats.
"""
import numpy as np
import torch
import torch.nn.functional as F


def n_free(L):
    return (L + 1) // 2


def flat_layout(schedule):
    """(w_off, b_off, n_param)."""
    off, w_off, b_off = 0, [], []
    for s in schedule:
        w_off.append(off)
        off += (s[0] * s[1] + 63) // 64 * 64
    for s in schedule:
        b_off.append(off)
        off += (s[1] + 63) // 64 * 64
    return w_off, b_off, off


def flatten(schedule, weights, biases, dtype=torch.float64):
    """weights[l] [out][in] (None: left zero), biases[l] [out] -> the flat vector."""
    w_off, b_off, n = flat_layout(schedule)
    flat = torch.zeros(n, dtype=dtype)
    for l, s in enumerate(schedule):
        if weights[l] is not None:
            flat[w_off[l]:w_off[l] + s[0] * s[1]] = torch.as_tensor(weights[l]).to(dtype).reshape(-1)
        flat[b_off[l]:b_off[l] + s[1]] = torch.as_tensor(biases[l]).to(dtype)
    return flat


def free_mask(schedule):
    """bool [n_param]: the elements of the free tensors (no decoder matrix, no padding)."""
    w_off, b_off, n = flat_layout(schedule)
    m = np.zeros(n, dtype=bool)
    for l, s in enumerate(schedule):
        if l < n_free(len(schedule)):
            m[w_off[l]:w_off[l] + s[0] * s[1]] = True
        m[b_off[l]:b_off[l] + s[1]] = True
    return m


def tied_init(schedule, seed, bias_scale=0.05):
    """[(W, b)] fp32 numpy, Xavier-uniform encoder matrices, decoder matrices their transposes, small non-zero biases."""
    rng = np.random.default_rng(seed)
    L = len(schedule)
    ws = []
    for l, s in enumerate(schedule):
        a = (6.0 / (s[0] + s[1])) ** 0.5
        w = rng.uniform(-a, a, size=(s[1], s[0])).astype(np.float32)
        ws.append(w if l < n_free(L) else np.ascontiguousarray(ws[L - 1 - l].T))
    return [(w, (bias_scale * rng.standard_normal(s[1])).astype(np.float32)) for w, s in zip(ws, schedule)]


def bf16_grid(t):
    """The value a bf16 store keeps, in t's dtype."""
    return t.to(torch.float32).bfloat16().to(t.dtype)


class _Round(torch.autograd.Function):
    """forward: round the value (fwd) or pass it; backward: round the gradient (bwd) or pass it."""

    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.bwd = bwd
        return bf16_grid(x) if fwd else x.clone()

    @staticmethod
    def backward(ctx, g):
        return (bf16_grid(g) if ctx.bwd else g), None, None


class TiedModel(torch.nn.Module):
    def __init__(self, schedule, params, dtype=torch.float64, tied=True, bf16=False):
        super().__init__()
        self.schedule = [tuple(s) for s in schedule]
        self.L = len(schedule)
        self.tied, self.bf16 = tied, bf16
        n_own = n_free(self.L) if tied else self.L
        self.w = torch.nn.ParameterList([torch.nn.Parameter(self._held(l, torch.as_tensor(params[l][0]).to(dtype))) for l in range(n_own)])
        self.b = torch.nn.ParameterList([torch.nn.Parameter(torch.as_tensor(params[l][1]).to(dtype).clone()) for l in range(self.L)])

    def _held(self, l, w):
        """a decoder matrix of the untied model is held transposed (the encoder's layout), every other matrix as it is"""
        return w.t().contiguous() if l >= n_free(self.L) else w.clone()

    def weight(self, l):
        if l < n_free(self.L):
            return self.w[l]
        return self.w[self.L - 1 - l].t() if self.tied else self.w[l].t()

    def forward(self, x):
        h = _Round.apply(x, True, False) if self.bf16 else x
        for l, s in enumerate(self.schedule):
            last = l == self.L - 1
            W = self.weight(l)
            if self.bf16:
                W = _Round.apply(W, True, False)
            if self.bf16 and last:
                z = _Round.apply(F.linear(h, W), False, True) + self.b[l]      # (the bias gradient sums the unrounded dL/dy)
            else:
                z = F.linear(h, W, self.b[l])
            if s[2]:
                z = torch.relu(z)
            if self.bf16 and not last:
                z = _Round.apply(z, True, True)
            h = z
        return h

    def loss(self, x, fmask):
        """MSELoss('mean') of the reconstruction of the blanked input against the clean row."""
        y = self.forward(x * fmask)
        return ((x - y) ** 2).mean()

    def flat_params(self):
        return flatten(self.schedule, [self.weight(l).detach() for l in range(self.L)], [b.detach() for b in self.b])

    def flat_grads(self):
        """Gradients in the flat layout; a tied model leaves the decoder ranges zero (the folded form)."""
        ws = [None if l >= len(self.w) else self.w[l].grad if l < n_free(self.L) else self.w[l].grad.t() for l in range(self.L)]
        return flatten(self.schedule, ws, [b.grad for b in self.b])
