"""Residual (skip) connections around equal-width hidden layers - the counterpart of codae_residual in include/codae_hip.h.

Layers are l = 0 .. L-1, h_0 is the corrupted input and skip_l is 0 or 1:

    z_l = W_l h_l + b_l        a_l = act_l(z_l)  (times the dropout factor f_l when layer l is dropped)
    h_{l+1} = a_l + skip_l h_l                   loss on h_L

An identity skip costs no parameters and no projection, so it is allowed only where in[l] == out[l]; never around the last
layer, whose output is the reconstruction; and only where act_l is none, ReLU or LeakyReLU: the engine takes a derivative from
the saved output, and once h_l is added that output no longer determines it (the skipped layers keep a 1-bit mask instead).
It is part of the MODEL: training steps, eval_batch, complete, score_outfits and the averaged weights all run through the skips.

Residual carries the choice of layers, resolves it against a stack (resolve), hands it to the HIP engine
(DaeEngine.set_residual, HipEmbeddingTrainer(residual=...)) and states the same network in whole-tensor torch ops with autograd
(forward) for host tensors and tests.
"""
from ..hip import ACT_ELU, ACT_HARDSIGMOID, ACT_LEAKY, ACT_NONE, ACT_RELU, ACT_RELU6, ACT_SOFTPLUS, HipError

_ACT_NAMES = {ACT_NONE: "none", ACT_RELU: "ReLU", ACT_LEAKY: "LeakyReLU", ACT_RELU6: "ReLU6", ACT_ELU: "ELU", ACT_SOFTPLUS: "Softplus",
              ACT_HARDSIGMOID: "Hardsigmoid"}
ALLOWED_ACTS = (ACT_NONE, ACT_RELU, ACT_LEAKY)


def _act_tuple(a):
    """(kind, p0, p1, p2) of one layer's entry: a bool (ReLU or none), a CODAE_ACT_* kind, or the engine's 4-tuple."""
    if isinstance(a, bool):
        return (ACT_RELU if a else ACT_NONE, 0.0, 0.0, 0.0)
    if isinstance(a, int):
        return (a, 0.0, 0.0, 0.0)
    a = tuple(a)
    if len(a) != 4:
        raise HipError("residual: activation per layer must be a bool, a kind or (kind, p0, p1, p2), got %r" % (a,))
    import numpy as np
    return (int(a[0]),) + tuple(float(np.float32(v)) for v in a[1:])       # (fp32 parameters, the type the C side sees)


def _apply_act(act, z):
    import torch
    kind, p0, p1, p2 = act
    if kind == ACT_NONE:
        return z
    if kind == ACT_RELU:
        return torch.relu(z)
    if kind == ACT_LEAKY:
        return torch.nn.functional.leaky_relu(z, p0)
    if kind == ACT_RELU6:
        return torch.nn.functional.relu6(z)
    if kind == ACT_ELU:               # scale p0, alpha p1, 1 / beta p2 (ELU, CELU and SELU in one form)
        return torch.where(z > 0, z * p0, torch.expm1(z * p2) * (p1 * p0))
    if kind == ACT_SOFTPLUS:
        return torch.nn.functional.softplus(z, beta=p0, threshold=p1)
    if kind == ACT_HARDSIGMOID:
        return torch.nn.functional.hardsigmoid(z)
    raise HipError("residual: unknown activation kind %r" % (kind,))


class Residual:
    """Residual("hidden") | Residual([1, 2, 5]).  "hidden": every layer 1 <= l <= L-2 with equal widths and an allowed
    activation (none, ReLU, LeakyReLU); a list: exactly those layers, each of which must qualify (layer 0 may be listed when
    its widths are equal).  An empty list = off: the engine runs exactly what it runs without the argument."""

    def __init__(self, layers="hidden"):
        if isinstance(layers, str):
            if layers != "hidden":
                raise HipError("residual: layers must be 'hidden' or a list of layer indices, got %r" % (layers,))
            self.layers = "hidden"
            return
        if not hasattr(layers, "__iter__"):
            raise HipError("residual: layers must be 'hidden' or a list of layer indices, got %r" % (layers,))
        out = []
        for v in layers:
            v = v.item() if hasattr(v, "item") else v
            if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                raise HipError("residual: layer indices must be integers >= 0, got %r" % (v,))
            out.append(int(v))
        if len(set(out)) != len(out):
            raise HipError("residual: a layer is listed twice in %r" % (out,))
        self.layers = tuple(sorted(out))

    def __repr__(self):
        return "Residual(%r)" % ("hidden" if self.layers == "hidden" else list(self.layers))

    @property
    def is_off(self):
        return self.layers == ()

    @staticmethod
    def refusal(l, in_features, out_features, acts):
        """Why layer l of the stack takes no skip, or None."""
        L = len(in_features)
        if l >= L:
            return "layer %d: the stack has %d layers" % (l, L)
        if l == L - 1:
            return "layer %d: the last layer's output is the reconstruction and takes no skip" % l
        if int(in_features[l]) != int(out_features[l]):
            return "layer %d: an identity skip needs equal widths (%d -> %d)" % (l, int(in_features[l]), int(out_features[l]))
        if acts[l][0] not in ALLOWED_ACTS:
            return "layer %d: a skipped layer's activation must be none, ReLU or LeakyReLU (got %s)" % (
                l, _ACT_NAMES.get(acts[l][0], acts[l][0]))
        return None

    def resolve(self, in_features, out_features, activation):
        """The L flags (0 / 1) of this choice on a stack: in_features / out_features per layer, activation per layer (a bool =
        ReLU or none, a CODAE_ACT_* kind, or the engine's (kind, p0, p1, p2)).  A listed layer that cannot take a skip raises
        HipError naming the layer and the reason; "hidden" takes the layers that can."""
        L = len(in_features)
        if len(out_features) != L or len(activation) != L:
            raise HipError("residual: %d input widths, %d output widths, %d activations" % (L, len(out_features), len(activation)))
        acts = [_act_tuple(a) for a in activation]
        if self.layers == "hidden":
            return [1 if 1 <= l <= L - 2 and self.refusal(l, in_features, out_features, acts) is None else 0 for l in range(L)]
        flags = [0] * L
        for l in self.layers:
            why = self.refusal(l, in_features, out_features, acts)
            if why is not None:
                raise HipError("residual: " + why)
            flags[l] = 1
        return flags

    def forward(self, x, weights, biases, activation, dropout_factors=None):
        """h_L of the definition above in whole-tensor torch ops (autograd works through it).  weights[l]: [out, in], biases[l]:
        [out]; activation as resolve takes it; dropout_factors: None, or per layer None / a [B, out[l]] tensor of factors
        (HiddenDropout.factor) that multiplies a_l before the skip is added."""
        L = len(weights)
        acts = [_act_tuple(a) for a in activation]
        flags = self.resolve([int(w.shape[1]) for w in weights], [int(w.shape[0]) for w in weights], acts)
        h = x
        for l in range(L):
            a = _apply_act(acts[l], h @ weights[l].t() + biases[l])
            if dropout_factors is not None and l < len(dropout_factors) and dropout_factors[l] is not None:
                a = a * dropout_factors[l]
            h = a + h if flags[l] else a
        return h


def meta_mismatch(meta, layers):
    """The checkpoint's structure check: None when the file's record of skipped layers (meta["residual"]: a list, or None; a
    file written before the key existed has none) names the layers `layers` of the trainer, else the sentence that says how
    they differ."""
    in_file = sorted(int(l) for l in (meta.get("residual") or ()))
    mine = sorted(int(l) for l in (layers or ()))
    if in_file == mine:
        return None
    return "the file was written with residual connections around layers %s, this trainer has them around %s" % (
        in_file or "none", mine or "none")


def residual_from_config(block):
    """The `HIP: RESIDUAL:` block of the embedding script's config: {LAYERS: hidden | [1, 2, ..]}.  None / empty -> None."""
    if not block:
        return None
    if not isinstance(block, dict):
        raise HipError("RESIDUAL must be a mapping with LAYERS, got %r" % (block,))
    known = {"LAYERS"}
    extra = sorted(set(block) - known, key=str)
    if extra:
        raise HipError("RESIDUAL: unknown key(s) %s (known: %s)" % (", ".join(map(str, extra)), ", ".join(sorted(known))))
    return Residual(block["LAYERS"])       # (the one known key: a non-empty block without unknown keys has it)
