"""Layer / RMS normalisation of hidden activations - the counterpart of codae_norm in include/codae_hip.h.

Layers are l = 0 .. L-1, h_0 is the corrupted input, norm_l and skip_l are 0 or 1:

    a_l = f_l act_l(W_l h_l + b_l)     (f_l: the dropout factor when layer l is dropped)
    s_l = a_l + skip_l h_l
    h_{l+1} = N(s_l) if norm_l else s_l                    (post-norm)             loss on h_L

N acts on one batch row x of width w = out[l], eps > 0:

    layer   mu = sum x / w,  v = sum (x - mu)^2 / w (biased),  r = 1 / sqrt(v + eps),  xhat = (x - mu) r
    rms     r = 1 / sqrt(sum x^2 / w + eps),                                        xhat = x r

There is no gain and no bias: every normalised layer is followed by a Linear that absorbs them (W diag(gamma), b + W beta), so
the parameter vector keeps its shape.  A norm is refused on the last layer (its output is the reconstruction) and behind any
activation but none, ReLU and LeakyReLU (the engine takes a derivative from the saved output, and after normalising that output
no longer determines it: a 1-bit mask carries it).  Unlike a skip it needs no equal widths: layer 0 and tapers are allowed.
It is part of the MODEL: training steps, eval_batch, complete, score_outfits and the averaged weights all run through it.

Norm carries the choice, resolves it against a stack (resolve), hands it to the HIP engine (DaeEngine.set_norm,
HipEmbeddingTrainer(norm=...)) and states the same network in whole-tensor torch ops with autograd (forward) for host tensors
and tests.
"""
import math

from ..hip import HipError
from .residual import ALLOWED_ACTS, _ACT_NAMES, _act_tuple, _apply_act

NORM_LAYER, NORM_RMS = 1, 2          # CODAE_NORM_* of include/codae_hip.h
KINDS = {"layer": NORM_LAYER, "rms": NORM_RMS}


class Norm:
    """Norm("layer") | Norm("rms", layers=[0, 2], eps=1e-6).  layers "hidden": every layer l <= L-2 with an allowed activation
    (none, ReLU, LeakyReLU), layer 0 included; a list: exactly those layers, each of which must qualify.  An empty list = off:
    the engine runs exactly what it runs without the argument."""

    def __init__(self, kind="layer", layers="hidden", eps=1e-5):
        if kind not in KINDS:
            raise HipError("norm: kind must be 'layer' or 'rms', got %r" % (kind,))
        self.kind = kind
        try:
            eps = float(eps)
        except (TypeError, ValueError):
            raise HipError("norm: eps must be a number, got %r" % (eps,))
        if not (math.isfinite(eps) and eps > 0.0):
            raise HipError("norm: eps must be finite and > 0, got %r" % (eps,))
        self.eps = eps
        if isinstance(layers, str):
            if layers != "hidden":
                raise HipError("norm: layers must be 'hidden' or a list of layer indices, got %r" % (layers,))
            self.layers = "hidden"
            return
        if not hasattr(layers, "__iter__"):
            raise HipError("norm: layers must be 'hidden' or a list of layer indices, got %r" % (layers,))
        out = []
        for v in layers:
            v = v.item() if hasattr(v, "item") else v
            if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                raise HipError("norm: layer indices must be integers >= 0, got %r" % (v,))
            out.append(int(v))
        if len(set(out)) != len(out):
            raise HipError("norm: a layer is listed twice in %r" % (out,))
        self.layers = tuple(sorted(out))

    def __repr__(self):
        return "Norm(%r, layers=%r, eps=%r)" % (self.kind, "hidden" if self.layers == "hidden" else list(self.layers), self.eps)

    @property
    def is_off(self):
        return self.layers == ()

    @property
    def kind_id(self):
        return KINDS[self.kind]

    @staticmethod
    def refusal(l, n_layers, acts):
        """Why layer l of a stack of n_layers takes no norm, or None."""
        if l >= n_layers:
            return "layer %d: the stack has %d layers" % (l, n_layers)
        if l == n_layers - 1:
            return "layer %d: the last layer's output is the reconstruction and takes no norm" % l
        if acts[l][0] not in ALLOWED_ACTS:
            return "layer %d: a normalised layer's activation must be none, ReLU or LeakyReLU (got %s)" % (
                l, _ACT_NAMES.get(acts[l][0], acts[l][0]))
        return None

    def resolve(self, in_features, out_features, activation):
        """The L flags (0 / 1) of this choice on a stack: in_features / out_features per layer (any widths), activation per layer
        (a bool = ReLU or none, a CODAE_ACT_* kind, or the engine's (kind, p0, p1, p2)).  A listed layer that cannot take a norm
        raises HipError naming the layer and the reason; "hidden" takes the layers that can."""
        L = len(in_features)
        if len(out_features) != L or len(activation) != L:
            raise HipError("norm: %d input widths, %d output widths, %d activations" % (L, len(out_features), len(activation)))
        acts = [_act_tuple(a) for a in activation]
        if self.layers == "hidden":
            return [1 if self.refusal(l, L, acts) is None else 0 for l in range(L)]
        flags = [0] * L
        for l in self.layers:
            why = self.refusal(l, L, acts)
            if why is not None:
                raise HipError("norm: " + why)
            flags[l] = 1
        return flags

    def normalise(self, s):
        """N of the definition on the last axis of a torch tensor, in its own dtype (autograd works through it)."""
        if self.kind == "layer":
            mu = s.mean(dim=-1, keepdim=True)
            c = s - mu
            return c / (c * c).mean(dim=-1, keepdim=True).add(self.eps).sqrt()
        return s / (s * s).mean(dim=-1, keepdim=True).add(self.eps).sqrt()

    def forward(self, x, weights, biases, activation, residual=None, dropout_factors=None):
        """h_L of the definition above in whole-tensor torch ops (autograd works through it).  weights[l]: [out, in], biases[l]:
        [out]; activation as resolve takes it; residual: None or a codae.tool.Residual (the skips of the same stack);
        dropout_factors: None, or per layer None / a [B, out[l]] tensor of factors that multiplies a_l."""
        L = len(weights)
        acts = [_act_tuple(a) for a in activation]
        ins, outs = [int(w.shape[1]) for w in weights], [int(w.shape[0]) for w in weights]
        flags = self.resolve(ins, outs, acts)
        skips = residual.resolve(ins, outs, acts) if residual is not None else [0] * L
        h = x
        for l in range(L):
            a = _apply_act(acts[l], h @ weights[l].t() + biases[l])
            if dropout_factors is not None and l < len(dropout_factors) and dropout_factors[l] is not None:
                a = a * dropout_factors[l]
            s = a + h if skips[l] else a
            h = self.normalise(s) if flags[l] else s
        return h


def meta_record(norm, layers):
    """What a checkpoint's meta keeps under "norm" for a trainer whose norm resolved to `layers`: {kind, eps, layers}, or None
    when no layer is normalised (the key is then not written at all)."""
    if norm is None or not layers:
        return None
    return {"kind": norm.kind, "eps": float(norm.eps), "layers": [int(l) for l in layers]}


def meta_mismatch(meta, norm, layers):
    """The checkpoint's structure check: None when the file's record (meta["norm"]: {kind, eps, layers}; a file without the key
    has no norm) is the trainer's (`norm` resolved to `layers`), else the sentence that says how they differ."""
    in_file = meta.get("norm") or None
    mine = meta_record(norm, layers)

    def say(r):
        return "none" if r is None else "%s norm (eps %r) on layers %s" % (r["kind"], float(r["eps"]), sorted(int(l) for l in r["layers"]))
    if in_file is None and mine is None:
        return None
    if in_file is not None and mine is not None and in_file.get("kind") == mine["kind"] and float(in_file.get("eps", 0.0)) == mine["eps"] \
            and sorted(int(l) for l in in_file.get("layers", ())) == sorted(mine["layers"]):
        return None
    return "the file was written with norm: %s, this trainer has norm: %s" % (say(in_file), say(mine))


def norm_from_meta(meta):
    """The Norm a checkpoint's record describes, or None."""
    r = meta.get("norm") or None
    if r is None:
        return None
    return Norm(r["kind"], layers=[int(l) for l in r["layers"]], eps=float(r["eps"]))


def norm_from_config(block):
    """The `HIP: NORM:` block of the embedding script's config: {KIND: layer | rms, LAYERS: hidden | [0, 1, ..], EPS: 1e-5}.
    None / empty -> None."""
    if not block:
        return None
    if not isinstance(block, dict):
        raise HipError("NORM must be a mapping with KIND, LAYERS and EPS, got %r" % (block,))
    known = {"KIND", "LAYERS", "EPS"}
    extra = sorted(set(block) - known, key=str)
    if extra:
        raise HipError("NORM: unknown key(s) %s (known: %s)" % (", ".join(map(str, extra)), ", ".join(sorted(known))))
    return Norm(str(block.get("KIND", "layer")).lower(), layers=block.get("LAYERS", "hidden"), eps=block.get("EPS", 1e-5))
