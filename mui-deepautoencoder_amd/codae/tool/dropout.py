"""Hidden dropout (Srivastava et al. 2014, the inverted form of torch.nn.Dropout) between the Linears of the fused training
step - the counterpart of codae_dropout in include/codae_hip.h.

The output of layer l (0 <= l <= L - 2; the last layer's output is never dropped) is multiplied by a factor that is a pure
function of (seed, dataset row, column, optimizer step, layer): Philox4x32-10 with key = (seed & 0xffffffff, seed >> 32) and
counter = (column // 4, dataset row, step, 1 + layer); word column % 4 belongs to the column.  With T = floor(p 2^32) the
element is dropped iff its word is below T:

    f = 0 if dropped else float32(1 / (1 - p))          forward: a <- a * f          backward: d <- d * f

The fourth counter word keeps the stream apart from the input noise (which uses 0) and from the other layers under the same
seed.  A row is dropped the same wherever it lands in a batch and on whichever data-parallel rank.  Training steps only:
eval_batch and complete never drop.

HiddenDropout carries the parameters (as fp32, the type the C side sees), hands them to the HIP engine
(DaeEngine.set_hidden_dropout, HipEmbeddingTrainer(hidden_dropout=...)) and states the factor in plain numpy / torch ops
(factor) for host tensors and drop-in loops.
"""
import math

import numpy as np

from ..hip import HipError
from .noise import philox4x32_10


def _prob(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise HipError("hidden dropout: %s must be a number, got %r" % (name, v))
    v = float(v)
    if not math.isfinite(v):
        raise HipError("hidden dropout: %s = %r is not finite" % (name, v))
    v = float(np.float32(v))
    if not 0.0 <= v < 1.0:
        raise HipError("hidden dropout: %s = %r outside [0, 1)" % (name, v))
    return v


class HiddenDropout:
    """HiddenDropout(0.5) | HiddenDropout([0.5, 0.0, 0.25], seed=3).  p: one probability for every hidden output, or one per
    hidden output (L - 1 values, resolved against the engine's depth when it is set); seed: 64-bit stream id.  All zeros = off:
    the engine runs exactly what it runs without dropout."""

    def __init__(self, p, seed=0):
        if isinstance(p, (str, bytes)):
            raise HipError("hidden dropout: p must be a number or a sequence of numbers, got %r" % (p,))
        if hasattr(p, "__iter__"):
            self.p = tuple(_prob("p[%d]" % i, v.item() if hasattr(v, "item") else v) for i, v in enumerate(p))
            if not self.p:
                raise HipError("hidden dropout: p is empty")
        else:
            self.p = _prob("p", p)
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
            raise HipError("hidden dropout: seed must be an integer in [0, 2^64), got %r" % (seed,))
        self.seed = int(seed)

    def __repr__(self):
        return "HiddenDropout(%r, seed=%d)" % (list(self.p) if isinstance(self.p, tuple) else self.p, self.seed)

    @property
    def is_identity(self):
        return all(v == 0.0 for v in (self.p if isinstance(self.p, tuple) else (self.p,)))

    def per_layer(self, n_layers):
        """The L - 1 probabilities (fp32 values as Python floats) of a stack of n_layers Linears."""
        n = int(n_layers) - 1
        if isinstance(self.p, tuple):
            if len(self.p) != n:
                raise HipError("hidden dropout: %d probabilities for %d hidden outputs (%d layers)" % (len(self.p), n, n + 1))
            return list(self.p)
        return [self.p] * n

    def p_of(self, layer, n_layers=None):
        if isinstance(self.p, tuple):
            if n_layers is not None:
                return self.per_layer(n_layers)[layer]
            if not 0 <= layer < len(self.p):
                raise HipError("hidden dropout: layer %d outside [0, %d)" % (layer, len(self.p)))
            return self.p[layer]
        return self.p

    @staticmethod
    def threshold(p):
        """T = floor(p 2^32) of the fp32 probability p: an element is dropped iff its word is below T."""
        return int(math.floor(float(np.float32(p)) * 4294967296.0))

    @staticmethod
    def scale(p):
        """float32(1 / (1 - p)), the factor of a kept element."""
        return np.float32(1.0 / (1.0 - float(np.float32(p))))

    def words(self, rows, layer, width, step):
        """uint32 [B, width]: the Philox word of every element of layer `layer`'s output for dataset rows `rows`."""
        rows = np.asarray(rows, dtype=np.int64).reshape(-1, 1)
        groups = np.arange((int(width) + 3) // 4, dtype=np.int64).reshape(1, -1)
        r = philox4x32_10((groups, rows & 0xFFFFFFFF, np.int64(step) & 0xFFFFFFFF, 1 + int(layer)),
                          (self.seed & 0xFFFFFFFF, self.seed >> 32))
        return np.stack(r, axis=-1).reshape(rows.shape[0], -1)[:, :int(width)]

    def factor(self, rows, layer, width, step, n_layers=None):
        """fp32 [B, width]: 0 where the element is dropped, float32(1 / (1 - p)) elsewhere.  rows: the dataset index of every
        batch row (a torch tensor gives a torch tensor on its device, anything else a numpy array); layer: whose output;
        step: the 1-based optimizer step."""
        for name, v in (("layer", layer), ("width", width), ("step", step)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < 2 ** 31:
                raise HipError("HiddenDropout.factor: %s must be an integer in [0, 2^31), got %r" % (name, v))
        p = self.p_of(int(layer), n_layers)
        as_torch = None
        if hasattr(rows, "detach"):
            as_torch = rows.device
            rows = rows.detach().cpu().numpy()
        w = self.words(rows, int(layer), int(width), int(step))
        f = np.where(w.astype(np.uint64) < np.uint64(self.threshold(p)), np.float32(0), self.scale(p)).astype(np.float32)
        if as_torch is not None:
            import torch
            return torch.from_numpy(f).to(as_torch)
        return f


def hidden_dropout_from_config(block):
    """The `HIP: HIDDEN_DROPOUT:` block of the embedding script's config: {P: 0.5 | [.. one per hidden output ..], SEED: 3}.
    None / empty -> None."""
    if not block:
        return None
    if not isinstance(block, dict):
        raise HipError("HIDDEN_DROPOUT must be a mapping with a P, got %r" % (block,))
    known = {"P", "SEED"}
    extra = sorted(set(block) - known, key=str)
    if extra:
        raise HipError("HIDDEN_DROPOUT: unknown key(s) %s (known: %s)" % (", ".join(map(str, extra)), ", ".join(sorted(known))))
    if "P" not in block:
        raise HipError("HIDDEN_DROPOUT: P is missing")
    return HiddenDropout(block["P"], seed=block.get("SEED", 0))
