"""Emphasised denoising loss (Vincent et al. 2010, section 4.3): the training loss weights the elements the corruption touched
and the ones it left alone differently - the counterpart of codae_emphasis in include/codae_hip.h.

    w(b, c) = column_weight[c] * (alpha if corrupted(b, c) else beta)
    L       = sum w (x - y)^2 / (rows * io)          rows = the GLOBAL batch: no renormalisation by the weights
    dL/dy   = 2 w (y - x) / (rows * io)

corrupted = blanked by the Corrupter's whole-slot mask OR replaced by masking / salt-and-pepper input noise (Gaussian noise
replaces nothing).  The metric sums of the engine (epoch_sums) stay unweighted, evaluation is never weighted.

LossEmphasis carries the parameters (as fp32, the type of the C struct), hands them to the HIP engine
(DaeEngine.set_loss_emphasis, HipEmbeddingTrainer(loss_emphasis=...)) and states the same loss in plain torch ops with
autograd for the drop-in loops (loss).
"""
import math

import numpy as np

from ..hip import HipError


def _weight(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise HipError("loss emphasis: %s must be a number, got %r" % (name, v))
    v = float(v)
    if not math.isfinite(v) or abs(v) > 3.4e38:
        raise HipError("loss emphasis: %s = %r is not finite" % (name, v))
    v = float(np.float32(v))
    if v < 0.0:
        raise HipError("loss emphasis: %s = %r must be >= 0" % (name, v))
    return v


def _weights(name, seq):
    if isinstance(seq, (str, bytes)) or not hasattr(seq, "__iter__"):
        raise HipError("loss emphasis: %s must be a sequence of numbers, got %r" % (name, seq))
    out = [_weight("%s[%d]" % (name, i), v.item() if hasattr(v, "item") else v) for i, v in enumerate(seq)]
    if not out:
        raise HipError("loss emphasis: %s is empty" % name)
    return tuple(out)


class LossEmphasis:
    """LossEmphasis(alpha=3.0, beta=1.0) | LossEmphasis(slot_weight=[0.5, 1, 2]) | LossEmphasis(column_weight=[...io values...]).
    alpha weights a corrupted element, beta an untouched one; slot_weight (one value per slot, expanded to the slot's
    columns once the number of slots is known) and column_weight (one per column) exclude each other.  All defaults = the
    plain mean squared error: `is_identity`, and the engine runs exactly what it runs without emphasis."""

    def __init__(self, alpha=1.0, beta=1.0, slot_weight=None, column_weight=None):
        self.alpha = _weight("alpha", alpha)
        self.beta = _weight("beta", beta)
        if self.alpha + self.beta <= 0.0:
            raise HipError("loss emphasis: alpha + beta must be > 0 (every element would weigh nothing)")
        if slot_weight is not None and column_weight is not None:
            raise HipError("loss emphasis: give slot_weight or column_weight, not both")
        self.slot_weight = None if slot_weight is None else _weights("slot_weight", slot_weight)
        self.column_weight = None if column_weight is None else _weights("column_weight", column_weight)

    def __repr__(self):
        extra = "".join(", %s=%r" % (k, list(getattr(self, k))) for k in ("slot_weight", "column_weight") if getattr(self, k) is not None)
        return "LossEmphasis(alpha=%r, beta=%r%s)" % (self.alpha, self.beta, extra)

    @property
    def is_identity(self):
        return self.alpha == 1.0 and self.beta == 1.0 and self.slot_weight is None and self.column_weight is None

    def column_weights(self, io, n_slots=None):
        """float32 numpy [io] of the per-column factor, or None when there is none."""
        io = int(io)
        if self.column_weight is not None:
            if len(self.column_weight) != io:
                raise HipError("loss emphasis: %d column weights for %d columns" % (len(self.column_weight), io))
            return np.asarray(self.column_weight, dtype=np.float32)
        if self.slot_weight is None:
            return None
        S = len(self.slot_weight)
        if n_slots is not None and int(n_slots) != S:
            raise HipError("loss emphasis: %d slot weights for %d slots" % (S, int(n_slots)))
        if io % S:
            raise HipError("loss emphasis: %d slot weights do not divide %d columns" % (S, io))
        return np.repeat(np.asarray(self.slot_weight, dtype=np.float32), io // S)

    def weights(self, corrupted, n_slots=None):
        """w [B, io] fp32 on corrupted's device: column weight * (alpha where corrupted != 0, else beta)."""
        import torch
        c = corrupted != 0
        w = torch.where(c, torch.tensor(self.alpha, dtype=torch.float32, device=c.device),
                        torch.tensor(self.beta, dtype=torch.float32, device=c.device))
        cw = self.column_weights(c.shape[-1], n_slots)
        if cw is not None:
            w = w * torch.from_numpy(cw).to(c.device)
        return w

    # ---- a dense batch (drop-in loops) ---------------------------------------------------------------
    def loss(self, input, output, fmask, corrupted=None, global_rows=None, n_slots=None):
        """The emphasised loss of the dense batch in plain torch ops (differentiable in `output`), on host or HIP tensors:
        sum w (input - output)^2 / (rows * io).  fmask [B, io]: 0 = blanked (Corrupter.get_masks); corrupted [B, io]: non-zero
        = touched by the corruption, default 1 - fmask (give `fmask == 0 | noise hit` when input noise replaces elements);
        global_rows: rows of the whole minibatch over all ranks (default: this batch's)."""
        if input.dim() != 2 or input.shape != output.shape:
            raise HipError("LossEmphasis.loss: input %s and output %s must be equal [B, io] shapes" % (tuple(input.shape), tuple(output.shape)))
        if corrupted is None:
            if fmask is None:
                raise HipError("LossEmphasis.loss: needs fmask or corrupted")
            corrupted = fmask == 0
        if tuple(corrupted.shape) != tuple(input.shape):
            raise HipError("LossEmphasis.loss: corrupted shape %s, batch shape %s" % (tuple(corrupted.shape), tuple(input.shape)))
        w = self.weights(corrupted.to(output.device), n_slots).to(output.dtype)
        rows = input.shape[0] if global_rows is None else global_rows
        d = input - output
        return (w * d * d).sum() / (float(rows) * input.shape[1])


def loss_emphasis_from_config(block):
    """The `HIP: LOSS_EMPHASIS:` block of the embedding script's config: {ALPHA: 3.0, BETA: 1.0, SLOT_WEIGHT: [..] |
    COLUMN_WEIGHT: [..]}.  None / empty -> None."""
    if not block:
        return None
    if not isinstance(block, dict):
        raise HipError("LOSS_EMPHASIS must be a mapping, got %r" % (block,))
    known = {"ALPHA", "BETA", "SLOT_WEIGHT", "COLUMN_WEIGHT"}
    extra = sorted(set(block) - known, key=str)
    if extra:
        raise HipError("LOSS_EMPHASIS: unknown key(s) %s (known: %s)" % (", ".join(map(str, extra)), ", ".join(sorted(known))))
    return LossEmphasis(alpha=block.get("ALPHA", 1.0), beta=block.get("BETA", 1.0), slot_weight=block.get("SLOT_WEIGHT"),
                        column_weight=block.get("COLUMN_WEIGHT"))
