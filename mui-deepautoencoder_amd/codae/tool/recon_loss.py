"""Training criterion of the fused step: the mean squared error of the reference script, or L1 / SmoothL1 / Huber / a per-slot
cosine - the counterpart of codae_recon_loss in include/codae_hip.h ("Training criterion").

    d = x - y, inv_n = 1 / (rows * io), rows = the GLOBAL batch, w = the emphasis weight (1 without emphasis)
    mse          sum w d^2 inv_n
    l1           sum w |d| inv_n
    smooth_l1    sum w (|d| < beta ? d^2 / (2 beta) : |d| - beta / 2) inv_n
    huber        sum w (|d| <= delta ? d^2 / 2 : delta (|d| - delta / 2)) inv_n
    slot_cosine  sum_{b,s} W (1 - cos(x_s, y_s)) / (rows S) + mse_weight sum w d^2 inv_n,  W = mean of w over the slot's columns

The stack fills a blanked slot with an embedding that is then ranked by cosine (RankingLoss, ComplementRetriever.topk,
HipEmbeddingTrainer.complete): slot_cosine trains what retrieval measures, mse_weight keeps the lengths anchored.

ReconstructionLoss carries the parameters (as fp32, the type of the C struct), hands them to the HIP engine
(DaeEngine.set_recon_loss, HipEmbeddingTrainer(criterion=...)) and states the same loss in plain torch ops with autograd for
the drop-in loops (loss); it composes with LossEmphasis.weights(...) through `weight=`.
"""
import math

import numpy as np

from ..hip import HipError

KINDS = {"mse": 0, "l1": 1, "smooth_l1": 2, "huber": 3, "slot_cosine": 4}      # CODAE_LOSS_* of include/codae_hip.h
COS_EPS = 1e-8                                                                  # CODAE_COS_EPS
MAX_SLOTS = 128


def _number(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise HipError("training criterion: %s must be a number, got %r" % (name, v))
    v = float(v)
    if not math.isfinite(v) or abs(v) > 3.4e38:
        raise HipError("training criterion: %s = %r is not finite" % (name, v))
    return float(np.float32(v))


class ReconstructionLoss:
    """ReconstructionLoss() | ("l1") | ("smooth_l1", beta=0.5) | ("huber", delta=1.0) | ("slot_cosine", mse_weight=0.1).
    beta goes with smooth_l1 and delta with huber (default 1.0, torch's), mse_weight with slot_cosine only.  The default is the
    mean squared error: `is_default`, and the engine runs exactly what it runs without a criterion."""

    def __init__(self, kind="mse", beta=None, delta=None, mse_weight=0.0):
        if not isinstance(kind, str) or kind.lower() not in KINDS:
            raise HipError("training criterion: unknown kind %r (known: %s)" % (kind, ", ".join(KINDS)))
        self.kind = kind.lower()
        if beta is not None and self.kind != "smooth_l1":
            raise HipError("training criterion: beta goes with smooth_l1, not %s" % self.kind)
        if delta is not None and self.kind != "huber":
            raise HipError("training criterion: delta goes with huber, not %s" % self.kind)
        self.beta = self.delta = None
        if self.kind == "smooth_l1":
            self.beta = _number("beta", 1.0 if beta is None else beta)
            if not self.beta > 0.0:
                raise HipError("training criterion: smooth_l1 beta %r must be > 0" % self.beta)
        if self.kind == "huber":
            self.delta = _number("delta", 1.0 if delta is None else delta)
            if not self.delta > 0.0:
                raise HipError("training criterion: huber delta %r must be > 0" % self.delta)
        self.mse_weight = _number("mse_weight", mse_weight)
        if self.mse_weight < 0.0:
            raise HipError("training criterion: mse_weight %r must be >= 0" % self.mse_weight)
        if self.mse_weight != 0.0 and self.kind != "slot_cosine":
            raise HipError("training criterion: mse_weight %r goes with slot_cosine only" % self.mse_weight)

    def __repr__(self):
        extra = "".join(", %s=%r" % (k, getattr(self, k)) for k in ("beta", "delta") if getattr(self, k) is not None)
        if self.mse_weight:
            extra += ", mse_weight=%r" % self.mse_weight
        return "ReconstructionLoss(%r%s)" % (self.kind, extra)

    @property
    def is_default(self):
        return self.kind == "mse"

    @property
    def param(self):
        return self.beta if self.kind == "smooth_l1" else (self.delta if self.kind == "huber" else 0.0)

    @staticmethod
    def _check_slots(n_slots, io=None):
        if n_slots is None or isinstance(n_slots, bool) or not isinstance(n_slots, (int, np.integer)) or int(n_slots) < 1:
            raise HipError("training criterion: slot_cosine needs n_slots >= 1, got %r" % (n_slots,))
        if io is not None and int(io) % int(n_slots):
            raise HipError("training criterion: n_slots %d does not divide io %d" % (int(n_slots), int(io)))
        return int(n_slots)

    def as_struct(self, n_slots=None):
        """The codae_recon_loss of this criterion; slot_cosine needs the number of slots."""
        from ..hip import ReconLoss
        S = 0
        if self.kind == "slot_cosine":
            S = self._check_slots(n_slots)
            if S > MAX_SLOTS:
                raise HipError("training criterion: slot_cosine takes at most %d slots, got %d" % (MAX_SLOTS, S))
        return ReconLoss(KINDS[self.kind], self.param, self.mse_weight, S)

    # ---- a dense batch (drop-in loops) ---------------------------------------------------------------
    def loss(self, input, output, weight=None, n_slots=None, global_rows=None):
        """The criterion of the dense batch in plain torch ops (differentiable in `output`), on host or HIP tensors.  input:
        the clean rows [B, io]; weight [B, io]: the element weights (LossEmphasis.weights(corrupted)), default 1; n_slots: S, for
        slot_cosine; global_rows: rows of the whole minibatch over all ranks (default: this batch's)."""
        import torch
        if input.dim() != 2 or input.shape != output.shape:
            raise HipError("ReconstructionLoss.loss: input %s and output %s must be equal [B, io] shapes" % (tuple(input.shape), tuple(output.shape)))
        if weight is not None and tuple(weight.shape) != tuple(input.shape):
            raise HipError("ReconstructionLoss.loss: weight shape %s, batch shape %s" % (tuple(weight.shape), tuple(input.shape)))
        B, io = input.shape
        rows = float(B if global_rows is None else global_rows)
        w = None if weight is None else weight.to(device=output.device, dtype=output.dtype)
        d = input - output

        def wsum(t):
            return (t if w is None else w * t).sum()

        if self.kind == "mse":
            return wsum(d * d) / (rows * io)
        if self.kind == "l1":
            return wsum(d.abs()) / (rows * io)
        if self.kind == "smooth_l1":
            a = d.abs()
            return wsum(torch.where(a < self.beta, 0.5 * d * d / self.beta, a - 0.5 * self.beta)) / (rows * io)
        if self.kind == "huber":
            a = d.abs()
            return wsum(torch.where(a <= self.delta, 0.5 * d * d, self.delta * (a - 0.5 * self.delta))) / (rows * io)
        S = self._check_slots(n_slots, io)
        E = io // S
        x3, y3 = input.reshape(B, S, E), output.reshape(B, S, E)
        nx = x3.norm(dim=-1).clamp_min(COS_EPS)
        ny = y3.norm(dim=-1).clamp_min(COS_EPS)
        cos = (x3 * y3).sum(dim=-1) / (nx * ny)
        term = 1.0 - cos
        if w is not None:
            term = w.reshape(B, S, E).mean(dim=-1) * term
        out = term.sum() / (rows * S)
        if self.mse_weight:
            out = out + self.mse_weight * wsum(d * d) / (rows * io)
        return out


def recon_loss_from_config(block):
    """The `HIP: CRITERION:` block of the embedding script's config: {KIND: slot_cosine, MSE_WEIGHT: 0.1} | {KIND: smooth_l1,
    BETA: 0.5} | {KIND: huber, DELTA: 1.0} | {KIND: l1} | {KIND: mse}.  None / empty -> None."""
    if not block:
        return None
    if not isinstance(block, dict):
        raise HipError("CRITERION must be a mapping, got %r" % (block,))
    known = {"KIND", "BETA", "DELTA", "MSE_WEIGHT"}
    extra = sorted(set(block) - known, key=str)
    if extra:
        raise HipError("CRITERION: unknown key(s) %s (known: %s)" % (", ".join(map(str, extra)), ", ".join(sorted(known))))
    if "KIND" not in block:
        raise HipError("CRITERION: KIND is missing (one of %s)" % ", ".join(KINDS))
    return ReconstructionLoss(block["KIND"], beta=block.get("BETA"), delta=block.get("DELTA"), mse_weight=block.get("MSE_WEIGHT", 0.0))
