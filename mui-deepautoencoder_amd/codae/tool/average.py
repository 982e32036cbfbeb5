"""An average of the iterates, kept by the update itself and used for evaluation: an exponential moving average (EMA) or the
equal-weight mean of the samples (Polyak / SWA) - the counterpart of codae_weight_average in include/codae_hip.h ("Weight average").

    t = the 1-based step of the update, p' = the parameter it has just produced, a = the average
    t < start or (t - start) % every != 0:  the step does not sample, the average is neither read nor written
    n = (t - start) / every                 the number of earlier samples; in float64:
    swa   w = 1 / (n + 1)
    ema   w = 1 when n == 0, else 1 - d_n,  d_n = debias ? min(decay, (1 + n) / (10 + n)) : decay
    w32 = float32(w);  a' = p' bit for bit when w32 == 1, else a' = a + w32 (p' - a) in fp32

The engine folds this into its update kernels (DaeEngine.set_weight_average, HipEmbeddingTrainer(weight_average=...)): the weight
is formed on the device from the step count it keeps there, so graph replay costs nothing.  WeightAverage carries the setting (as
the fp32 / int32 values of the C struct), tells the weight of a step (weight) and runs the same definition on its own (update): on
device tensors through codae_weight_average_update, on host tensors in torch ops - for loops that keep torch's optimizer.
"""
import math

import numpy as np

from ..hip import HipError

KINDS = {"off": 0, "ema": 1, "swa": 2}                                       # CODAE_AVG_* of include/codae_hip.h


def _count(name, v, lo):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) < 2 ** 31:
        raise HipError("weight average: %s must be an integer in [%d, 2^31), got %r" % (name, lo, v))
    return int(v)


class WeightAverage:
    """WeightAverage() = an EMA with decay 0.999, debiased, every step from the first | ("swa", start=1000, every=10) |
    ("ema", decay=0.99, debias=False) | ("off").  decay and debias are read by ema only.  debias caps the decay of the n-th
    update at (1 + n) / (10 + n), so that an average started on a fresh model forgets its start."""

    def __init__(self, kind="ema", decay=0.999, debias=True, start=1, every=1):
        if not isinstance(kind, str) or kind.lower() not in KINDS:
            raise HipError("weight average: unknown kind %r (known: %s)" % (kind, ", ".join(KINDS)))
        self.kind = kind.lower()
        if isinstance(decay, bool) or not isinstance(decay, (int, float, np.integer, np.floating)) or not math.isfinite(float(decay)):
            raise HipError("weight average: decay must be a finite number, got %r" % (decay,))
        self.decay = float(np.float32(decay))
        if not 0.0 <= self.decay < 1.0:
            raise HipError("weight average: decay %r outside [0, 1)" % (decay,))
        if not isinstance(debias, (bool, np.bool_)):
            raise HipError("weight average: debias must be true or false, got %r" % (debias,))
        self.debias = bool(debias)
        self.start = _count("start", start, 1)
        self.every = _count("every", every, 1)

    @property
    def is_default(self):
        """Off: the engine runs exactly what it runs without the setting."""
        return self.kind == "off"

    def __repr__(self):
        return "WeightAverage(%r, decay=%r, debias=%r, start=%d, every=%d)" % (self.kind, self.decay, self.debias, self.start, self.every)

    def weight(self, step):
        """w32 of the 1-based step as a Python float, or None when the step does not sample (or the kind is off)."""
        t = _count("step", step, 1)
        if self.kind == "off" or t < self.start or (t - self.start) % self.every:
            return None
        n = (t - self.start) // self.every
        if self.kind == "swa":
            w = 1.0 / float(n + 1)
        elif n == 0:
            w = 1.0
        else:
            d = min(self.decay, (1.0 + n) / (10.0 + n)) if self.debias else self.decay
            w = 1.0 - d
        return float(np.float32(w))

    def as_struct(self, avg=None):
        """The codae_weight_average struct; avg: the data pointer of the average (ctypes.c_void_p or None)."""
        from ..hip import WeightAverage as Struct
        return Struct(KINDS[self.kind], self.decay, int(self.debias), self.start, self.every, avg)

    def as_config(self):
        """The `HIP: WEIGHT_AVERAGE:` block weight_average_from_config reads back into an equal setting."""
        c = {"KIND": self.kind, "START": self.start, "EVERY": self.every}
        if self.kind == "ema":
            c.update(DECAY=self.decay, DEBIAS=self.debias)
        return c

    def update(self, avg, params, step):
        """avg <- the definition above with p' = params, in place; both fp32, contiguous, the same shape and device.  Device
        tensors run codae_weight_average_update, host tensors the same arithmetic in torch ops.  Returns avg."""
        import torch
        if avg.dtype != torch.float32 or params.dtype != torch.float32 or avg.shape != params.shape or avg.device != params.device \
                or not avg.is_contiguous() or not params.is_contiguous():
            raise HipError("weight average: avg and params must be contiguous fp32 tensors of one shape on one device")
        w = self.weight(step)
        if w is None or avg.numel() == 0:
            return avg
        if avg.is_cuda:
            import ctypes as C
            from ..hip import check, current_stream, lib, ptr
            st = self.as_struct(None)
            with torch.cuda.device(avg.device):
                check(lib().codae_weight_average_update(ptr(avg), ptr(params), avg.numel(), C.byref(st), int(step), current_stream()))
            return avg
        with torch.no_grad():
            if w == 1.0:
                return avg.copy_(params)
            return avg.add_((params - avg).mul_(w))


def weight_average_from_config(block, batches_per_epoch=None):
    """The `HIP: WEIGHT_AVERAGE:` block of the embedding script's config: {KIND: ema | swa, DECAY: 0.999, DEBIAS: true, START: 1,
    START_EPOCH: k, EVERY: 1}.  None / empty -> None.  START_EPOCH (1-based; not together with START) becomes START = (k - 1) *
    batches_per_epoch + 1, the first step of that epoch."""
    if not block:
        return None
    if not isinstance(block, dict):
        raise HipError("WEIGHT_AVERAGE must be a mapping, got %r" % (block,))
    known = {"KIND", "DECAY", "DEBIAS", "START", "START_EPOCH", "EVERY"}
    extra = sorted(set(map(str, block)) - known)
    if extra:
        raise HipError("WEIGHT_AVERAGE: unknown key(s) %s (known: %s)" % (", ".join(extra), ", ".join(sorted(known))))
    start = block.get("START", 1)
    if block.get("START_EPOCH") is not None:
        if "START" in block:
            raise HipError("WEIGHT_AVERAGE: give START or START_EPOCH, not both")
        if batches_per_epoch is None:
            raise HipError("WEIGHT_AVERAGE: START_EPOCH needs the number of batches per epoch")
        start = (_count("START_EPOCH", block["START_EPOCH"], 1) - 1) * _count("batches per epoch", batches_per_epoch, 1) + 1
    return WeightAverage(str(block.get("KIND", "ema")), decay=block.get("DECAY", 0.999), debias=block.get("DEBIAS", True), start=start,
                         every=block.get("EVERY", 1))
