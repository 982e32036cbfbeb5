"""Mixed-variable criterion of the fused step: the reference's CombinedCriterion(reduction="mean") for rows made of variables
(tabular data: one-hot and numeric columns) - the counterpart of codae_variable_loss in include/codae_hip.h ("Mixed-variable
criterion").

    L = (1 / n_var) sum_v w_v L_v
    regression      L_v = sqrt(mean over the variable's [B, size] slice of (x - y)^2)
    classification  L_v = mean_b NLL(log_softmax(y_slice), t_b),  t_b = the first maximum of the clean x slice

VariableLoss carries the table (position, size, type, weight per variable; disjoint, ascending, covering every column), hands it
to the HIP engine (DaeEngine.set_variable_loss, HipEmbeddingTrainer(criterion=VariableLoss(...))), states the same loss in plain
torch ops with autograd for host tensors and drop-in loops (loss), and reads a reconstruction per variable (predict).
"""
import ctypes as C
import math

import numpy as np

from ..hip import HipError

TYPES = {"regression": 0, "classification": 1}      # CODAE_VAR_* of include/codae_hip.h
MAX_VARS = 65536                                    # CODAE_VAR_MAX


class VariableLoss:
    """VariableLoss(arch, weight=None): arch is the list of {"position", "size", "type"} dicts MixedVariableDataset.arch and
    CombinedCriterion use, type "regression" or "classification"; weight one number per variable (default: all 1)."""

    def __init__(self, arch, weight=None):
        if not isinstance(arch, (list, tuple)) or len(arch) < 1:
            raise HipError("variable loss: arch must be a non-empty list of variables, got %r" % (arch,))
        if len(arch) > MAX_VARS:
            raise HipError("variable loss: %d variables, at most %d" % (len(arch), MAX_VARS))
        self.arch = []
        nxt = 0
        for i, v in enumerate(arch):
            try:
                p, s, t = v["position"], v["size"], v["type"]
            except (KeyError, TypeError, IndexError):
                raise HipError("variable loss: variable %d needs position, size and type, got %r" % (i, v))
            if t not in TYPES:
                raise HipError("variable loss: variable %d has unknown type %r (known: %s)" % (i, t, ", ".join(TYPES)))
            if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or s < 1:
                raise HipError("variable loss: variable %d has size %r (must be an integer >= 1)" % (i, s))
            if isinstance(p, bool) or not isinstance(p, (int, np.integer)):
                raise HipError("variable loss: variable %d has position %r (must be an integer)" % (i, p))
            if p < nxt:
                raise HipError("variable loss: variable %d at position %d overlaps the one before it (which ends at %d)" % (i, p, nxt))
            if p > nxt:
                raise HipError("variable loss: columns [%d, %d) are covered by no variable" % (nxt, p))
            nxt = int(p) + int(s)
            self.arch.append({"position": int(p), "size": int(s), "type": t})
        self.io = nxt
        if weight is None:
            w = np.ones(len(self.arch), dtype=np.float32)
        else:
            try:
                w = np.asarray(weight, dtype=np.float64).reshape(-1)
            except (TypeError, ValueError):
                raise HipError("variable loss: weight must be one number per variable, got %r" % (weight,))
            if w.size != len(self.arch):
                raise HipError("variable loss: %d weights for %d variables" % (w.size, len(self.arch)))
            for i, x in enumerate(w):
                if not math.isfinite(x) or abs(x) > 3.4e38 or x < 0:
                    raise HipError("variable loss: weight %d = %r must be finite and >= 0" % (i, float(x)))
            w = w.astype(np.float32)
        self.weight = w

    is_default = False

    @property
    def n_var(self):
        return len(self.arch)

    def __repr__(self):
        return "VariableLoss(%d variables over %d columns)" % (self.n_var, self.io)

    def describe(self):
        """What a checkpoint's informational options record."""
        return {"n_var": self.n_var, "io": self.io, "types": [v["type"] for v in self.arch], "sizes": [v["size"] for v in self.arch],
                "weight": [float(x) for x in self.weight]}

    def as_struct(self, ws=None):
        """The codae_variable_loss of this table; ws: the uint8 device tensor it borrows (DaeEngine.set_variable_loss allocates
        it).  The struct points into host arrays kept on it (`_keep`)."""
        from ..hip import VariableLossStruct
        n = self.n_var
        pos = (C.c_int32 * n)(*[v["position"] for v in self.arch])
        size = (C.c_int32 * n)(*[v["size"] for v in self.arch])
        typ = (C.c_int32 * n)(*[TYPES[v["type"]] for v in self.arch])
        w = (C.c_float * n)(*[float(x) for x in self.weight])
        st = VariableLossStruct(n, 0, pos, size, typ, w, None if ws is None else C.c_void_p(ws.data_ptr()), 0 if ws is None else int(ws.numel()))
        st._keep = (pos, size, typ, w, ws)
        return st

    def loss(self, x, y):
        """The criterion in torch ops (autograd through y): a 0-dim tensor.  x: the clean rows, y: the reconstruction, [B, io]."""
        import torch
        if x.dim() != 2 or x.shape != y.shape or int(x.shape[1]) != self.io:
            raise HipError("variable loss: x %s / y %s are not [B, %d]" % (tuple(x.shape), tuple(y.shape), self.io))
        total = None
        for v, w in zip(self.arch, self.weight):
            p, s = v["position"], v["size"]
            xs, ys = x[:, p:p + s], y[:, p:p + s]
            if v["type"] == "regression":
                li = torch.sqrt(torch.nn.functional.mse_loss(ys, xs))
            else:
                li = torch.nn.functional.nll_loss(torch.log_softmax(ys, dim=1), xs.max(dim=1)[1])
            li = li * float(w)
            total = li if total is None else total + li
        return total / self.n_var

    def predict(self, y):
        """Per variable: the regression columns [B, size] as they are; for a classification variable (argmax index [B], softmax
        probabilities [B, size])."""
        import torch
        if y.dim() != 2 or int(y.shape[1]) != self.io:
            raise HipError("variable loss: y %s is not [B, %d]" % (tuple(y.shape), self.io))
        out = []
        for v in self.arch:
            ys = y[:, v["position"]:v["position"] + v["size"]]
            if v["type"] == "regression":
                out.append(ys)
            else:
                out.append((ys.argmax(dim=1), torch.softmax(ys, dim=1)))
        return out
