"""Optimizer and learning-rate schedule of the fused step's update: Adam (the reference script's line), AdamW, SGD with
(Nesterov) momentum, AMSGrad, and a warm-up + cosine / linear / step schedule - the counterpart of codae_optimizer in
include/codae_hip.h ("Optimizer and schedule").

    t = the 1-based step, coef = the clip coefficient, lr, wd, b1, b2, eps = the trainer's hyperparameters
    w(t)  = W > 0 and t <= W ? t / W : 1                      q(t) = clamp((t - W) / (T - W), 0, 1)
    f(t)  = w(t) * { constant: 1 | cosine: min_factor + (1 - min_factor) (1 + cos(pi q)) / 2
                     linear: 1 - (1 - min_factor) q | step: gamma ^ floor((t - 1) / period) }
    lr_t  = float32(lr * f(t))                                (torch's LambdaLR with lambda(t - 1); past T the end value stays)
    adam   g' = g coef + wd p;  m' = b1 m + (1 - b1) g';  v' = b2 v + (1 - b2) g'^2;  d = v'
    adamw  g' = g coef;  p1 = p (1 - lr_t wd);  m', v' from g';  d = v'
      amsgrad: vmax' = maximum(vmax, v') (NaN stays);  d = vmax'
           p' = (p | p1) - lr_t / (1 - b1^t) m' / (sqrt(d) / sqrt(1 - b2^t) + eps)
    sgd    g' = g coef + wd p;  m' = mu m + g';  u = nesterov ? g' + mu m' : m';  p' = p - lr_t u

Layer-wise trust ratios (include/codae_hip.h, "Layer-wise trust ratios"): per weight matrix P = ||p||, U = ||u||, G = ||g'||, squares
in fp32, sums in double; wd' = wd in a matrix, decay_bias ? wd : 0 in the bias block, whose ratio is 1; every fp32 operation rounded
on its own, in the order written:
    lamb   g' = g coef;  m' = b1 m + (1 - b1) g';  v' = b2 v + ((1 - b2) g') g'
           u = (m' / (sqrt(v') float32(1 / sqrt(1 - b2^t)) + eps)) float32(1 / (1 - b1^t)) + wd' p
           phi = P > 0 and U > 0 ? P / U : 1, min(phi, trust_clip) when trust_clip > 0;  p' = p - (lr_t float32(phi)) u
    lars   g' = g coef;  lambda = P > 0 and G > 0 ? trust_coef P / (G + wd P + eps) : 1, clipped alike
           d = float32(lambda) (g' + wd' p);  m' = mu m + d;  u = nesterov ? d + mu m' : m';  p' = p - lr_t u

The engine evaluates f(t) on the device from the step count it keeps there, so a schedule costs a replayed graph nothing: the
learning rate the trainer holds stays the base lr.  Optimizer carries the setting (as the fp32 / int32 values of the C struct), hands
it to the HIP engine (DaeEngine.set_optimizer, HipEmbeddingTrainer(optimizer=...)), tells the scheduled rate for logs (lr_at) and
states the same update in plain torch ops for host tensors and the drop-in loops (step).
"""
import math

import numpy as np

from ..hip import HipError

KINDS = {"adam": 0, "adamw": 1, "sgd": 2, "lamb": 3, "lars": 4}                                # CODAE_OPT_* of include/codae_hip.h
SCHEDULES = {"constant": 0, "cosine": 1, "linear": 2, "step": 3}            # CODAE_SCHED_*


def _number(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise HipError("optimizer: %s must be a number, got %r" % (name, v))
    v = float(v)
    if not math.isfinite(v) or abs(v) > 3.4e38:
        raise HipError("optimizer: %s = %r is not finite" % (name, v))
    return float(np.float32(v))


def _count(name, v, lo):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) < 2 ** 31:
        raise HipError("optimizer: %s must be an integer in [%d, 2^31), got %r" % (name, lo, v))
    return int(v)


def _flag(name, v):
    if not isinstance(v, (bool, np.bool_)):
        raise HipError("optimizer: %s must be true or false, got %r" % (name, v))
    return bool(v)


class LRSchedule:
    """LRSchedule() | ("cosine", warmup=100, total=10000, min_factor=0.01) | ("linear", total=..., ...) | ("step", gamma=0.5,
    period=1000); warmup: linear ramp over the first `warmup` steps, with every kind.  cosine and linear need total > warmup."""

    def __init__(self, kind="constant", warmup=0, total=None, min_factor=0.0, gamma=1.0, period=1):
        if not isinstance(kind, str) or kind.lower() not in SCHEDULES:
            raise HipError("optimizer: unknown schedule %r (known: %s)" % (kind, ", ".join(SCHEDULES)))
        self.kind = kind.lower()
        self.warmup = _count("warmup", warmup, 0)
        self.total = None if total is None else _count("total", total, 0)
        if self.kind in ("cosine", "linear") and (self.total is None or self.total <= self.warmup):
            raise HipError("optimizer: a %s schedule needs total > warmup, got total %r, warmup %d" % (self.kind, self.total, self.warmup))
        self.min_factor = _number("min_factor", min_factor)
        if not 0.0 <= self.min_factor <= 1.0:
            raise HipError("optimizer: min_factor %r outside [0, 1]" % self.min_factor)
        self.gamma = _number("gamma", gamma)
        if not 0.0 < self.gamma <= 1.0:
            raise HipError("optimizer: gamma %r outside (0, 1]" % self.gamma)
        self.period = _count("period", period, 1)

    @property
    def is_default(self):
        return self.kind == "constant" and self.warmup == 0

    def __repr__(self):
        return "LRSchedule(%r, warmup=%d, total=%r, min_factor=%r, gamma=%r, period=%d)" % (
            self.kind, self.warmup, self.total, self.min_factor, self.gamma, self.period)

    def factor(self, step):
        """f(t) in float64 for the 1-based step t."""
        t = float(_count("step", step, 1))
        W = float(self.warmup)
        w = t / W if self.warmup > 0 and t <= W else 1.0
        if self.kind in ("cosine", "linear"):
            q = min(max((t - W) / (float(self.total) - W), 0.0), 1.0)
            if self.kind == "cosine":
                return w * (self.min_factor + (1.0 - self.min_factor) * (1.0 + math.cos(math.pi * q)) / 2.0)
            return w * (1.0 - (1.0 - self.min_factor) * q)
        if self.kind == "step":
            return w * self.gamma ** math.floor((t - 1.0) / float(self.period))
        return w

    def as_config(self):
        c = {"KIND": self.kind, "WARMUP": self.warmup}
        if self.kind in ("cosine", "linear"):
            c.update(TOTAL=self.total, MIN_FACTOR=self.min_factor)
        if self.kind == "step":
            c.update(GAMMA=self.gamma, PERIOD=self.period)
        return c


class Optimizer:
    """Optimizer() | ("adamw") | ("adam", amsgrad=True) | ("sgd", momentum=0.9, nesterov=True) | ("lamb", trust_clip=0.0,
    decay_bias=False) | ("lars", momentum=0.9, nesterov=False, trust_coef=1e-3, trust_clip=0.0, decay_bias=False), each with
    schedule=LRSchedule(...).  momentum and nesterov are read by sgd and lars only, amsgrad belongs to adam / adamw, trust_clip (an
    upper bound of the layer-wise ratio, 0 = none) and decay_bias (weight decay on the biases too) to lamb / lars, trust_coef to lars.
    The default - Adam with L2 decay, AMSGrad off, a constant rate - is `is_default`: the engine then runs exactly what it runs
    without an optimizer setting."""

    def __init__(self, kind="adam", amsgrad=False, momentum=0.0, nesterov=False, schedule=None, trust_clip=0.0, trust_coef=1e-3,
                 decay_bias=False):
        if not isinstance(kind, str) or kind.lower() not in KINDS:
            raise HipError("optimizer: unknown kind %r (known: %s)" % (kind, ", ".join(KINDS)))
        self.kind = kind.lower()
        self.amsgrad = _flag("amsgrad", amsgrad)
        self.momentum = _number("momentum", momentum)
        self.nesterov = _flag("nesterov", nesterov)
        if not 0.0 <= self.momentum < 1.0:
            raise HipError("optimizer: momentum %r outside [0, 1)" % self.momentum)
        if self.nesterov and not self.momentum > 0.0:
            raise HipError("optimizer: nesterov needs momentum > 0")
        if self.amsgrad and self.kind in ("sgd", "lamb", "lars"):
            raise HipError("optimizer: amsgrad belongs to adam / adamw, not to %s" % self.kind)
        self.trust_clip = self._trust_number("trust_clip", trust_clip)
        self.trust_coef = self._trust_number("trust_coef", trust_coef)
        self.decay_bias = _flag("decay_bias", decay_bias)
        if not self.trust_clip >= 0.0:
            raise HipError("optimizer: trust_clip %r is negative or not finite" % self.trust_clip)
        if self.kind == "lars" and not self.trust_coef > 0.0:
            raise HipError("optimizer: trust_coef %r is not a finite value > 0" % self.trust_coef)
        if schedule is not None and not isinstance(schedule, LRSchedule):
            raise HipError("optimizer: schedule must be an LRSchedule or None, got %r" % (schedule,))
        self.schedule = LRSchedule() if schedule is None else schedule

    @staticmethod
    def _trust_number(name, v):
        """fp32 value of a trust setting; a non-finite one is refused in the words the library uses."""
        if isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and not math.isfinite(float(v)):
            raise HipError("optimizer: %s %r is negative or not finite" % (name, v))
        return _number(name, v)

    @property
    def is_default(self):
        return self.kind == "adam" and not self.amsgrad and self.schedule.is_default

    @property
    def is_trust(self):
        """lamb / lars: the update scales each weight matrix's step by its layer-wise trust ratio."""
        return self.kind in ("lamb", "lars")

    def __repr__(self):
        if self.is_trust:
            return "Optimizer(%r, momentum=%r, nesterov=%r, trust_clip=%r, trust_coef=%r, decay_bias=%r, schedule=%r)" % (
                self.kind, self.momentum, self.nesterov, self.trust_clip, self.trust_coef, self.decay_bias, self.schedule)
        return "Optimizer(%r, amsgrad=%r, momentum=%r, nesterov=%r, schedule=%r)" % (
            self.kind, self.amsgrad, self.momentum, self.nesterov, self.schedule)

    def lr_at(self, lr, step):
        """lr_t of the 1-based step: float32(float32(lr) * f(step)), as a Python float."""
        return float(np.float32(float(np.float32(lr)) * self.schedule.factor(step)))

    def as_struct(self, vmax=None, trust_ws=None):
        """The codae_optimizer struct; vmax: the data pointer of AMSGrad's running maximum, trust_ws: that of the trust kinds' work
        space (ctypes.c_void_p or None)."""
        from ..hip import Optimizer as Struct
        s = self.schedule
        st = Struct(KINDS[self.kind], int(self.amsgrad), self.momentum, int(self.nesterov), SCHEDULES[s.kind], s.warmup,
                    0 if s.total is None else s.total, s.period, s.min_factor, s.gamma, vmax if self.amsgrad else None)
        if self.is_trust:
            st.trust_clip, st.trust_coef, st.decay_bias, st.trust_ws = self.trust_clip, self.trust_coef, int(self.decay_bias), trust_ws
        return st

    def as_config(self):
        """The `HIP: OPTIMIZER:` block optimizer_from_config reads back into an equal setting."""
        c = {"KIND": self.kind, "AMSGRAD": self.amsgrad, "MOMENTUM": self.momentum, "NESTEROV": self.nesterov,
             "SCHEDULE": self.schedule.as_config()}
        if self.is_trust:
            c.update(TRUST_CLIP=self.trust_clip, DECAY_BIAS=self.decay_bias)
            if self.kind == "lars":
                c.update(TRUST_COEF=self.trust_coef)
        return c

    # ---- host tensors and the drop-in loops --------------------------------------------------------
    def _trust_step(self, p, g, state, lr_t, wd, b1, b2, eps, c, t, matrix):
        """lamb / lars on one tensor: a matrix with its own ratio (left in state["ratio"], a Python float of the fp32 value), or
        a bias (matrix=False: ratio 1, decay only with decay_bias).  One torch op per fp32 operation of the definition."""
        import torch
        f = lambda x: float(np.float32(x))
        wd1 = wd if matrix or self.decay_bias else 0.0
        norm = lambda x: math.sqrt(float((x * x).double().sum()))
        m = state["m"]
        g1 = g * c
        if self.kind == "lamb":
            v = state["v"]
            bc1, bc2 = 1.0 - b1 ** float(t), 1.0 - b2 ** float(t)
            m.mul_(b1).add_(g1 * f(np.float32(1) - np.float32(b1)))
            v.mul_(b2).add_((g1 * f(np.float32(1) - np.float32(b2))) * g1)
            # (the root through double: the correctly rounded fp32 root the device takes - a vectorised fp32 sqrt may be an ulp off)
            u = (m / (v.double().sqrt().to(v.dtype) * f(1.0 / math.sqrt(bc2)) + eps)) * f(1.0 / bc1) + p * wd1
            other = u
        else:
            other = g1
        ratio = 1.0
        if matrix:
            P, D = norm(p), norm(other)
            if P > 0.0 and D > 0.0:
                ratio = P / D if self.kind == "lamb" else self.trust_coef * P / (D + wd * P + eps)
            if self.trust_clip > 0.0 and ratio > self.trust_clip:
                ratio = self.trust_clip
        ratio = f(ratio) if p.dtype == torch.float32 else ratio
        state["ratio"] = ratio
        if self.kind == "lamb":
            return p.sub_(u * (f(np.float32(lr_t) * np.float32(ratio)) if p.dtype == torch.float32 else lr_t * ratio))
        d = (g1 + p * wd1) * ratio
        m.mul_(self.momentum).add_(d)
        u = d + m * self.momentum if self.nesterov else m
        return p.sub_(u * lr_t)

    def step(self, p, g, state, hyper, coef=1.0, matrix=True):
        """One update of the tensor p in place from its (unclipped) gradient g, in plain torch ops and p's dtype.
        state: a dict the call keeps the tensor's moments in ("m", "v", "vmax": created as zeros when missing); hyper: anything
        with lr, weight_decay, beta1, beta2, eps and the 1-based step (a codae.hip.Hyper, DaeEngine.hyper()); coef: the clip
        coefficient of clip_grad_norm_ (1 = no clipping); matrix (lamb / lars only): the tensor is a weight matrix with a trust
        ratio of its own (left in state["ratio"]), False: a bias.  Returns p."""
        import torch
        t = int(hyper.step)
        lr_t = self.lr_at(hyper.lr, t)
        wd, b1, b2, eps = (float(np.float32(x)) for x in (hyper.weight_decay, hyper.beta1, hyper.beta2, hyper.eps))
        c = float(coef)
        with torch.no_grad():
            for key in ("m",) + (() if self.kind in ("sgd", "lars") else ("v",)) + (("vmax",) if self.amsgrad else ()):
                if state.get(key) is None:
                    state[key] = torch.zeros_like(p)
            if self.is_trust:
                return self._trust_step(p, g, state, lr_t, wd, b1, b2, eps, float(np.float32(c)), t, bool(matrix))
            m = state["m"]
            if self.kind == "sgd":
                g1 = g.mul(c).add_(p, alpha=wd)
                m.mul_(self.momentum).add_(g1)
                u = g1.add(m, alpha=self.momentum) if self.nesterov else m
                return p.sub_(u, alpha=lr_t)
            if self.kind == "adamw":
                g1 = g.mul(c)
                p.sub_(p, alpha=float(np.float32(lr_t) * np.float32(wd)) if p.dtype == torch.float32 else lr_t * wd)
            else:
                g1 = g.mul(c).add_(p, alpha=wd)
            v = state["v"]
            m.mul_(b1).add_(g1, alpha=1.0 - b1)
            v.mul_(b2).addcmul_(g1, g1, value=1.0 - b2)
            d = v
            if self.amsgrad:
                d = torch.maximum(state["vmax"], v, out=state["vmax"])
            bc1, bc2 = 1.0 - b1 ** float(t), 1.0 - b2 ** float(t)
            denom = d.sqrt().mul_(1.0 / math.sqrt(bc2)).add_(eps)
            return p.addcdiv_(m, denom, value=-(lr_t / bc1))


def optimizer_from_config(block, total_steps=None):
    """The `HIP: OPTIMIZER:` block of the embedding script's config: {KIND: adam | adamw | sgd | lamb | lars, AMSGRAD: false,
    MOMENTUM: 0.9, NESTEROV: true, TRUST_CLIP: 0.0, TRUST_COEF: 0.001, DECAY_BIAS: false, SCHEDULE: {KIND: constant | cosine | linear | step, WARMUP: 100, TOTAL: 10000, MIN_FACTOR: 0.01, GAMMA: 0.5,
    PERIOD: 1000}}.  None / empty -> None.  total_steps: what a SCHEDULE without TOTAL gets (the script's own loop count)."""
    if not block:
        return None
    if not isinstance(block, dict):
        raise HipError("OPTIMIZER must be a mapping, got %r" % (block,))
    known = {"KIND", "AMSGRAD", "MOMENTUM", "NESTEROV", "SCHEDULE", "TRUST_CLIP", "TRUST_COEF", "DECAY_BIAS"}
    extra = sorted(set(map(str, block)) - known)
    if extra:
        raise HipError("OPTIMIZER: unknown key(s) %s (known: %s)" % (", ".join(extra), ", ".join(sorted(known))))
    schedule = None
    sb = block.get("SCHEDULE")
    if sb:
        if not isinstance(sb, dict):
            raise HipError("OPTIMIZER: SCHEDULE must be a mapping, got %r" % (sb,))
        sknown = {"KIND", "WARMUP", "TOTAL", "MIN_FACTOR", "GAMMA", "PERIOD"}
        extra = sorted(set(map(str, sb)) - sknown)
        if extra:
            raise HipError("OPTIMIZER: SCHEDULE: unknown key(s) %s (known: %s)" % (", ".join(extra), ", ".join(sorted(sknown))))
        total = sb.get("TOTAL")
        schedule = LRSchedule(str(sb.get("KIND", "constant")), warmup=sb.get("WARMUP", 0), total=total_steps if total is None else total,
                              min_factor=sb.get("MIN_FACTOR", 0.0), gamma=sb.get("GAMMA", 1.0), period=sb.get("PERIOD", 1))
    return Optimizer(str(block.get("KIND", "adam")), amsgrad=block.get("AMSGRAD", False), momentum=block.get("MOMENTUM", 0.0),
                     nesterov=block.get("NESTEROV", False), schedule=schedule, trust_clip=block.get("TRUST_CLIP", 0.0),
                     trust_coef=block.get("TRUST_COEF", 1e-3), decay_bias=block.get("DECAY_BIAS", False))
