"""CPU-only tests of tests/optim_ref.py - the reference tests/test_gpu_optimizer_kinds.py holds every optimizer kind and the
learning-rate schedule to - and of codae.tool.optimizer, the host statement of the same definition.

1. The bounds: the fp32 emulation of the kernels' arithmetic (step32_emulated) stays inside bounds() on adam_ref's planted generator
   with room to spare - worst |error| / bound <= 0.75 - for every kind, with and without AMSGrad, on a first and a later step, with
   weight decay 0 and > 0, clipped and not.  The bounds are thus measured against the emulation, never against a GPU run.
2. The formula: step64 / factor against float64 torch.optim.AdamW, Adam(amsgrad=True), SGD(momentum, nesterov) under LambdaLR, five
   steps on three tensors, W = 2 and T = 4 so that the steps are t < W, t = W, W < t < T, t = T and t > T; float64 against float64
   (the unrounded lr_t on both sides), different operation order only: |difference| <= 1e-12 max |value| per tensor.
3. codae.tool.Optimizer.step (fp32 torch ops) and lr_at stay within the bounds of the restatement.
4. optimizer_from_config round-trips the documented block and refuses what the C setter refuses.
"""
import math

import numpy as np
import pytest
import torch

import optim_ref as OR

HYPERS = {"a": dict(lr=1e-3, wd=1e-2, betas=(0.9, 0.999), eps=1e-8),
          "b": dict(lr=3e-2, wd=0.0, betas=(0.8, 0.95), eps=1e-6)}
STEPS = (1, 1000)
SHAPES = [(136, 192), (72, 136), (4099,), (1,), (5,)]
COSINE = dict(sched="cosine", warmup=100, total=10000, min_factor=0.01)
OPTS = {
    "adam-cos": OR.opt("adam", **COSINE),
    "adam-ams": OR.opt("adam", amsgrad=True),
    "adamw": OR.opt("adamw"),
    "adamw-cos": OR.opt("adamw", **COSINE),
    "adamw-ams-cos": OR.opt("adamw", amsgrad=True, **COSINE),
    "sgd": OR.opt("sgd"),
    "sgd-mom": OR.opt("sgd", momentum=0.9, sched="step", gamma=0.5, period=300),
    "sgd-nesterov-cos": OR.opt("sgd", momentum=0.9, nesterov=True, **COSINE),
}


def _state(shape_seed, t, wd, o):
    out = []
    for i, s in enumerate(OR.planted_state(SHAPES, shape_seed, t == 1, wd)):
        s = dict(s)
        s["vmax"] = OR.planted_vmax(s["v"], 40 + i) if o.amsgrad else None
        if o.kind == "sgd":
            s["v"] = None
        out.append(s)
    return out


def test_the_emulated_fp32_updates_stay_inside_the_bounds():
    worst = {}
    for oname, o in sorted(OPTS.items()):
        for hname, hy in sorted(HYPERS.items()):
            for t in STEPS:
                h = OR.hyper(hy["lr"], hy["wd"], hy["betas"], hy["eps"], t)
                for coef in (1.0, 0.0123):
                    for s in _state(100 + t, t, hy["wd"], o):
                        args = (s["p"], s["g"], s["m"], s["v"], s["vmax"], h, o, np.float32(coef))
                        r = OR.worst_ratios(OR.step32_emulated(*args), OR.step64(*args), OR.bounds(*args))
                        for k, x in r.items():
                            worst[(oname, k)] = max(worst.get((oname, k), 0.0), x)
    for oname in sorted(OPTS):
        print("MEASURE emulation %-18s worst |error| / bound: %s" % (oname, "  ".join(
            "%s %.3f" % (k, worst[(oname, k)]) for k in OR.KEYS if (oname, k) in worst)))
    assert all(np.isfinite(x) and x <= 0.75 for x in worst.values()), {k: x for k, x in worst.items() if not x <= 0.75}
    assert ("sgd", "v") not in worst and ("adam-ams", "vmax") in worst


def test_amsgrad_maximum_keeps_a_nan_from_either_side():
    h = OR.hyper(1e-3, 0.0, t=3)
    o = OR.opt("adam", amsgrad=True)
    p, g, m = np.ones(3, np.float32), np.array([1.0, np.nan, 1.0], np.float32), np.zeros(3, np.float32)
    v, x = np.ones(3, np.float32), np.array([5.0, 5.0, np.nan], np.float32)
    for fn in (OR.step64, OR.step32_emulated):
        w = fn(p, g, m, v, x, h, o, 1.0)
        assert np.isfinite(w["vmax"][0]) and np.isnan(w["vmax"][1]) and np.isnan(w["vmax"][2]), fn
        assert np.isfinite(w["p"][0]) and np.isnan(w["p"][1]) and np.isnan(w["p"][2]), fn


def test_factor_at_the_corners():
    cos = OR.opt("adam", sched="cosine", warmup=4, total=12, min_factor=0.25)
    assert [OR.factor(cos, t) for t in (1, 2, 4)] == [0.25, 0.5, 1.0]                  # the ramp; q = 0 at t = W
    assert abs(OR.factor(cos, 8) - 0.625) <= 1e-15 and OR.factor(cos, 12) == OR.factor(cos, 500) == 0.25
    lin = OR.opt("adam", sched="linear", warmup=0, total=10, min_factor=0.5)
    assert OR.factor(lin, 5) == 0.75 and OR.factor(lin, 10) == OR.factor(lin, 11) == 0.5
    stp = OR.opt("adam", sched="step", gamma=0.5, period=3, warmup=2)
    assert [OR.factor(stp, t) for t in (1, 2, 3, 4, 7)] == [0.5, 1.0, 1.0, 0.5, 0.25]
    assert OR.factor(OR.opt("adam", warmup=3), 2) == 2.0 / 3.0 and OR.factor(OR.opt("adam"), 9) == 1.0
    h = OR.hyper(1e-3, 0.0, t=8)
    assert OR.lr_t(h, cos) == float(np.float32(h.lr * 0.625)) != OR.lr_t(h, cos, rounded=False)


# ---- 2. against torch ------------------------------------------------------------------------------------------------------
W_T, T_T = 2, 4


def _lambda(kind, epoch):
    """LambdaLR's multiplier for its epoch counter e = t - 1, written in e from the definition."""
    t = epoch + 1
    w = t / W_T if t <= W_T else 1.0
    q = min(max((t - W_T) / (T_T - W_T), 0.0), 1.0)
    if kind == "cosine":
        return w * (0.125 + 0.875 * (1.0 + math.cos(math.pi * q)) / 2.0)
    if kind == "linear":
        return w * (1.0 - 0.875 * q)
    return w * 0.5 ** (epoch // 2)


TORCH_CASES = {
    "adamw-cosine": ("adamw", False, "cosine"),
    "adamw-amsgrad-linear": ("adamw", True, "linear"),
    "adam-amsgrad-cosine": ("adam", True, "cosine"),
    "adam-step": ("adam", False, "step"),
    "sgd-momentum-cosine": ("sgd", False, "cosine"),
    "sgd-nesterov-step": ("sgd", True, "step"),          # (the flag is nesterov here)
    "sgd-plain-linear": ("sgd", None, "linear"),         # (None: momentum 0)
}


@pytest.mark.parametrize("case", sorted(TORCH_CASES))
def test_step64_is_the_torch_optimizer_under_lambda_lr(case):
    kind, flag, sched = TORCH_CASES[case]
    lr, wd, betas, eps = 1e-2, 1e-2, (0.8, 0.95), 1e-6
    h1 = OR.hyper(lr, wd, betas, eps, 1)
    rng = np.random.default_rng(17)
    shapes = [(7, 5), (33,), (4, 3, 2)]
    ps = [rng.standard_normal(s) for s in shapes]
    ref = [torch.nn.Parameter(torch.tensor(p.copy())) for p in ps]
    mu = 0.0 if flag is None else float(np.float32(0.9))
    if kind == "sgd":
        o = OR.opt("sgd", momentum=mu, nesterov=bool(flag), sched=sched, warmup=W_T, total=T_T, min_factor=0.125, gamma=0.5, period=2)
        topt = torch.optim.SGD(ref, lr=h1.lr, momentum=mu, nesterov=bool(flag), weight_decay=h1.wd)
    else:
        o = OR.opt(kind, amsgrad=flag, sched=sched, warmup=W_T, total=T_T, min_factor=0.125, gamma=0.5, period=2)
        cls = torch.optim.AdamW if kind == "adamw" else torch.optim.Adam
        topt = cls(ref, lr=h1.lr, betas=(h1.b1, h1.b2), eps=h1.eps, weight_decay=h1.wd, amsgrad=bool(flag))
    tsched = torch.optim.lr_scheduler.LambdaLR(topt, lambda e: _lambda(sched, e))
    st = [dict(p=p, m=np.zeros(p.shape), v=None if kind == "sgd" else np.zeros(p.shape), x=np.zeros(p.shape) if o.amsgrad else None)
          for p in ps]
    for t in range(1, 6):
        h = OR.hyper(lr, wd, betas, eps, t)
        assert abs(topt.param_groups[0]["lr"] - OR.lr_t(h, o, rounded=False)) <= 1e-15 * h.lr, (case, t)
        for r, s in zip(ref, st):
            g = rng.standard_normal(s["p"].shape)
            r.grad = torch.tensor(g)
            w = OR.step64(s["p"], g, s["m"], s["v"], s["x"], h, o, 1.0, rounded_lr=False)          # (float64 state carried on)
            s.update(p=w["p"], m=w["m"], v=w["v"], x=w["vmax"])
        topt.step()
        tsched.step()
        for r, s in zip(ref, st):
            want = r.detach().numpy()
            err = float(np.abs(s["p"] - want).max())
            assert err <= 1e-12 * float(np.abs(want).max()), (case, t, err)
            if o.amsgrad:
                tmax = topt.state[r]["max_exp_avg_sq"].numpy()
                assert float(np.abs(s["x"] - tmax).max()) <= 1e-12 * float(tmax.max()), (case, t)


# ---- 3. codae.tool.Optimizer -----------------------------------------------------------------------------------------------
class _H:
    def __init__(self, h):
        self.lr, self.weight_decay, self.beta1, self.beta2, self.eps, self.step = h.lr, h.wd, h.b1, h.b2, h.eps, h.t


def _tool(o):
    from codae.tool import LRSchedule, Optimizer
    return Optimizer(o.kind, amsgrad=o.amsgrad, momentum=o.mu, nesterov=o.nesterov,
                     schedule=LRSchedule(o.sched, warmup=o.warmup, total=o.total or None, min_factor=o.min_factor, gamma=o.gamma, period=o.period))


@pytest.mark.parametrize("oname", sorted(OPTS))
def test_tool_optimizer_step_and_lr_at_stay_inside_the_bounds(oname):
    o = OPTS[oname]
    tool = _tool(o)
    assert OR.opt_of(tool) == o
    worst = {}
    for hname, hy in sorted(HYPERS.items()):
        for t in STEPS:
            h = OR.hyper(hy["lr"], hy["wd"], hy["betas"], hy["eps"], t)
            want_lr = OR.lr_t(h, o)
            assert abs(tool.lr_at(hy["lr"], t) - want_lr) <= 2 * OR.U * want_lr, (oname, t)
            for coef in (1.0, 0.0123):
                for s in _state(300 + t, t, hy["wd"], o)[:3]:
                    args = (s["p"], s["g"], s["m"], s["v"], s["vmax"], h, o, np.float32(coef))
                    p = torch.tensor(s["p"].copy())
                    state = {k: torch.tensor(s[src].copy()) for k, src in (("m", "m"), ("v", "v"), ("vmax", "vmax")) if s[src] is not None}
                    out = tool.step(p, torch.tensor(s["g"]), state, _H(h), float(np.float32(coef)))
                    assert out is p and p.dtype == torch.float32
                    got = {"p": p.numpy(), "m": state["m"].numpy(), "v": state["v"].numpy() if "v" in state else None,
                           "vmax": state["vmax"].numpy() if "vmax" in state else None}
                    for k, x in OR.worst_ratios(got, OR.step64(*args), OR.bounds(*args)).items():
                        worst[k] = max(worst.get(k, 0.0), x)
    print("MEASURE Optimizer.step %-18s worst |error| / bound: %s" % (oname, "  ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    assert all(x <= 1.0 for x in worst.values()), worst


def test_tool_optimizer_step_creates_zero_state_and_propagates_nan():
    from codae.tool import Optimizer
    h = _H(OR.hyper(1e-3, 1e-2, t=1))
    for tool, keys in ((Optimizer("adamw", amsgrad=True), {"m", "v", "vmax"}), (Optimizer("sgd", momentum=0.5), {"m"})):
        p, g, state = torch.ones(4), torch.full((4,), 0.5), {}
        tool.step(p, g, state, h, float("nan"))
        assert set(state) == keys and all(torch.isnan(t).all() for t in state.values()) and torch.isnan(p).all()


# ---- 4. the config block ---------------------------------------------------------------------------------------------------
BLOCK = {"KIND": "adamw", "AMSGRAD": False, "MOMENTUM": 0.9, "NESTEROV": True,
         "SCHEDULE": {"KIND": "cosine", "WARMUP": 100, "TOTAL": 10000, "MIN_FACTOR": 0.01}}


def test_optimizer_from_config_round_trips_and_refuses():
    from codae.hip import HipError
    from codae.tool import Optimizer, optimizer_from_config
    o = optimizer_from_config(BLOCK)
    f32 = lambda x: float(np.float32(x))
    assert (o.kind, o.amsgrad, o.momentum, o.nesterov) == ("adamw", False, f32(0.9), True)
    s = o.schedule
    assert (s.kind, s.warmup, s.total, s.min_factor) == ("cosine", 100, 10000, f32(0.01)) and not o.is_default
    again = optimizer_from_config(o.as_config())
    assert again.as_config() == o.as_config() and OR.opt_of(again) == OR.opt_of(o)
    assert {k: (f32(v) if isinstance(v, float) else v) for k, v in BLOCK.items() if k != "SCHEDULE"} == \
        {k: v for k, v in o.as_config().items() if k != "SCHEDULE"}
    assert {k: (f32(v) if isinstance(v, float) else v) for k, v in BLOCK["SCHEDULE"].items()} == o.as_config()["SCHEDULE"]
    assert optimizer_from_config(None) is None and optimizer_from_config({}) is None
    assert optimizer_from_config({"KIND": "adam"}).is_default and Optimizer().is_default
    # TOTAL left out: the caller's loop count
    assert optimizer_from_config({"SCHEDULE": {"KIND": "linear", "WARMUP": 3}}, total_steps=40).schedule.total == 40
    sch = lambda **kw: {"SCHEDULE": dict({"KIND": "cosine", "TOTAL": 10}, **kw)}
    bad = [
        {"KIND": "adamw", "LR": 1e-3}, {"SCHEDULE": {"KIND": "cosine", "TOTAL": 10, "POWER": 2}},          # unknown keys
        {"KIND": "lion"}, sch(KIND="exponential"),                                                           # unknown kinds
        {"KIND": "sgd", "AMSGRAD": True}, {"KIND": "sgd", "NESTEROV": True}, {"KIND": "sgd", "MOMENTUM": 1.0},
        {"KIND": "sgd", "MOMENTUM": -0.1}, {"KIND": "sgd", "MOMENTUM": float("nan")}, {"KIND": "adam", "AMSGRAD": 1},
        sch(WARMUP=-1), sch(WARMUP=10), sch(TOTAL=None), sch(MIN_FACTOR=1.5), sch(MIN_FACTOR=-0.1),
        {"SCHEDULE": {"KIND": "step", "GAMMA": 0.0}}, {"SCHEDULE": {"KIND": "step", "GAMMA": 1.5}}, {"SCHEDULE": {"KIND": "step", "PERIOD": 0}},
        {"SCHEDULE": {"KIND": "linear"}}, "adamw",
    ]
    for block in bad:
        with pytest.raises(HipError):
            optimizer_from_config(block)
