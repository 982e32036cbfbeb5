"""Every optimizer kind and the on-device learning-rate schedule, on every update path, against the float64 restatement of
tests/optim_ref.py fed the same fp32 inputs, at rounding-level bounds (fixed by tests/test_optimizer_host.py against an fp32
emulation, never by a GPU run).  The layout follows tests/test_gpu_optimizer.py, whose helpers it shares: plant the state, run
the update, compare; or take a real step, read back the gradients it consumed, and compare with the reference applied to the state
cloned before the step.

  A. codae_optimizer_update, the flat kernel alone: n = 1, 5 (tail alone), 64 (float4 body alone), 1000, 4099 (body + tail);
     every kind x amsgrad under a cosine schedule at t = 1 and t = 1000.  vmax untouched where AMSGrad is off, v untouched bit
     for bit under SGD, 16 guard elements behind n untouched.
  B. codae_step_update on planted state: bf16 72 -> 136 -> 72 (the tiled kernel: 136 rows = two row tiles + 8, 72 and 136 columns
     both ragged against 128, a flat bias block) and fp32 48 -> 16 -> 48 (the flat kernel); p, m, v, vmax within bounds, both bf16
     shadows the rounding of the new p, all padding still zero.
  C. the same states through codae_step_update_span on two spans split at a multiple of 4 that is no multiple of a tile size.
  D. whole steps (AdamW + warm-up + cosine, SGD + Nesterov) on the chain path and on the per-layer path.
  E. graph replay: six steps bit-identical to six plain steps, ONE capture; a changed setting captures again.
  F. the default setting is a no-op, refused settings leave the previous one in force, non-finite values propagate.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import optim_ref as OR
from test_gpu_optimizer import bits, check_shadows, clip_values, live_mask, plant, shapes, _square, _widths

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"

HY = dict(lr=1e-3, wd=1e-2, betas=(0.9, 0.999), eps=1e-8)
COSINE = dict(warmup=100, total=10000, min_factor=0.01)


def tool_opt(name, **sched):
    """codae.tool.Optimizer by case name; sched: the cosine schedule's arguments (default COSINE)."""
    from codae.tool import LRSchedule, Optimizer
    s = LRSchedule("cosine", **(sched or COSINE))
    return {"adam": lambda: Optimizer("adam", schedule=s),
            "adam-ams": lambda: Optimizer("adam", amsgrad=True, schedule=s),
            "adamw": lambda: Optimizer("adamw", schedule=s),
            "adamw-ams": lambda: Optimizer("adamw", amsgrad=True, schedule=s),
            "sgd": lambda: Optimizer("sgd", momentum=0.9, nesterov=True, schedule=s)}[name]()


KINDS = ("adam", "adam-ams", "adamw", "adamw-ams", "sgd")


@pytest.fixture
def hip():
    from codae import hip as H
    H.lib()
    return H


def check_kind(before, got, hp, o, what, grad_sq, live=None, branch=None):
    """before / got: {"p", "g", "m", "v", "vmax"} / {"p", "m", "v", "vmax"} flat fp32 arrays (None where the kind keeps none); the
    coefficient comes from `grad_sq`, the scalar the update left (None: clipping off).  Returns the worst ratios."""
    h = OR.hyper_of_struct(hp)
    clip = float(hp.max_grad_norm)
    coef = np.float32(1.0)
    if clip > 0:
        want_sq = float((before["g"].astype(np.float64) ** 2).sum())
        assert abs(grad_sq - want_sq) <= 1e-6 * want_sq, "%s: grad-square scalar %.17g, float64 sum g^2 %.17g" % (what, grad_sq, want_sq)
        coef = OR.clip_coef32(grad_sq, clip)
    if branch is not None:
        assert (coef < 1) == (branch == "on"), "%s: clip %s but the coefficient is %r" % (what, branch, coef)
    live = np.ones(before["p"].size, dtype=bool) if live is None else live
    pick = lambda a: None if a is None else a[live]
    args = (pick(before["p"]), pick(before["g"]), pick(before["m"]), pick(before["v"]) if o.kind != "sgd" else None,
            pick(before["vmax"]) if o.amsgrad else None, h, o, coef)
    want, tol = OR.step64(*args), OR.bounds(*args)
    ratios = OR.worst_ratios({k: pick(got[k]) for k in OR.KEYS}, want, tol)
    print("MEASURE optimizer kinds %s: t %d lr_t %.6g coef %.6g  worst |error| / bound  %s" % (
        what, h.t, OR.lr_t(h, o), float(coef), "  ".join("%s %.3f" % kv for kv in ratios.items())))
    for k, r in ratios.items():
        if not r <= 1.0:
            a = pick(got[k]).astype(np.float64)
            e = np.abs(a - want[k])
            with np.errstate(divide="ignore", invalid="ignore"):
                i = int(np.argmax(np.where(e == 0, 0.0, e / tol[k])))
            raise AssertionError("%s: %s is %.3f bounds from the float64 update at live element %d: got %.9g want %.9g bound %.3g" % (
                what, k, r, i, a[i], want[k][i], tol[k][i]))
        assert (got[k][~live] == 0).all(), "%s: a pad element of %s moved" % (what, k)
    return ratios


# ---- A. the stand-alone entry ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", (1, 1000))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", (1, 5, 64, 1000, 4099))
def test_optimizer_update_entry_point_on_planted_state(hip, n, kind, t):
    tool = tool_opt(kind)
    o = OR.opt_of(tool)
    s = dict(OR.planted_state([(n,)], 700 + n, t == 1, HY["wd"])[0])
    s["vmax"] = OR.planted_vmax(s["v"], n)
    guard = np.float32(123.25)
    for branch in ("off", "on"):
        dev = {k: torch.full((n + 16,), float(guard), dtype=torch.float32, device=DEV) for k in ("p", "g", "m", "v", "vmax")}
        for k in dev:
            dev[k][:n].copy_(torch.from_numpy(s[k]))
        sc = torch.zeros(hip.S_COUNT, dtype=torch.float64, device=DEV)
        hp = hip.Hyper(HY["lr"], HY["wd"], HY["betas"][0], HY["betas"][1], HY["eps"], clip_values(s["g"])[branch], t, 0.0)
        st = tool.as_struct(hip.ptr(dev["vmax"]))
        hip.check(hip.lib().codae_optimizer_update(hip.ptr(dev["p"]), hip.ptr(dev["g"]), hip.ptr(dev["m"]), hip.ptr(dev["v"]),
                                                   hip.ptr(dev["vmax"]), n, C.byref(hp), C.byref(st), hip.ptr(sc), hip.current_stream()))
        torch.cuda.synchronize()
        scal = sc.cpu()
        gsq = float(scal[hip.S_GRAD_SQ]) + float(scal[hip.S_GRAD_SQ_SLOTS:hip.S_GRAD_SQ_SLOTS + hip.S_N_SLOTS].sum())
        out = {k: dev[k].cpu().numpy() for k in dev}
        what = "entry n %d %s clip %s" % (n, kind, branch)
        check_kind(s, {k: out[k][:n] for k in OR.KEYS}, hp, o, what, gsq, branch=branch)
        for k in out:
            assert (out[k][n:] == guard).all(), "%s: wrote behind n in %s" % (what, k)
        assert np.array_equal(bits(out["g"][:n]), bits(s["g"])), what
        if not o.amsgrad:
            assert np.array_equal(bits(out["vmax"][:n]), bits(s["vmax"])), "%s: vmax written without amsgrad" % what
        if o.kind == "sgd":
            assert np.array_equal(bits(out["v"][:n]), bits(s["v"])), "%s: v written under sgd" % what


# ---- B / C. the engine's update on planted state -----------------------------------------------------------------------------
STACKS = {"bf16": ("bf16", _widths([72, 136, 72])), "f32": ("f32", _widths([48, 16, 48]))}


@functools.lru_cache(maxsize=None)
def planted(stack, first_step):
    """Computed once per (stack, first step) and left unchanged."""
    return OR.planted_state(shapes(STACKS[stack][1]), 9100 + sorted(STACKS).index(stack), first_step, HY["wd"])


def engine_for(stack, tool):
    from codae.hip.engine import DaeEngine
    prec, sched = STACKS[stack]
    eng = DaeEngine(sched, 16, prec, DEV)
    eng.set_optimizer(tool)
    return eng


def plant_all(eng, state):
    """test_gpu_optimizer.plant, plus AMSGrad's maximum (planted_vmax of the planted v, inside the tensors only).  {"p", "g", ...}."""
    P, G, M, V = plant(eng, state)
    X = None
    if eng.adam_vmax is not None:
        live = live_mask(eng)
        X = np.zeros_like(V)
        X[live] = OR.planted_vmax(V[live], 77)
        eng.adam_vmax.copy_(torch.from_numpy(X))
        torch.cuda.synchronize()
    return {"p": P, "g": G, "m": M, "v": V, "vmax": X}


def read_state(eng):
    torch.cuda.synchronize()
    return {"p": eng.params.cpu().numpy(), "m": eng.adam_m.cpu().numpy(), "v": eng.adam_v.cpu().numpy(),
            "vmax": None if eng.adam_vmax is None else eng.adam_vmax.cpu().numpy()}


def check_engine(eng, before, hp, o, what, grad_sq=None, branch=None):
    got = read_state(eng)
    if float(hp.max_grad_norm) > 0 and grad_sq is None:
        grad_sq = eng.read_scalars()[2]
    r = check_kind(before, got, hp, o, what, grad_sq, live=live_mask(eng), branch=branch)
    if o.kind == "sgd":
        assert np.array_equal(bits(got["v"]), bits(before["v"])), "%s: v written under sgd" % what
    if eng.shadow is not None:
        check_shadows(eng, got["p"], what)
    return r


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("stack", sorted(STACKS))
def test_step_update_on_planted_state(stack, kind):
    tool = tool_opt(kind)
    o = OR.opt_of(tool)
    eng = engine_for(stack, tool)
    assert (eng.adam_vmax is not None) == o.amsgrad
    for t in (1, 1000):
        for branch in ("off", "on"):
            before = plant_all(eng, planted(stack, t == 1))
            hp = eng.hyper(HY["lr"], HY["wd"], clip=clip_values(before["g"])[branch], betas=HY["betas"], eps=HY["eps"], step=t)
            eng.step_update(hp)
            what = "planted %s %s t %d clip %s" % (stack, kind, t, branch)
            check_engine(eng, before, hp, o, what, branch=branch)
            assert np.array_equal(bits(eng.grads), bits(before["g"])), "%s: the update wrote into grads" % what


def two_spans(eng):
    """[0, a) and [a, n_param): a a multiple of 4 inside the first weight matrix, no multiple of 8, 64 or 128 (no tile size)."""
    a = eng.n_param // 3 // 4 * 4 + 4
    while a % 8 == 0:
        a += 4
    assert 0 < a < eng.n_param and a % 4 == 0 and a % 8 and eng.n_param % 4 == 0
    return [(0, a), (a, eng.n_param)]


def span_update(eng, hp):
    acc = eng.new_accumulator()
    for lo, hi in two_spans(eng):
        eng.span_sumsq(lo, hi, acc)
    eng.record_grad_sq(acc)
    for lo, hi in two_spans(eng):
        eng.step_update_span(hp, lo, hi, acc)
    eng.after_replica_sync()
    eng.step_count += 1
    torch.cuda.synchronize()
    return float(acc)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("stack", sorted(STACKS))
def test_step_update_span_on_planted_state(stack, kind):
    tool = tool_opt(kind)
    o = OR.opt_of(tool)
    eng = engine_for(stack, tool)
    t = 1000
    before = plant_all(eng, planted(stack, False))
    hp = eng.hyper(HY["lr"], HY["wd"], clip=clip_values(before["g"])["on"], betas=HY["betas"], eps=HY["eps"], step=t)
    gsq = span_update(eng, hp)
    check_engine(eng, before, hp, o, "spans %s %s" % (stack, kind), grad_sq=gsq, branch="on")
    if stack == "f32":
        # the flat kernel on both sides: with clipping off (no coefficient to agree on) two spans give the whole update's bits
        hp0 = eng.hyper(HY["lr"], HY["wd"], clip=0.0, betas=HY["betas"], eps=HY["eps"], step=t)
        plant_all(eng, planted(stack, False))
        span_update(eng, hp0)
        spans = read_state(eng)
        plant_all(eng, planted(stack, False))
        eng.step_update(hp0)
        whole = read_state(eng)
        for k in OR.KEYS:
            if whole[k] is not None:
                assert np.array_equal(bits(spans[k]), bits(whole[k])), "spans f32 %s: %s differs from the whole update" % (kind, k)


# ---- D / E. whole steps ------------------------------------------------------------------------------------------------------
# form -> (schedule, batch rows, the path codae_step_path must report)
WHOLE = {"chain": (_square(192, 4), 64, "chain"), "layers": (_widths([72, 136, 72]), 16, "layers")}
N_STEPS = 6


class Problem:
    pass


@functools.lru_cache(maxsize=None)
def problem(form):
    from oracle import dae_oracle as O
    p = Problem()
    p.sched, p.B, p.path = WHOLE[form]
    io = p.sched[0][0]
    assert io % 3 == 0 and p.sched[-1][1] == io
    rng = np.random.default_rng(8100 + io)
    p.params = O.init_params(p.sched, rng)
    p.n = 3 * p.B
    p.data = torch.tensor(8 * rng.random((p.n, io), dtype=np.float32), device=DEV)
    bm, _, _ = O.corrupter_tables([{"size": io // 3, "position": s * (io // 3)} for s in range(3)], 1)
    p.table = torch.tensor(bm).to(torch.uint8).to(DEV)
    p.draws = [(torch.tensor(rng.permutation(p.n)[:p.B], dtype=torch.int32, device=DEV),
                torch.tensor(rng.integers(0, 3, p.B), dtype=torch.int32, device=DEV)) for _ in range(N_STEPS)]
    return p


@pytest.fixture(scope="module", autouse=True)
def _release_device_memory():
    yield
    problem.cache_clear()
    torch.cuda.empty_cache()


def trainer_for(p, optimizer="none", use_graph=False):
    from codae.train import HipEmbeddingTrainer
    kw = {} if isinstance(optimizer, str) else {"optimizer": optimizer}
    tr = HipEmbeddingTrainer(p.sched, p.data, p.table, None, HY["lr"], HY["wd"], clip=1.0, max_batch=p.B, precision="bf16", device=DEV,
                             use_graph=use_graph, **kw)
    tr.engine.load_params(p.params)
    return tr


def all_bits(eng):
    torch.cuda.synchronize()
    ts = [eng.params, eng.adam_m, eng.adam_v, eng.shadow, eng.shadow_t] + ([] if eng.adam_vmax is None else [eng.adam_vmax])
    return [bits(t).copy() for t in ts]


@pytest.mark.parametrize("kind", ("adamw", "sgd"))
@pytest.mark.parametrize("form", sorted(WHOLE))
def test_whole_steps_update_as_the_float64_kind_of_their_own_gradients(form, kind):
    p = problem(form)
    tool = tool_opt(kind, warmup=2, total=4, min_factor=0.01)
    o = OR.opt_of(tool)
    tr = trainer_for(p, tool)
    eng = tr.engine
    assert eng.step_path(p.B) == p.path, (form, eng.step_path(p.B))
    clipped = 0
    for i, (rows, mid) in enumerate(p.draws[:4]):
        before = read_state(eng)
        t = eng.step_count + 1
        assert tr.current_lr() == tool.lr_at(HY["lr"], t) and abs(tr.current_lr() - OR.lr_t(OR.hyper(HY["lr"], 0, t=t), o)) <= 2 * OR.U * HY["lr"]
        hp = eng.hyper(HY["lr"], HY["wd"], clip=1.0, global_rows=p.B, step=t)
        assert tr.train_batch(rows, mask_id=mid) == p.B
        torch.cuda.synchronize()
        assert eng.step_count == t
        before["g"] = eng.grads.cpu().numpy().copy()
        assert np.isfinite(before["g"]).all() and (before["g"] != 0).mean() > 0.25
        check_engine(eng, before, hp, o, "whole %s %s step %d" % (form, kind, i))
        clipped += int(OR.clip_coef32(eng.read_scalars()[2], 1.0) < 1)
    assert clipped >= 1, "%s %s: no step was clipped" % (form, kind)


def test_graph_replay_is_plain_steps_bit_for_bit_and_a_schedule_never_recaptures():
    from codae.tool import LRSchedule, Optimizer
    p = problem("chain")
    tool = Optimizer("adamw", schedule=LRSchedule("cosine", warmup=3, total=6, min_factor=0.05))
    plain, graph = trainer_for(p, tool), trainer_for(p, tool, use_graph=True)
    assert graph.engine.step_path(p.B) == "chain" and graph.engine.graph_captures() == 0
    lrs = []
    for rows, mid in p.draws:
        lrs.append(graph.current_lr())
        assert plain.train_batch(rows, mask_id=mid) == graph.train_batch(rows, mask_id=mid) == p.B
    assert len(set(lrs)) == N_STEPS, lrs                                  # (six different rates, one graph)
    for name, a, b in zip(("params", "adam_m", "adam_v", "shadow", "shadow_t"), all_bits(plain.engine), all_bits(graph.engine)):
        assert np.array_equal(a, b), "graph replay: %s differs from six plain steps at %d elements" % (name, int((a != b).sum()))
    assert graph.engine.graph_captures() == 1
    graph.set_optimizer(Optimizer("adamw", schedule=LRSchedule("cosine", warmup=3, total=60, min_factor=0.05)))
    graph.train_batch(p.draws[0][0], mask_id=p.draws[0][1])
    torch.cuda.synchronize()
    assert graph.engine.graph_captures() == 2


# ---- F. default, refusals, non-finite ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(WHOLE))
def test_the_default_optimizer_is_a_no_op(form):
    from codae.tool import Optimizer
    p = problem(form)
    a, b = trainer_for(p), trainer_for(p, Optimizer())
    assert b.engine.optimizer.is_default and b.engine.adam_vmax is None and b.current_lr() == a.current_lr() == float(np.float32(HY["lr"]))
    for rows, mid in p.draws[:3]:
        a.train_batch(rows, mask_id=mid)
        b.train_batch(rows, mask_id=mid)
    for name, x, y in zip(("params", "adam_m", "adam_v", "shadow", "shadow_t"), all_bits(a.engine), all_bits(b.engine)):
        assert np.array_equal(x, y), "%s: %s differs under Optimizer()" % (form, name)


def test_a_refused_setting_leaves_the_previous_one_in_force(hip):
    tool = tool_opt("adamw-ams")
    a, b = engine_for("f32", tool), engine_for("f32", tool)
    vmax = hip.ptr(a.adam_vmax)
    off = C.c_void_p(a.adam_vmax.data_ptr() + 4)
    S = hip.Optimizer
    #           kind ams  mu  nest sched W   T  per  mf   gamma vmax
    refused = {
        "unknown kind": S(7, 0, 0.0, 0, 0, 0, 0, 1, 0.0, 1.0, None),
        "unknown schedule": S(0, 0, 0.0, 0, 9, 0, 0, 1, 0.0, 1.0, None),
        "momentum 1": S(2, 0, 1.0, 0, 0, 0, 0, 1, 0.0, 1.0, None),
        "momentum < 0": S(2, 0, -0.5, 0, 0, 0, 0, 1, 0.0, 1.0, None),
        "amsgrad with sgd": S(2, 1, 0.5, 0, 0, 0, 0, 1, 0.0, 1.0, vmax),
        "nesterov without momentum": S(2, 0, 0.0, 1, 0, 0, 0, 1, 0.0, 1.0, None),
        "amsgrad without vmax": S(1, 1, 0.0, 0, 0, 0, 0, 1, 0.0, 1.0, None),
        "amsgrad with a misaligned vmax": S(1, 1, 0.0, 0, 0, 0, 0, 1, 0.0, 1.0, off),
        "warmup < 0": S(1, 0, 0.0, 0, 1, -1, 10, 1, 0.0, 1.0, None),
        "total <= warmup": S(1, 0, 0.0, 0, 1, 10, 10, 1, 0.0, 1.0, None),
        "linear without total": S(1, 0, 0.0, 0, 2, 0, 0, 1, 0.0, 1.0, None),
        "min_factor > 1": S(1, 0, 0.0, 0, 1, 0, 10, 1, 1.5, 1.0, None),
        "min_factor NaN": S(1, 0, 0.0, 0, 1, 0, 10, 1, float("nan"), 1.0, None),
        "gamma 0": S(1, 0, 0.0, 0, 3, 0, 0, 1, 0.0, 0.0, None),
        "gamma > 1": S(1, 0, 0.0, 0, 3, 0, 0, 1, 0.0, 1.5, None),
        "period 0": S(1, 0, 0.0, 0, 3, 0, 0, 0, 0.0, 0.5, None),
    }
    for name, st in refused.items():
        with pytest.raises(hip.HipError):
            a._set_optimizer_struct(st)
    hp = a.hyper(HY["lr"], HY["wd"], clip=0.5, betas=HY["betas"], eps=HY["eps"], step=500)
    for eng in (a, b):
        plant_all(eng, planted("f32", False))
        eng.step_update(hp)
    for name, x, y in zip(("params", "adam_m", "adam_v", "vmax"), *[[bits(t) for t in (e.params, e.adam_m, e.adam_v, e.adam_vmax)] for e in (a, b)]):
        assert np.array_equal(x, y), "after the refusals %s differs from an engine that saw none" % name
    plain = engine_for("f32", None)
    plant(plain, planted("f32", False))
    plain.step_update(hp)
    assert not np.array_equal(bits(plain.params), bits(a.params))          # (and that setting is not the default's)


def _entry(hip, tool, s, clip, t=5):
    n = s["p"].size
    dev = {k: torch.from_numpy(s[k].copy()).to(DEV) for k in ("p", "g", "m", "v", "vmax")}
    sc = torch.zeros(hip.S_COUNT, dtype=torch.float64, device=DEV)
    hp = hip.Hyper(HY["lr"], HY["wd"], HY["betas"][0], HY["betas"][1], HY["eps"], clip, t, 0.0)
    st = tool.as_struct(hip.ptr(dev["vmax"]))
    hip.check(hip.lib().codae_optimizer_update(hip.ptr(dev["p"]), hip.ptr(dev["g"]), hip.ptr(dev["m"]), hip.ptr(dev["v"]),
                                               hip.ptr(dev["vmax"]), n, C.byref(hp), C.byref(st), hip.ptr(sc), hip.current_stream()))
    torch.cuda.synchronize()
    return {k: dev[k].cpu().numpy() for k in dev}


def test_non_finite_values_propagate_as_in_torch(hip):
    n = 1003
    s = dict(OR.planted_state([(n,)], 31, False, HY["wd"])[0])
    s["vmax"] = OR.planted_vmax(s["v"], 5)
    nan_g = dict(s, g=s["g"].copy())
    nan_g["g"][417] = np.nan
    # a NaN gradient under clipping: a NaN norm, a NaN coefficient - everything the kind writes is NaN
    out = _entry(hip, tool_opt("adamw-ams"), nan_g, 1.0)
    for k in ("p", "m", "v", "vmax"):
        assert np.isnan(out[k]).all(), "adamw + amsgrad: %s is not all NaN after a NaN gradient" % k
    out = _entry(hip, tool_opt("sgd"), nan_g, 1.0)
    assert np.isnan(out["p"]).all() and np.isnan(out["m"]).all() and np.array_equal(bits(out["v"]), bits(s["v"]))
    # without clipping the NaN stays where it is; a NaN v' makes vmax' NaN although vmax was finite (torch.maximum, not fmaxf)
    out = _entry(hip, tool_opt("adam-ams"), nan_g, 0.0)
    for k in ("p", "m", "v", "vmax"):
        assert np.isnan(out[k][417]) and np.isfinite(np.delete(out[k], 417)).all(), k
    nan_v = dict(s, v=s["v"].copy(), vmax=s["vmax"].copy())
    nan_v["v"][12] = np.nan
    nan_v["vmax"][500] = np.nan
    out = _entry(hip, tool_opt("adam-ams"), nan_v, 0.0)
    assert np.isnan(out["vmax"][[12, 500]]).all() and np.isnan(out["p"][[12, 500]]).all()
    assert np.isfinite(np.delete(out["vmax"], [12, 500])).all() and np.isfinite(out["m"]).all()
