"""The layer-wise trust-ratio kinds (LAMB, LARS) on the GPU, against the float64 restatement of tests/trust_ref.py fed the same
fp32 inputs, at the bounds tests/test_trust_host.py fixes against an fp32 emulation (never against a GPU run).  The layout and the
helpers are those of tests/test_gpu_optimizer_kinds.py: plant the state, run the update, compare; or take a real step, read back the
gradients it consumed, and compare with the restatement applied to the state cloned before the step.

  A. codae_trust_update, [0, n) as one matrix: n = 1, 5, 64, 1000, 4099 (one block's tail alone, a float4 body alone, two blocks
     with a tail), t = 1 and 1000, clip off and on; lamb, lamb clipped below its ratio, lars, lars with Nesterov.
  B. codae_step_update on planted state: bf16 72 -> 136 -> 72 (the tiled passes) and fp32 48 -> 16 -> 48 (the flat ones): per-matrix
     ratios, the bias block with ratio 1 and no decay, shadows, grads untouched, v untouched under lars.
  C. edge ratios: zero matrix, zero step, NaN gradient with and without clipping.
  D. whole steps on the chain and the per-layer path, twice for the same bits; graph replay; tied weights, weight average,
     save / load; the refused sharded update.
"""
import ctypes as C

import numpy as np
import pytest

import adam_ref as AR
import average_ref as AVR
import trust_ref as TR
from test_gpu_optimizer import bits, check_shadows, clip_values, live_mask, plant
from test_gpu_optimizer_kinds import HY, STACKS, all_bits, planted, problem, read_state

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"

COSINE = dict(warmup=100, total=10000, min_factor=0.01)
# sum g^2 on the device against the float64 sum of the same fp32 gradients, relative: at these sizes a lane squares and adds one
# float4 (a rounding per square, three additions), a wave adds in six butterfly steps, a block its four waves, the slots are doubles:
# 13 fp32 roundings on terms of one sign, 16 u with room (9.5e-7)
SUMSQ_TOL = 16.0 * TR.U
CASES = {"lamb": ("lamb", {}), "lamb-decay-bias": ("lamb", dict(decay_bias=True)), "lars": ("lars", dict(momentum=0.9)),
         "lars-nesterov": ("lars", dict(momentum=0.9, nesterov=True, trust_coef=0.02))}


def tool_of(case, trust_clip=0.0, **sched):
    from codae.tool import LRSchedule, Optimizer
    kind, kw = CASES[case]
    return Optimizer(kind, schedule=LRSchedule("cosine", **(sched or COSINE)), trust_clip=trust_clip, **kw)


@pytest.fixture
def hip():
    from codae import hip as H
    H.lib()
    return H


def coef_of(g, hp, grad_sq, what, branch=None):
    clip = float(hp.max_grad_norm)
    coef = np.float32(1.0)
    if clip > 0:
        want_sq = float((g.astype(np.float64) ** 2).sum())
        assert abs(grad_sq - want_sq) <= SUMSQ_TOL * want_sq, "%s: grad-square scalar %.17g, float64 sum g^2 %.17g" % (what, grad_sq, want_sq)
        coef = AR.clip_coef32(grad_sq, clip)
    if branch is not None:
        assert (coef < 1) == (branch == "on"), "%s: clip %s but the coefficient is %r" % (what, branch, coef)
    return coef


def check_tensor(before, got, ratio, h, tr, coef, matrix, what):
    """One tensor: before / got flat fp32 arrays by key, ratio: what the device left (None for a bias).  Returns the worst ratios."""
    args = (before["p"], before["g"], before["m"], before["v"], h, tr, coef, matrix)
    want, tol = TR.step64(*args), TR.bounds(*args)
    r = TR.worst_ratios(dict(got, ratio=want["ratio"] if ratio is None else float(ratio)), want, tol)
    for k, x in r.items():
        if not x <= 1.0:
            if k == "ratio":
                raise AssertionError("%s: ratio %.9g, float64 %.9g, bound %.3g" % (what, float(ratio), want["ratio"], tol["ratio"]))
            e = np.abs(got[k].astype(np.float64) - want[k])
            with np.errstate(divide="ignore", invalid="ignore"):
                i = int(np.argmax(np.where(e == 0, 0.0, e / tol[k])))
            raise AssertionError("%s: %s is %.3f bounds from the float64 update at element %d: got %.9g want %.9g bound %.3g" % (
                what, k, x, i, got[k][i], want[k][i], tol[k][i]))
    if tr.kind == "lars":
        assert np.array_equal(bits(got["v"]), bits(before["v"])), "%s: v written under lars" % what
    return r


# ---- A. the stand-alone entry --------------------------------------------------------------------------------------------------
def run_entry(hip, tool, s, clip, t, guard=None, wd=HY["wd"]):
    n = s["p"].size
    pad = 0 if guard is None else 16
    dev = {k: torch.full((n + pad,), 0.0 if guard is None else float(guard), dtype=torch.float32, device=DEV) for k in "pgmv"}
    for k in dev:
        dev[k][:n].copy_(torch.from_numpy(s[k].reshape(-1)))
    sc = torch.zeros(hip.S_COUNT, dtype=torch.float64, device=DEV)
    nbytes = int(hip.lib().codae_trust_ws_bytes_flat(n))
    assert nbytes == 4 * hip.TRUST_MAX_MATRICES + 16 * ((n + hip.TRUST_CHUNK - 1) // hip.TRUST_CHUNK)
    ws = torch.zeros(nbytes // 4 + 16, dtype=torch.float32, device=DEV)
    ws[nbytes // 4:] = 7.5
    hp = hip.Hyper(HY["lr"], wd, HY["betas"][0], HY["betas"][1], HY["eps"], clip, t, 0.0)
    st = tool.as_struct(None, None)
    hip.check(hip.lib().codae_trust_update(hip.ptr(dev["p"]), hip.ptr(dev["g"]), hip.ptr(dev["m"]), hip.ptr(dev["v"]), n, C.byref(hp),
                                           C.byref(st), hip.ptr(sc), hip.ptr(ws), nbytes, hip.current_stream()))
    torch.cuda.synchronize()
    scal = sc.cpu()
    gsq = float(scal[hip.S_GRAD_SQ]) + float(scal[hip.S_GRAD_SQ_SLOTS:hip.S_GRAD_SQ_SLOTS + hip.S_N_SLOTS].sum())
    w = ws.cpu().numpy()
    assert (w[nbytes // 4:] == 7.5).all() and (w[1:hip.TRUST_MAX_MATRICES] == 0).all(), "wrote outside the work space it asked for"
    return {k: dev[k].cpu().numpy() for k in dev}, float(w[0]), gsq, hp


@pytest.mark.parametrize("t", (1, 1000))
@pytest.mark.parametrize("case", ("lamb", "lamb-clipped", "lars", "lars-nesterov"))
@pytest.mark.parametrize("n", (1, 5, 64, 1000, 4099))
def test_trust_update_entry_point_on_planted_state(hip, n, case, t):
    s = AR.planted_state([(n,)], 700 + n, t == 1, HY["wd"])[0]
    guard = np.float32(123.25)
    for branch in ("off", "on"):
        clip = clip_values(s["g"])[branch]
        h = AR.hyper(HY["lr"], HY["wd"], HY["betas"], HY["eps"], t)
        base = case.replace("-clipped", "")
        tool = tool_of(base)
        if case.endswith("clipped"):
            # half the ratio the planted state has under this very coefficient
            coef0 = AR.clip_coef32(float((s["g"].astype(np.float64) ** 2).sum()), clip)
            own = TR.step64(s["p"], s["g"], s["m"], s["v"], h, TR.trust_of(tool), coef0)["ratio"]
            tool = tool_of(base, trust_clip=0.5 * own)
        tr = TR.trust_of(tool)
        out, ratio, gsq, hp = run_entry(hip, tool, s, clip, t, guard)
        what = "entry n %d %s t %d clip %s" % (n, case, t, branch)
        coef = coef_of(s["g"], hp, gsq, what, branch)
        r = check_tensor(s, {k: out[k][:n] for k in "pmv"}, ratio, h, tr, coef, True, what)
        print("MEASURE trust %s: ratio %.6g  worst |error| / bound  %s" % (what, ratio, "  ".join("%s %.3f" % kv for kv in r.items())))
        if tr.trust_clip > 0:
            assert np.float32(ratio) == np.float32(tr.trust_clip), (what, ratio, tr.trust_clip)
        for k in out:
            assert (out[k][n:] == guard).all(), "%s: wrote behind n in %s" % (what, k)
        assert np.array_equal(bits(out["g"][:n]), bits(s["g"])), what


# ---- C. edge ratios ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ("lamb", "lars"))
def test_edge_ratios(hip, case):
    n = 4099
    tool = tool_of(case)
    tr = TR.trust_of(tool)
    s = AR.planted_state([(n,)], 31, False, HY["wd"])[0]
    zero = {k: np.zeros(n, dtype=np.float32) for k in "pgmv"}
    out, ratio, _, _ = run_entry(hip, tool, zero, 0.0, 5)
    assert ratio == 1.0 and all((out[k] == 0).all() for k in "pmv"), "an all-zero matrix: ratio %r" % ratio
    # g = 0, m = 0, wd = 0: no step at all - ratio 1 and p bit for bit
    still = dict(s, g=zero["g"], m=zero["m"])
    out, ratio, _, _ = run_entry(hip, tool, still, 0.0, 5, wd=0.0)
    assert ratio == 1.0 and np.array_equal(bits(out["p"]), bits(s["p"])), "a zero step: ratio %r" % ratio
    # a NaN gradient element under clipping: a NaN norm, a NaN coefficient - everything the kind writes is NaN
    nan_g = dict(s, g=s["g"].copy())
    nan_g["g"][417] = np.nan
    out, ratio, _, _ = run_entry(hip, tool, nan_g, 1.0, 5)
    assert ratio == 1.0 and np.isnan(out["p"]).all() and np.isnan(out["m"]).all()
    assert np.isnan(out["v"]).all() if case == "lamb" else np.array_equal(bits(out["v"]), bits(s["v"]))
    # without clipping the NaN stays where it is: the norm it enters is NaN, so the ratio is 1, every other element as the
    # restatement with that ratio has it
    out, ratio, _, hp = run_entry(hip, tool, nan_g, 0.0, 5)
    h = AR.hyper(HY["lr"], HY["wd"], HY["betas"], HY["eps"], 5)
    want = TR.step32_emulated(nan_g["p"], nan_g["g"], nan_g["m"], nan_g["v"], h, tr, 1.0)
    assert ratio == 1.0 == want["ratio"]
    keep = np.arange(n) != 417
    for k in ("p", "m") + (("v",) if case == "lamb" else ()):
        assert np.isnan(out[k][417]) and np.isfinite(out[k][keep]).all(), k
        assert np.array_equal(np.isnan(out[k]), np.isnan(want[k])), k
    # (ratio exactly 1 and the matrix's decay: what the restatement calls a bias with decay_bias)
    fin = {k: nan_g[k][keep] for k in "pgmv"}
    check_tensor(fin, {k: out[k][keep] for k in "pmv"}, None, h, tr._replace(decay_bias=True), np.float32(1.0), False,
                 "NaN gradient, clip off, %s" % case)


# ---- B. the engine's update on planted state -------------------------------------------------------------------------------------
def tensors_of(eng, n_mats=None):
    """(name, lo, hi, is_matrix, ratio index) of every live tensor the update owns."""
    out = []
    for l, (k, n, _) in enumerate(eng.schedule):
        if n_mats is None or l < n_mats:
            out.append(("W%d" % l, eng.w_off[l], eng.w_off[l] + n * k, True, l))
    for l, (k, n, _) in enumerate(eng.schedule):
        out.append(("b%d" % l, eng.b_off[l], eng.b_off[l] + n, False, None))
    return out


def check_engine(eng, before, hp, tr, what, grad_sq=None, branch=None, n_mats=None):
    got = read_state(eng)
    ratios = eng.trust_ratios().cpu().numpy()
    assert ratios.dtype == np.float32 and ratios.shape == (eng.L if n_mats is None else n_mats,), ratios.shape
    if float(hp.max_grad_norm) > 0 and grad_sq is None:
        grad_sq = eng.read_scalars()[2]
    coef = coef_of(before["g"], hp, grad_sq, what, branch)
    h = AR.hyper_of_struct(hp)
    worst = {}
    for name, lo, hi, is_mat, ri in tensors_of(eng, n_mats):
        b = {k: before[k][lo:hi] for k in "pgmv"}
        g = {k: got[k][lo:hi] for k in "pmv"}
        r = check_tensor(b, g, ratios[ri] if is_mat else None, h, tr, coef, is_mat, "%s %s" % (what, name))
        for k, x in r.items():
            worst[k] = max(worst.get(k, 0.0), x)
    print("MEASURE trust %s: t %d coef %.6g ratios %s  worst |error| / bound  %s" % (
        what, h.t, float(coef), np.array2string(ratios, precision=5), "  ".join("%s %.3f" % kv for kv in worst.items())))
    live = live_mask(eng)
    for k in "pmv":
        assert (got[k][~live] == 0).all(), "%s: a pad element of %s moved" % (what, k)
    if eng.shadow is not None:
        check_shadows(eng, got["p"], what)
    return ratios


def plant_trust(eng, state):
    P, G, M, V = plant(eng, state)
    return {"p": P, "g": G, "m": M, "v": V}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("stack", sorted(STACKS))
def test_step_update_on_planted_state(stack, case):
    from codae.hip.engine import DaeEngine
    tool = tool_of(case)
    tr = TR.trust_of(tool)
    prec, sched = STACKS[stack]
    eng = DaeEngine(sched, 16, prec, DEV)
    eng.set_optimizer(tool)
    assert (eng.trust_ratios().cpu().numpy() == 0).all()                       # (zero before the first update)
    for t in (1, 1000):
        for branch in ("off", "on"):
            before = plant_trust(eng, planted(stack, t == 1))
            hp = eng.hyper(HY["lr"], HY["wd"], clip=clip_values(before["g"])[branch], betas=HY["betas"], eps=HY["eps"], step=t)
            eng.step_update(hp)
            what = "planted %s %s t %d clip %s" % (stack, case, t, branch)
            ratios = check_engine(eng, before, hp, tr, what, branch=branch)
            assert len(set(ratios.tolist())) == len(ratios), "%s: the matrices share a ratio: %s" % (what, ratios)
            assert np.array_equal(bits(eng.grads), bits(before["g"])), "%s: the update wrote into grads" % what
    if not tr.decay_bias:
        # the bias block: no decay by default - with wd 100 times larger its parameters move exactly as with wd 0 (clip off)
        outs = []
        for wd in (0.0, 100.0 * HY["wd"]):
            before = plant_trust(eng, planted(stack, False))
            eng.step_update(eng.hyper(HY["lr"], wd, clip=0.0, betas=HY["betas"], eps=HY["eps"], step=7))
            torch.cuda.synchronize()
            outs.append(eng.params[eng.b_off[0]:].cpu().numpy().copy())
        assert np.array_equal(bits(outs[0]), bits(outs[1])), "%s %s: weight decay reached the bias block" % (stack, case)


@pytest.mark.parametrize("case", ("lamb", "lars"))
@pytest.mark.parametrize("stack", sorted(STACKS))
def test_the_sharded_update_is_refused_and_touches_nothing(hip, stack, case):
    from codae.hip.engine import DaeEngine
    prec, sched = STACKS[stack]
    eng = DaeEngine(sched, 16, prec, DEV)
    eng.set_optimizer(tool_of(case))
    plant_trust(eng, planted(stack, False))
    was = all_state_bits(eng)
    hp = eng.hyper(HY["lr"], HY["wd"], clip=0.0, betas=HY["betas"], eps=HY["eps"], step=3)
    rc = hip.lib().codae_step_update_span(eng._h, C.byref(eng.bufs), C.byref(hp), 0, eng.n_param, None, hip.current_stream())
    assert rc == -3, rc                                                         # CODAE_E_UNSUPPORTED
    with pytest.raises(hip.HipError, match="norm spans shards"):
        hip.check(rc)
    for a, b in zip(was, all_state_bits(eng)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("case", ("lamb", "lars"))
def test_the_trainer_refuses_the_sharded_update_when_built_and_when_set(hip, case):
    from codae.tool import Optimizer
    p = problem("layers")
    with pytest.raises(hip.HipError, match="the sharded update is not supported: a matrix's norm spans shards"):
        trainer_for(p, tool_of(case), distributed=True, sharded_update=True)
    tr = trainer_for(p, Optimizer("adamw"), distributed=True, sharded_update=True)
    with pytest.raises(hip.HipError, match="norm spans shards"):
        tr.set_optimizer(tool_of(case))
    assert tr.engine.optimizer.kind == "adamw"                                  # (the previous setting stays)
    assert trainer_for(p, tool_of(case), distributed=True).dp.sharded is False


def all_state_bits(eng):
    torch.cuda.synchronize()
    ts = [eng.params, eng.grads, eng.adam_m, eng.adam_v] + ([] if eng.shadow is None else [eng.shadow, eng.shadow_t])
    return [bits(t).copy() for t in ts]


# ---- D. whole steps --------------------------------------------------------------------------------------------------------------
def trainer_for(p, tool, use_graph=False, **kw):
    from codae.train import HipEmbeddingTrainer
    tr = HipEmbeddingTrainer(p.sched, p.data, p.table, None, HY["lr"], HY["wd"], clip=1.0, max_batch=p.B, precision="bf16", device=DEV,
                             use_graph=use_graph, optimizer=tool, **kw)
    tr.engine.load_params(p.params)
    return tr


@pytest.mark.parametrize("case", ("lamb", "lars-nesterov"))
@pytest.mark.parametrize("form", ("chain", "layers"))
def test_whole_steps_update_as_the_float64_kind_of_their_own_gradients(form, case):
    p = problem(form)
    tool = tool_of(case, warmup=2, total=6, min_factor=0.01)
    ref = TR.trust_of(tool)
    tr, twin = trainer_for(p, tool), trainer_for(p, tool)
    eng = tr.engine
    assert eng.step_path(p.B) == p.path, (form, eng.step_path(p.B))
    for i, (rows, mid) in enumerate(p.draws):
        before = read_state(eng)
        t = eng.step_count + 1
        hp = eng.hyper(HY["lr"], HY["wd"], clip=1.0, global_rows=p.B, step=t)
        assert tr.train_batch(rows, mask_id=mid) == p.B and twin.train_batch(rows, mask_id=mid) == p.B
        torch.cuda.synchronize()
        before["g"] = eng.grads.cpu().numpy().copy()
        assert np.isfinite(before["g"]).all() and (before["g"] != 0).mean() > 0.25
        ratios = check_engine(eng, before, hp, ref, "whole %s %s step %d" % (form, case, i))
        assert np.array_equal(ratios, tr.trust_ratios().cpu().numpy()) and np.isfinite(ratios).all() and (ratios > 0).all()
    a, b = tr.state_digest(), twin.state_digest()
    assert a == b, "two runs of the same six steps differ: %s" % sorted(k for k in a if a[k] != b[k])
    assert np.array_equal(bits(tr.trust_ratios()), bits(twin.trust_ratios()))


@pytest.mark.parametrize("case", ("lamb", "lars"))
def test_graph_replay_is_plain_steps_bit_for_bit_with_one_capture(case):
    p = problem("chain")
    tool = tool_of(case, warmup=3, total=6, min_factor=0.05)
    plain, graph = trainer_for(p, tool), trainer_for(p, tool, use_graph=True)
    assert graph.engine.step_path(p.B) == "chain" and graph.engine.graph_captures() == 0
    for rows, mid in p.draws:
        assert plain.train_batch(rows, mask_id=mid) == graph.train_batch(rows, mask_id=mid) == p.B
    for name, a, b in zip(("params", "adam_m", "adam_v", "shadow", "shadow_t"), all_bits(plain.engine), all_bits(graph.engine)):
        assert np.array_equal(a, b), "graph replay: %s differs from six plain steps at %d elements" % (name, int((a != b).sum()))
    assert np.array_equal(bits(plain.trust_ratios()), bits(graph.trust_ratios()))
    assert graph.engine.graph_captures() == 1


def test_tied_weights_one_ratio_per_free_matrix_and_a_mirrored_decoder():
    p = problem("chain")
    tool = tool_of("lamb", warmup=2, total=6, min_factor=0.01)
    tr = trainer_for(p, tool, tied_weights=True)
    eng = tr.engine
    n_free = (eng.L + 1) // 2
    for i, (rows, mid) in enumerate(p.draws[:3]):
        before = read_state(eng)
        hp = eng.hyper(HY["lr"], HY["wd"], clip=1.0, global_rows=p.B, step=eng.step_count + 1)
        tr.train_batch(rows, mask_id=mid)
        torch.cuda.synchronize()
        before["g"] = eng.grads.cpu().numpy().copy()                            # (the folded gradient: the decoder ranges are +0)
        # the free matrices and every bias as the restatement has them; the decoder's moments were never touched
        got = read_state(eng)
        ratios = eng.trust_ratios().cpu().numpy()
        assert ratios.shape == (n_free,)
        h = AR.hyper_of_struct(hp)
        coef = coef_of(before["g"], hp, eng.read_scalars()[2], "tied step %d" % i)
        for name, lo, hi, is_mat, ri in tensors_of(eng, n_free):
            check_tensor({k: before[k][lo:hi] for k in "pgmv"}, {k: got[k][lo:hi] for k in "pmv"}, ratios[ri] if is_mat else None, h,
                         TR.trust_of(tool), coef, is_mat, "tied step %d %s" % (i, name))
        for l in range(n_free, eng.L):
            k, n, _ = eng.schedule[l]
            lo, hi = eng.w_off[l], eng.w_off[l] + n * k
            assert np.array_equal(bits(got["m"][lo:hi]), bits(before["m"][lo:hi])) and np.array_equal(bits(got["v"][lo:hi]), bits(before["v"][lo:hi]))
            assert torch.equal(eng.weight(l), eng.weight(eng.L - 1 - l).t()), "layer %d is not the mirror of layer %d" % (l, eng.L - 1 - l)
        check_shadows(eng, got["p"], "tied step %d" % i)


def test_weight_average_rides_along_and_save_load_continues_bit_for_bit(tmp_path):
    from codae.hip import HipError
    from codae.tool import Optimizer, WeightAverage
    p = problem("layers")
    tool = tool_of("lamb", warmup=2, total=6, min_factor=0.01)
    avg = WeightAverage("ema", decay=0.9, debias=False)
    s = AVR.setting_of(avg)
    whole, bare = trainer_for(p, tool, weight_average=avg), trainer_for(p, tool)
    path = str(tmp_path / "lamb.ckpt")
    for i, (rows, mid) in enumerate(p.draws):
        a0 = whole.engine.weight_avg.cpu().numpy().copy()
        whole.train_batch(rows, mask_id=mid)
        bare.train_batch(rows, mask_id=mid)
        torch.cuda.synchronize()
        # the average is the stand-alone definition applied to the parameters this update produced
        p1 = whole.engine.params.cpu().numpy()
        w32 = AVR.weight32(s, i + 1)
        got = whole.engine.weight_avg.cpu().numpy()
        live = live_mask(whole.engine)
        r = AVR.worst_ratio(got[live], AVR.step64(a0[live], p1[live], w32), AVR.bound(a0[live], p1[live]))
        assert r <= 1.0, "step %d: the average is %.3f bounds from its definition" % (i, r)
        if i == 2:
            whole.save(path)
    # parameters, moments and shadows are those of the same steps without the average
    for name, a, b in zip(("params", "adam_m", "adam_v", "shadow", "shadow_t"), all_bits(whole.engine), all_bits(bare.engine)):
        assert np.array_equal(a, b), "%s differs under the weight average" % name
    # load, then the same three steps: bit for bit the uninterrupted run
    again = trainer_for(p, tool, weight_average=avg)
    again.load(path)
    for rows, mid in p.draws[3:]:
        again.train_batch(rows, mask_id=mid)
    a, b = whole.state_digest(), again.state_digest()
    assert a == b, "resumed run differs: %s" % sorted(k for k in a if a[k] != b[k])
    assert np.array_equal(bits(whole.trust_ratios()), bits(again.trust_ratios()))
    # a file written under lamb is refused by a trainer of another kind, and the other way round
    other = trainer_for(p, Optimizer("adamw"), weight_average=avg)
    was = other.state_digest()
    with pytest.raises(HipError, match="optimizer"):
        other.load(path)
    assert other.state_digest() == was
    other_path = str(tmp_path / "adamw.ckpt")
    other.save(other_path)
    with pytest.raises(HipError, match="optimizer"):
        again.load(other_path)
    lars = trainer_for(p, tool_of("lars"), weight_average=avg)
    with pytest.raises(HipError, match="optimizer"):
        lars.load(path)
