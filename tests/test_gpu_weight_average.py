"""The weight average (include/codae_hip.h, "Weight average") on the device, against the float64 restatement of
tests/average_ref.py at the bound tests/test_weight_average_host.py fixes on the CPU: |a' - a'_64| <= 3 u (|a| + |p'|).

  A. codae_weight_average_update alone: n = 1, 5 (tail alone), 64 (float4 body alone), 1000, 4099 (body + tail); EMA and SWA; a step
     with w32 < 1, one with w32 == 1 (bit copy) and one that does not sample (bit-identical avg); 16 guard elements untouched.
  B. codae_step_update on planted state, bf16 72 -> 136 -> 72 (tiled kernel), the same under CODAE_FLAT_ADAM=1 (set before the engine
     is created, the way tests/test_gpu_optimizer.py switches it) and fp32 48 -> 16 -> 48 (flat kernel); adam and sgd; t = 1 and 1000:
     avg' against the definition applied to the p' of the same launch, everything else bit-identical to the update without it.
  C. whole steps on the chain form and the per-layer form: SWA is the float64 mean of the snapshots, EMA follows its recurrence.
  D. graph replay: bit-identical to plain steps, one capture, a changed setting captures again.
  E. tied weights: the update never writes the decoder ranges of the average; the synchronised average is tied.
  F. evaluation on the average is evaluation of a trainer that has the average loaded; it does not disturb training.
  G. off is a no-op; the sharded update, unknown `weights` and an average that is not kept are refused; NaN propagates.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import average_ref as AR
import optim_ref as OR
from test_gpu_optimizer import bits, clip_values, live_mask, plant, set_env, shapes, _square, _widths
from test_gpu_optimizer_kinds import HY, tool_opt

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"


@pytest.fixture
def hip():
    from codae import hip as H
    H.lib()
    return H


def WA(*a, **k):
    from codae.tool import WeightAverage
    return WeightAverage(*a, **k)


def check_avg(got, a, p, w32, what, live=None):
    """got against the float64 definition of (a, p', w32) at the host test's bound; bit rules at w32 == 1 and without a sample."""
    live = np.ones(a.size, dtype=bool) if live is None else live
    want, tol = AR.step64(a[live], p[live], w32), AR.bound(a[live], p[live])
    r = AR.worst_ratio(got[live], want, tol)
    print("MEASURE weight average %s: w32 %r  worst |error| / bound %.3f" % (what, w32, r))
    assert r <= 1.0, "%s: %.3f bounds from the float64 definition" % (what, r)
    if w32 is None:
        assert np.array_equal(bits(got), bits(a)), "%s: avg moved on a step that does not sample" % what
    elif w32 == np.float32(1):
        assert np.array_equal(bits(got[live]), bits(p[live])), "%s: not a bit copy at w32 == 1" % what
    return r


# ---- A. the stand-alone entry ------------------------------------------------------------------------------------------------
ALONE = {"ema": (dict(kind="ema", decay=0.9, debias=False, start=1, every=2), {"blend": 3, "copy": 1, "skip": 2}),
         "ema-debias": (dict(kind="ema", decay=0.999, debias=True, start=1, every=1), {"blend": 4, "copy": 1}),
         "swa": (dict(kind="swa", start=3, every=1), {"blend": 5, "copy": 3, "skip": 2})}


@pytest.mark.parametrize("case", sorted(ALONE))
@pytest.mark.parametrize("n", (1, 5, 64, 1000, 4099))
def test_update_entry_point(hip, n, case):
    kw, steps = ALONE[case]
    tool = WA(**kw)
    s = AR.setting_of(tool)
    a, p = AR.planted(n, 40 + n)
    guard = np.float32(123.25)
    for name, t in steps.items():
        w = AR.weight32(s, t)
        assert {"blend": w is not None and w < 1, "copy": w == np.float32(1), "skip": w is None}[name], (case, name, w)
        assert tool.weight(t) == (None if w is None else float(w))
        da = torch.full((n + 16,), float(guard), dtype=torch.float32, device=DEV)
        dp = torch.full((n + 16,), float(guard), dtype=torch.float32, device=DEV)
        da[:n].copy_(torch.from_numpy(a))
        dp[:n].copy_(torch.from_numpy(p))
        st = tool.as_struct(None)
        hip.check(hip.lib().codae_weight_average_update(hip.ptr(da), hip.ptr(dp), n, C.byref(st), t, hip.current_stream()))
        torch.cuda.synchronize()
        got, gp = da.cpu().numpy(), dp.cpu().numpy()
        what = "entry n %d %s %s t %d" % (n, case, name, t)
        check_avg(got[:n], a, p, w, what)
        assert (got[n:] == guard).all() and (gp[n:] == guard).all(), "%s: wrote behind n" % what
        assert np.array_equal(bits(gp[:n]), bits(p)), "%s: p was written" % what
        # the tool's own route to the same entry
        db = torch.from_numpy(a).to(DEV)
        tool.update(db, dp[:n].clone(), t)
        assert np.array_equal(bits(db), bits(got[:n])), what


def test_update_entry_point_refuses_a_bad_call(hip):
    a = torch.zeros(64, dtype=torch.float32, device=DEV)
    S = hip.WeightAverage
    lib = hip.lib()
    call = lambda st, av, n=32, t=1: lib.codae_weight_average_update(av, hip.ptr(a), n, C.byref(st), t, hip.current_stream())
    ok = S(hip.AVG_EMA, 0.9, 0, 1, 1, None)
    assert call(S(hip.AVG_EMA, 1.5, 0, 1, 1, None), hip.ptr(a[32:])) == -1
    assert call(S(9, 0.5, 0, 1, 1, None), hip.ptr(a[32:])) == -1
    assert call(ok, C.c_void_p(a.data_ptr() + 4)) == -1 and call(ok, None) == -1
    assert call(ok, hip.ptr(a[32:]), n=0) == -1 and call(ok, hip.ptr(a[32:]), t=0) == -1
    torch.cuda.synchronize()
    assert (a == 0).all()


# ---- B. the engine's update on planted state ---------------------------------------------------------------------------------
STACKS = {"bf16": ("bf16", {}, _widths([72, 136, 72])), "bf16-flat": ("bf16", {"CODAE_FLAT_ADAM": "1"}, _widths([72, 136, 72])),
          "f32": ("f32", {}, _widths([48, 16, 48]))}


@functools.lru_cache(maxsize=None)
def planted(stack, first_step):
    """Computed once per (stack, first step) and left unchanged: the optimizer state, and an average to start from."""
    sched = STACKS[stack][2]
    state = OR.planted_state(shapes(sched), 9300 + sorted(STACKS).index(stack), first_step, HY["wd"])
    rng = np.random.default_rng(77 + sorted(STACKS).index(stack))
    return state, [(s["p"] + rng.standard_normal(s["p"].shape).astype(np.float32) * np.float32(0.01)).astype(np.float32) for s in state]


def plant_avg(eng, avgs):
    from test_gpu_optimizer import tensor_ids
    eng.weight_avg.zero_()
    for (l, is_bias), a in zip(tensor_ids(eng), avgs):
        eng._view(eng.weight_avg, l, is_bias).copy_(torch.from_numpy(a))
    torch.cuda.synchronize()
    return eng.weight_avg.cpu().numpy().copy()


def state_bits(eng):
    torch.cuda.synchronize()
    ts = {"params": eng.params, "adam_m": eng.adam_m, "adam_v": eng.adam_v}
    if eng.shadow is not None:
        ts.update(shadow=eng.shadow, shadow_t=eng.shadow_t)
    return {k: bits(t).copy() for k, t in ts.items()}


B_SETTINGS = {"ema": dict(kind="ema", decay=0.9, debias=False), "swa": dict(kind="swa"), "skip": dict(kind="ema", decay=0.9, every=2, start=2)}


@pytest.mark.parametrize("kind", ("adam", "sgd"))
@pytest.mark.parametrize("stack", sorted(STACKS))
def test_step_update_on_planted_state(stack, kind, monkeypatch):
    from codae.hip.engine import DaeEngine
    prec, env, sched = STACKS[stack]
    set_env(monkeypatch, env)
    opt = None if kind == "adam" else tool_opt("sgd")
    plain, eng = DaeEngine(sched, 16, prec, DEV), DaeEngine(sched, 16, prec, DEV)
    for e in (plain, eng):
        e.set_optimizer(opt)
    live = live_mask(eng)
    for name, kw in B_SETTINGS.items():
        tool = WA(**kw)
        s = AR.setting_of(tool)
        eng.set_weight_average(tool)
        assert eng.weight_avg is not None and eng.weight_avg.numel() == eng.n_param and (eng.avg_shadow is not None) == (prec == "bf16")
        for t in (1, 1000):
            state, avgs = planted(stack, t == 1)
            before = plant(eng, state)
            plant(plain, state)
            a = plant_avg(eng, avgs)
            hp = eng.hyper(HY["lr"], HY["wd"], clip=clip_values(before[1])["on"], betas=HY["betas"], eps=HY["eps"], step=t)
            eng.step_update(hp)
            plain.step_update(hp)
            what = "planted %s %s %s t %d" % (stack, kind, name, t)
            got, want = state_bits(eng), state_bits(plain)
            for k in want:
                assert np.array_equal(got[k], want[k]), "%s: %s differs from the update without averaging" % (what, k)
            assert not np.array_equal(got["params"], bits(before[0])), what
            p_new = eng.params.cpu().numpy()
            avg = eng.weight_avg.cpu().numpy()
            w = AR.weight32(s, t)
            assert (w is None) == (name == "skip" and t == 1), (what, w)
            check_avg(avg, a, p_new, w, what, live=live)
            assert (avg[~live] == 0).all(), "%s: the padding of avg moved" % what
            assert np.array_equal(bits(eng.grads), bits(before[1])), "%s: the update wrote into grads" % what


# ---- C - G. whole steps ------------------------------------------------------------------------------------------------------
# form -> (precision, schedule, batch rows, the path codae_step_path must report)
WHOLE = {"chain": ("bf16", _square(192, 4), 64, "chain"), "layers": ("bf16", _widths([72, 136, 72]), 16, "layers"),
         "f32": ("f32", _widths([48, 16, 48]), 16, "layers")}
N_STEPS = 6


class Problem:
    pass


@functools.lru_cache(maxsize=None)
def problem(form):
    from oracle import dae_oracle as O
    p = Problem()
    p.prec, p.sched, p.B, p.path = WHOLE[form]
    io = p.sched[0][0]
    assert io % 3 == 0 and p.sched[-1][1] == io
    rng = np.random.default_rng(8300 + io)
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


def trainer_for(p, **kw):
    from codae.train import HipEmbeddingTrainer
    tr = HipEmbeddingTrainer(p.sched, p.data, p.table, None, HY["lr"], HY["wd"], clip=1.0, max_batch=p.B, precision=p.prec, device=DEV, **kw)
    tr.load_params(p.params)
    return tr


def assert_same_training_state(a, b, what):
    x, y = state_bits(a.engine), state_bits(b.engine)
    for k in x:
        assert np.array_equal(x[k], y[k]), "%s: %s differs at %d elements" % (what, k, int((x[k] != y[k]).sum()))


def flat(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


@pytest.mark.parametrize("form", ("chain", "layers"))
def test_swa_is_the_mean_of_the_snapshots_and_ema_follows_its_recurrence(form):
    p = problem(form)
    plain = trainer_for(p)
    swa = trainer_for(p, weight_average=WA("swa"))
    ema_tool = WA("ema", decay=0.9, debias=False, start=2, every=2)
    ema = trainer_for(p, weight_average=ema_tool)
    assert swa.engine.step_path(p.B) == p.path == plain.engine.step_path(p.B)
    live = live_mask(plain.engine)
    p0 = flat(plain.engine.params)
    assert np.array_equal(bits(flat(swa.engine.weight_avg)), bits(p0)), "the average does not start as a copy of the parameters"
    snaps = []
    s = AR.setting_of(ema_tool)
    a64, tol = p0.astype(np.float64), np.zeros(p0.size)
    for t, (rows, mid) in enumerate(p.draws, start=1):
        for tr in (plain, swa, ema):
            assert tr.train_batch(rows, mask_id=mid) == p.B
        snaps.append(flat(plain.engine.params))
        w = AR.weight32(s, t)
        if t == 1:
            assert w is None and np.array_equal(bits(flat(ema.engine.weight_avg)), bits(p0)), "%s: avg moved before start" % form
        if w is not None:
            # every sampled step adds at most its own bound to what the earlier ones left, which it shrinks by 1 - w32
            if w == 1:
                a64, tol = snaps[-1].astype(np.float64), np.zeros(p0.size)               # (a bit copy: nothing is left of the past)
            else:
                tol = (1.0 - float(w)) * tol + AR.bound(a64, snaps[-1]) * (1 + 8 * AR.U)
                a64 = a64 + float(w) * (snaps[-1].astype(np.float64) - a64)
    assert_same_training_state(plain, swa, form + " swa")
    assert_same_training_state(plain, ema, form + " ema")
    mean = np.mean(np.stack([x.astype(np.float64) for x in snaps]), axis=0)
    got = flat(swa.engine.weight_avg)
    r = AR.worst_ratio(got[live], mean[live], AR.swa_mean_bound(snaps)[live])
    print("MEASURE weight average whole %s: swa over %d steps, worst |error| / bound %.3f" % (form, N_STEPS, r))
    assert r <= 1.0 and (got[~live] == 0).all()
    assert np.abs(snaps[-1] - snaps[0]).max() > 1e-3                                  # (the parameters did move)
    got = flat(ema.engine.weight_avg)
    r = AR.worst_ratio(got[live], a64[live], tol[live])
    print("MEASURE weight average whole %s: ema (0.9, start 2, every 2), worst |error| / bound %.3f" % (form, r))
    assert r <= 1.0 and (got[~live] == 0).all()


def test_graph_replay_is_plain_steps_bit_for_bit_with_one_capture():
    p = problem("chain")
    tool = WA("ema", decay=0.999, debias=True)                    # (six different weights, one graph)
    assert len({tool.weight(t) for t in range(1, N_STEPS + 1)}) == N_STEPS
    plain, graph = trainer_for(p, weight_average=tool), trainer_for(p, weight_average=tool, use_graph=True)
    assert graph.engine.step_path(p.B) == "chain" and graph.engine.graph_captures() == 0
    for rows, mid in p.draws:
        assert plain.train_batch(rows, mask_id=mid) == graph.train_batch(rows, mask_id=mid) == p.B
    assert_same_training_state(plain, graph, "graph replay")
    a, b = bits(flat(plain.engine.weight_avg)), bits(flat(graph.engine.weight_avg))
    assert np.array_equal(a, b), "graph replay: weight_avg differs from six plain steps at %d elements" % int((a != b).sum())
    assert not np.array_equal(a, bits(flat(plain.engine.params)))
    assert graph.engine.graph_captures() == 1
    graph.set_weight_average(WA("ema", decay=0.99, debias=True))
    graph.train_batch(p.draws[0][0], mask_id=p.draws[0][1])
    torch.cuda.synchronize()
    assert graph.engine.graph_captures() == 2


def test_tied_weights_average_the_free_parameters_only():
    p = problem("chain")
    tr = trainer_for(p, tied_weights=True, weight_average=WA("swa"))
    plain = trainer_for(p, tied_weights=True)
    eng = tr.engine
    pairs = eng.tie_pairs()
    assert len(pairs) == 2
    sentinel = 123.25
    for _, dec, rows, cols in pairs:
        eng.weight_avg[dec:dec + rows * cols] = sentinel
    snaps = []
    for rows, mid in p.draws[:3]:
        tr.train_batch(rows, mask_id=mid)
        plain.train_batch(rows, mask_id=mid)
        snaps.append(flat(eng.params))
    assert_same_training_state(plain, tr, "tied")
    raw = flat(eng.weight_avg)
    for _, dec, rows, cols in pairs:
        assert (raw[dec:dec + rows * cols] == sentinel).all(), "the update wrote a decoder range of the average"
    avg = [(flat(w), flat(b)) for w, b in tr.average_params()]
    for l in range(eng.L // 2):
        assert np.array_equal(bits(avg[eng.L - 1 - l][0]), bits(np.ascontiguousarray(avg[l][0].T))), "layer %d of the average is not tied" % l
    free = live_mask(eng)
    for _, dec, rows, cols in pairs:
        free[dec:dec + rows * cols] = False
    mean = np.mean(np.stack([x.astype(np.float64) for x in snaps]), axis=0)
    r = AR.worst_ratio(flat(eng.weight_avg)[free], mean[free], AR.swa_mean_bound(snaps)[free])
    assert r <= 1.0, r
    if eng.avg_shadow is not None:
        n = eng.n_param
        assert np.array_equal(bits(eng.avg_shadow)[:n], bits(eng.weight_avg.bfloat16()))


@pytest.mark.parametrize("form", sorted(WHOLE))
def test_evaluation_on_the_average(form, monkeypatch):
    p = problem(form)
    set_env(monkeypatch, {"CODAE_NO_CHAIN": "1"})          # the trainer that has the average LOADED runs the per-layer forward, which
    other = trainer_for(p)                                 # is what an averaged evaluation runs (it keeps no transposed image)
    set_env(monkeypatch, {})
    plain = trainer_for(p)
    tr = trainer_for(p, weight_average=WA("ema", decay=0.5, debias=False))
    assert tr.engine.step_path(p.B) == p.path
    rows = p.draws[5][0]
    for i, (r, mid) in enumerate(p.draws[:4]):
        if i == 2:
            # an averaged evaluation between two steps: the workspaces are shared, the live images must not be disturbed
            live_before = tr.eval_batch(rows, want_y=True)
            tr.epoch_sums()
            y_mid = tr.eval_batch(rows, want_y=True, weights="average")
            assert not np.array_equal(bits(y_mid), bits(live_before))
            assert np.array_equal(bits(tr.eval_batch(rows, want_y=True)), bits(live_before)), "%s: the live images were disturbed" % form
            tr.epoch_sums()
            plain.eval_batch(rows)
            plain.epoch_sums()
        tr.train_batch(r, mask_id=mid)
        plain.train_batch(r, mask_id=mid)
    assert_same_training_state(plain, tr, form + " with an averaged evaluation in between")
    assert np.array_equal(bits(tr.eval_batch(rows, want_y=True)), bits(plain.eval_batch(rows, want_y=True))), "weights='live' changed"
    tr.epoch_sums()
    y = tr.eval_batch(rows, want_y=True, weights="average")
    sums = tr.epoch_sums()
    other.load_params([(w.clone(), b.clone()) for w, b in tr.average_params()])
    other.epoch_sums()
    y2 = other.eval_batch(rows, want_y=True)
    sums2 = other.epoch_sums()
    assert np.array_equal(bits(y), bits(y2)), "%s: %d elements differ from a trainer with the average loaded" % (form, int((bits(y) != bits(y2)).sum()))
    assert sums == sums2 and sums[0] > 0, (sums, sums2)
    assert not np.array_equal(bits(y), bits(tr.eval_batch(rows, want_y=True)))
    assert [np.array_equal(bits(a), bits(b)) for (a, _), (b, _) in zip(tr.params(average=True), tr.average_params())] == [True] * tr.engine.L
    idx, score = tr.complete(rows[:8], 1, 5, weights="average")
    idx2, score2 = other.complete(rows[:8], 1, 5)
    assert torch.equal(idx, idx2) and np.array_equal(bits(score), bits(score2))
    # load_average / reset_average
    tr.load_average(p.params)
    assert np.array_equal(bits(tr.average_params()[0][0]), bits(torch.as_tensor(p.params[0][0])))
    tr.reset_average()
    assert np.array_equal(bits(tr.engine.weight_avg), bits(tr.engine.params))
    assert np.array_equal(bits(tr.eval_batch(rows, want_y=True, weights="average")), bits(tr.eval_batch(rows, want_y=True)))


@pytest.mark.parametrize("form", ("chain", "layers"))
def test_off_is_a_no_op(form):
    p = problem(form)
    trs = [trainer_for(p), trainer_for(p, weight_average=None), trainer_for(p, weight_average=WA(kind="off"))]
    for rows, mid in p.draws[:3]:
        for tr in trs:
            tr.train_batch(rows, mask_id=mid)
    for tr in trs[1:]:
        assert tr.engine.weight_avg is None and tr.engine.avg_bufs is None
        assert_same_training_state(trs[0], tr, form + " off")


def test_refusals(hip):
    from codae.hip.engine import DaeEngine
    from codae.train import DataParallel
    p = problem("layers")
    tr = trainer_for(p)
    with pytest.raises(hip.HipError, match="average"):
        tr.eval_batch(p.draws[0][0], weights="average")
    with pytest.raises(hip.HipError, match="weights"):
        tr.eval_batch(p.draws[0][0], weights="mean")
    with pytest.raises(hip.HipError):
        tr.average_params()
    tr.set_weight_average(WA("swa"))
    tr.set_weight_average(None)                                   # switched off again: the average stays readable, not evaluable
    with pytest.raises(hip.HipError, match="average"):
        tr.eval_batch(p.draws[0][0], weights="average")
    with pytest.raises(hip.HipError):
        tr.engine.set_weight_average("ema")
    # the sharded update
    prec, _, sched = STACKS["f32"]
    eng = DaeEngine(sched, 16, prec, DEV)
    eng.set_weight_average(WA("ema"))
    state, avgs = planted("f32", False)
    before = plant(eng, state)
    a = plant_avg(eng, avgs)
    hp = eng.hyper(HY["lr"], HY["wd"], clip=0.0, step=5)
    acc = eng.new_accumulator()
    with pytest.raises(hip.HipError, match="-3.*weight average"):
        eng.step_update_span(hp, 0, 64, acc)
    torch.cuda.synchronize()
    for name, t, want in (("params", eng.params, before[0]), ("adam_m", eng.adam_m, before[2]), ("adam_v", eng.adam_v, before[3]),
                          ("weight_avg", eng.weight_avg, a)):
        assert np.array_equal(bits(t), bits(want)), "the refused span update wrote %s" % name
    with pytest.raises(hip.HipError, match="sharded"):
        DataParallel(eng, sharded=True)
    dp = DataParallel(DaeEngine(sched, 16, prec, DEV), sharded=True)
    dp.engine.set_weight_average(WA("ema"))
    with pytest.raises(hip.HipError, match="sharded"):
        dp._refuse_sharded_average()
    # a refused setting leaves the previous one in force
    with pytest.raises(hip.HipError):
        eng._set_average_struct(hip.WeightAverage(hip.AVG_EMA, 1.0, 0, 1, 1, hip.ptr(eng.weight_avg)))
    plant(eng, state)
    plant_avg(eng, avgs)
    eng.step_update(hp)
    assert not np.array_equal(bits(eng.weight_avg), bits(a)), "the refused setting switched averaging off"


def test_nan_propagates_into_the_average():
    from codae.hip.engine import DaeEngine
    prec, _, sched = STACKS["f32"]
    eng = DaeEngine(sched, 16, prec, DEV)
    eng.set_weight_average(WA("ema", decay=0.9, debias=False))
    state, avgs = planted("f32", False)
    live = live_mask(eng)
    i = int(np.flatnonzero(live)[417])
    for clip, everywhere in ((0.0, False), (1.0, True)):
        plant(eng, state)
        plant_avg(eng, avgs)
        eng.grads[i] = float("nan")
        eng.step_update(eng.hyper(HY["lr"], HY["wd"], clip=clip, step=7))
        pn, an = np.isnan(flat(eng.params)), np.isnan(flat(eng.weight_avg))
        assert np.array_equal(pn, an), "clip %r: the average is NaN at other elements than the parameters" % clip
        assert an[i] and (an[live].all() if everywhere else an.sum() == 1), (clip, int(an.sum()))
