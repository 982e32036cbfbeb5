"""Every optimizer-update path against a float64 Adam fed the same fp32 inputs (tests/adam_ref.py), at rounding-level bounds.

All update paths read eng.grads, and codae_step_update runs on whatever the caller left in grads, params, adam_m and adam_v, so
the optimizer is tested apart from the GEMMs: plant the state, run the update, compare (part A); or take a real step, read back
the gradients it consumed, and compare with the reference applied to the state cloned before the step (part B) - the next step
starts from the engine's own state, so nothing compounds.  Part C is the stand-alone codae_clip_adam.

What every case asserts (check_update):
  - params, adam_m, adam_v within adam_ref.bounds() of adam_ref.adam_step64 at every element of every weight and bias; the
    bounds are fixed by tests/test_adam_host.py against an fp32 emulation, never by a GPU run;
  - with clipping on, the grad-square scalar (read_scalars()[2]) within 1e-6 relative of the float64 sum g^2 - its terms are
    fp32 squares - and the reference's coefficient comes from that scalar through clip_coef32.  With clip = 0 no step form
    computes the scalar (include/codae_hip.h: max_grad_norm <= 0 disables clipping), so there is nothing to read;
  - bf16: shadow[:n_param] == params.bfloat16() bit for bit; for every layer l >= 1 the layer's region of shadow_t is the
    transpose of its region of shadow bit for bit (layer 0 has no data gradient: not specified); the slack of both shadows
    behind n_param is still zero;
  - params, adam_m, adam_v outside every weight and bias view are still exactly 0; in part A grads is unchanged bit for bit.
One MEASURE line per case: the worst |error| / bound for p, m and v.

Part A shapes ([out][in] per layer; the tiled kernel walks 64 x 128 tiles, 8-row groups on the transposed sweep):
  ragged  192 -> 136 -> 72 -> 40 -> 72 -> 136 -> 192: 136 x 192 (two row tiles + 8 rows, one and a half column tiles), 72 x 136
          (a column tile 8 wide, 64 + 8 rows), 40 x 72 and 72 x 40 (a single partial tile) and their mirrors
  tiny    8 -> 16 -> 8, the smallest legal widths
  deep    64 layers of 64 x 64: the ABI's layer limit, every entry of the kernel's job arrays in use
  f32     30 -> 20 -> 11 -> 20 -> 30: the pad elements sit between the tensors of the flat vectors
"""
import ctypes as C
import functools

import numpy as np
import pytest

import adam_ref as AR

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"

HYPERS = {"a": dict(lr=1e-3, wd=1e-2, betas=(0.9, 0.999), eps=1e-8),
          "b": dict(lr=3e-2, wd=0.0, betas=(0.8, 0.95), eps=1e-6),
          "c": dict(lr=1e-5, wd=1e-4, betas=(0.9, 0.999), eps=1e-8)}
STEPS = (1, 2, 7, 1000)
CLIPS = ("off", "on", "loose")


def _widths(ws):
    return [(ws[i], ws[i + 1], i + 2 < len(ws)) for i in range(len(ws) - 1)]


def _square(io, n_layers):
    return [(io, io, l + 1 < n_layers) for l in range(n_layers)]


RAGGED = _widths([192, 136, 72, 40, 72, 136, 192])
# engine form -> (precision, CODAE_* switches set before the engine is created, schedule)
PLANTED = {
    "tiled-ragged": ("bf16", {}, RAGGED),
    "tiled-tiny": ("bf16", {}, _widths([8, 16, 8])),
    "tiled-deep": ("bf16", {}, _square(64, 64)),
    "flat-ragged": ("bf16", {"CODAE_FLAT_ADAM": "1"}, RAGGED),
    "flat-tiny": ("bf16", {"CODAE_FLAT_ADAM": "1"}, _widths([8, 16, 8])),
    "flat-deep": ("bf16", {"CODAE_FLAT_ADAM": "1"}, _square(64, 64)),
    "f32": ("f32", {}, _widths([30, 20, 11, 20, 30])),
}


@pytest.fixture
def hip():
    from codae import hip as H
    H.lib()
    return H


def bits(a):
    """The bit patterns of an fp32 / bf16 tensor or array, as integers."""
    if isinstance(a, np.ndarray):
        return a.view(np.uint32)
    if a.dtype == torch.bfloat16:
        return a.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)
    return a.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32)


def tensor_ids(eng):
    """(layer, is_bias) in the order planted_state's shapes are listed: every weight, then every bias."""
    return [(l, False) for l in range(eng.L)] + [(l, True) for l in range(eng.L)]


def shapes(sched):
    return [(n, k) for k, n, _ in sched] + [(n,) for _, n, _ in sched]


def live_mask(eng):
    live = np.zeros(eng.n_param, dtype=bool)
    for l, (k, n, _) in enumerate(eng.schedule):
        live[eng.w_off[l]:eng.w_off[l] + n * k] = True
        live[eng.b_off[l]:eng.b_off[l] + n] = True
    return live


@functools.lru_cache(maxsize=None)
def planted(form, first_step, wd):
    """Computed once per (schedule, first step, decay) and left unchanged."""
    return AR.planted_state(shapes(PLANTED[form][2]), 9000 + sorted(PLANTED).index(form), first_step, wd)


def plant(eng, state):
    """Through weight(l) / bias(l) and the same views of grads, adam_m, adam_v; then sync_shadows().  Returns the flat vectors as
    the device holds them (P, G, M, V float32 numpy)."""
    flats = (("p", eng._params), ("g", eng.grads), ("m", eng.adam_m), ("v", eng.adam_v))
    for (l, is_bias), s in zip(tensor_ids(eng), state):
        for key, flat in flats:
            eng._view(flat, l, is_bias).copy_(torch.from_numpy(s[key]))
    eng.sync_shadows()
    torch.cuda.synchronize()
    return tuple(flat.cpu().numpy().copy() for _, flat in flats)


def clip_values(G):
    """off, one that triggers, one that does not - from the float64 norm of the gradient (+ the coefficient's own 1e-6, so that an
    all-zero gradient still has a value that triggers)."""
    norm = float(np.sqrt((G.astype(np.float64) ** 2).sum()))
    return {"off": 0.0, "on": 0.01 * (norm + 1e-6), "loose": 100.0 * (norm + 1e-6)}


def check_update(eng, before, hp, what, grad_sq=None, got=None, branch=None):
    """The module docstring's assertions for one update from `before` = (P, G, M, V) flat fp32 arrays under the struct `hp`.
    got: (p, m, v) flat arrays when they do not come from an engine (part C).  Returns (coef, ratios)."""
    torch.cuda.synchronize()
    P, G, M, V = before
    h = AR.hyper_of_struct(hp)
    clip = float(hp.max_grad_norm)
    coef = np.float32(1.0)
    if clip > 0:
        gsq = eng.read_scalars()[2] if grad_sq is None else grad_sq
        want_sq = float((G.astype(np.float64) ** 2).sum())
        assert abs(gsq - want_sq) <= 1e-6 * want_sq, "%s: grad-square scalar %.17g, float64 sum g^2 %.17g" % (what, gsq, want_sq)
        coef = AR.clip_coef32(gsq, clip)
    if branch is not None:
        assert (coef < 1) == (branch == "on"), "%s: clip %s but the coefficient is %r" % (what, branch, coef)
    live = np.ones(P.size, dtype=bool) if eng is None else live_mask(eng)
    if got is None:
        got = tuple(t.cpu().numpy() for t in (eng.params, eng.adam_m, eng.adam_v))
    args = (P[live], G[live], M[live], V[live], h, coef)
    want = AR.adam_step64(*args)
    tol = AR.bounds(*args)
    ratios = AR.worst_ratios([a[live] for a in got], want, tol)
    print("MEASURE optimizer %s: t %d coef %.6g  worst |error| / bound  p %.3f  m %.3f  v %.3f" % ((what, h.t, float(coef)) + ratios))
    for name, a, w, t, r in zip("pmv", got, want, tol, ratios):
        if not r <= 1.0:
            e = np.abs(a[live].astype(np.float64) - w)
            with np.errstate(divide="ignore", invalid="ignore"):
                i = int(np.argmax(np.where(e == 0, 0.0, e / t)))
            flat_i = int(np.flatnonzero(live)[i])
            raise AssertionError("%s: %s is %.3f bounds from the float64 Adam at flat element %d: got %.9g want %.9g bound %.3g "
                                 "(p %.9g g %.9g m %.9g v %.9g)" % (what, name, r, flat_i, a[flat_i], w[i], t[i], P[flat_i], G[flat_i],
                                                                    M[flat_i], V[flat_i]))
        assert (a[~live] == 0).all(), "%s: a pad element of %s moved" % (what, name)
    if eng is not None and eng.shadow is not None:
        check_shadows(eng, got[0], what)
    return coef, ratios


def check_shadows(eng, p, what):
    n = eng.n_param
    sh, sht = bits(eng.shadow), bits(eng.shadow_t)
    want = bits(torch.from_numpy(np.ascontiguousarray(p)).bfloat16())
    bad = np.flatnonzero(sh[:n] != want)
    assert bad.size == 0, "%s: shadow differs from params.bfloat16() at %d elements, first flat %d" % (what, bad.size, bad[0])
    for l in range(1, eng.L):
        k, nn, _ = eng.schedule[l]
        o = eng.w_off[l]
        w = sh[o:o + nn * k].reshape(nn, k)
        wt = sht[o:o + nn * k].reshape(k, nn)
        bad = np.argwhere(wt != w.T)
        assert bad.size == 0, "%s: layer %d: shadow_t is not the transpose of shadow at %d elements, first [in %d][out %d]" % (
            what, l, len(bad), bad[0][0], bad[0][1])
    assert (sh[n:] == 0).all() and (sht[n:] == 0).all(), "%s: the slack behind n_param moved" % what


def set_env(monkeypatch, env):
    """(codae_create reads the switches: set before the engine is made, gone again after the test)"""
    for k in ("CODAE_FLAT_ADAM", "CODAE_NO_CHAIN"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ---- A. update kernels on planted state -------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", STEPS)
@pytest.mark.parametrize("hy", sorted(HYPERS))
@pytest.mark.parametrize("form", sorted(PLANTED))
def test_step_update_on_planted_state(form, hy, t, monkeypatch):
    from codae.hip.engine import DaeEngine
    prec, env, sched = PLANTED[form]
    set_env(monkeypatch, env)
    H = HYPERS[hy]
    eng = DaeEngine(sched, 16, prec, DEV)
    state = planted(form, t == 1, H["wd"])
    for branch in CLIPS:
        before = plant(eng, state)
        assert before[0][live_mask(eng)].all() and (before[1] != 0).any() and ((before[3] != 0).any() or t == 1)
        clip = clip_values(before[1])[branch]
        hp = eng.hyper(H["lr"], H["wd"], clip=clip, betas=H["betas"], eps=H["eps"], step=t)
        eng.step_update(hp)
        what = "planted %s %s clip %s" % (form, hy, branch)
        check_update(eng, before, hp, what, branch=branch)
        assert np.array_equal(bits(eng.grads), bits(before[1])), "%s: the update wrote into grads" % what


# ---- B. whole steps, six in a row -------------------------------------------------------------------------------------------
N_STEPS = 6
# form -> (precision, switches, schedule, batch rows)
WHOLE = {
    "chain": ("bf16", {}, _square(192, 4), 40),
    "layers": ("bf16", {"CODAE_NO_CHAIN": "1"}, _square(192, 4), 40),
    "ragged": ("bf16", {}, RAGGED, 100),
    "f32": ("f32", {}, None, 40),                   # 48 -> 48 -> 40 -> 32 -> 24 -> 16 and back: the stock fixtures' taper
    "graph": ("bf16", {}, _square(192, 4), 40),
    "graph-t500": ("bf16", {}, _square(192, 4), 40),
    "split": ("bf16", {}, _square(192, 4), 40),
    "sharded": ("bf16", {}, _square(192, 4), 40),
}


class Problem:
    pass


@functools.lru_cache(maxsize=None)
def problem(form):
    from oracle import dae_oracle as O
    p = Problem()
    p.prec, p.env, sched, p.B = WHOLE[form]
    p.sched = O.layer_schedule(48, 16, 4, 4, False, "embedding") if sched is None else sched
    io = p.sched[0][0]
    assert io % 3 == 0 and p.sched[-1][1] == io
    rng = np.random.default_rng(7300 + len(p.sched) + io)
    p.params = O.init_params(p.sched, rng)
    p.n = 3 * p.B
    # (values in [0, 8): the gradient norm of the first steps is far above 1, so clip = 1.0 clips - asserted by the test)
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


def spans_of(eng):
    """Three spans that tile [0, n_param) at multiples of 4, cut inside tensors (not at their 64-element boundaries)."""
    n = eng.n_param
    a, b = n // 3 // 4 * 4 + 4, 2 * n // 3 // 4 * 4 + 8
    assert 0 < a < b < n and a % 64 and b % 64 and a % 4 == 0 and b % 4 == 0 and n % 4 == 0
    return [(0, a), (a, b), (b, n)]


def sharded_update(eng, hp, what):
    """The sequence codae.train's sharded data-parallel mode issues with one rank; a span's call must leave everything outside
    the span as it was."""
    acc = eng.new_accumulator()
    spans = spans_of(eng)
    for lo, hi in spans:
        eng.span_sumsq(lo, hi, acc)
    eng.record_grad_sq(acc)
    state = (eng._params, eng.adam_m, eng.adam_v, eng.shadow)
    for lo, hi in spans:
        torch.cuda.synchronize()
        snap = [bits(t) for t in state]
        eng.step_update_span(hp, lo, hi, acc)
        torch.cuda.synchronize()
        for name, t, s in zip(("params", "adam_m", "adam_v", "shadow"), state, snap):
            now = bits(t)
            assert np.array_equal(now[:lo], s[:lo]) and np.array_equal(now[hi:], s[hi:]), \
                "%s: the update of span [%d, %d) changed %s outside it" % (what, lo, hi, name)
            assert not np.array_equal(now[lo:hi], s[lo:hi]), (what, lo, hi, name)
    eng.after_replica_sync()
    eng.step_count += 1
    return float(acc)


@pytest.mark.parametrize("clip", [1.0, 0.0], ids=["clip1", "clip0"])
@pytest.mark.parametrize("form", list(WHOLE))
def test_whole_steps_update_as_float64_adam_of_their_own_gradients(form, clip, monkeypatch):
    from codae.hip.engine import DaeEngine
    H = HYPERS["a"]
    p = problem(form)
    set_env(monkeypatch, p.env)
    trainer = None
    if form.startswith("graph"):
        from codae.train import HipEmbeddingTrainer
        trainer = HipEmbeddingTrainer(p.sched, p.data, p.table, None, H["lr"], H["wd"], clip=clip, max_batch=p.B, precision=p.prec,
                                      device=DEV, use_graph=True)
        eng = trainer.engine
    else:
        eng = DaeEngine(p.sched, p.B, p.prec, DEV)
    eng.load_params(p.params)
    if form == "graph-t500":
        eng.step_count = 500            # (as a caller that goes on from a checkpoint: the bias corrections are rebuilt on the device)
    want_path = "chain" if form in ("chain", "graph", "graph-t500") else "layers"
    if form in ("chain", "layers", "ragged", "f32", "graph", "graph-t500"):
        assert eng.step_path(p.B) == want_path, (form, eng.step_path(p.B))
    worst, clipped = np.zeros(3), 0
    for i, (rows, mid) in enumerate(p.draws):
        torch.cuda.synchronize()
        state = tuple(t.cpu().numpy().copy() for t in (eng.params, eng.adam_m, eng.adam_v))
        t = eng.step_count + 1
        hp = eng.hyper(H["lr"], H["wd"], clip=clip, global_rows=p.B, step=t)
        what = "%s clip %g step %d" % (form, clip, i)
        grad_sq = None
        if trainer is not None:
            assert trainer.train_batch(rows, mask_id=mid) == p.B
        else:
            batch = eng.make_batch(p.data, rows, mid, p.table)
            if form == "split":
                eng.step_forward_loss(batch, hp)
                eng.step_backward(p.B, 0, eng.L)
                eng.step_update(hp)
            elif form == "sharded":
                eng.step_forward_loss(batch, hp)
                eng.step_backward(p.B, 0, eng.L)
                grad_sq = sharded_update(eng, hp, what)
            else:
                eng.train_step(batch, hp)
        torch.cuda.synchronize()
        assert eng.step_count == t
        G = eng.grads.cpu().numpy().copy()
        assert np.isfinite(G).all() and (G != 0).mean() > 0.25, what
        if grad_sq is not None and clip > 0:
            assert eng.read_scalars()[2] == grad_sq, what            # (record_grad_sq: where a fused step leaves it)
        coef, r = check_update(eng, (state[0], G, state[1], state[2]), hp, what, grad_sq=grad_sq if clip > 0 else None)
        worst = np.maximum(worst, r)
        clipped += int(coef < 1)
    assert clipped == (N_STEPS if clip > 0 else 0), "%s clip %g: %d of %d steps were clipped" % (form, clip, clipped, N_STEPS)
    print("MEASURE optimizer %s clip %g: worst over %d steps  p %.3f  m %.3f  v %.3f" % ((form, clip, N_STEPS) + tuple(worst)))


# ---- C. the stand-alone entry point -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", (1, 1000))
@pytest.mark.parametrize("hy", ("a", "b"))
@pytest.mark.parametrize("n", (1, 5, 64, 1000, 4099))
def test_clip_adam_entry_point_on_planted_state(hip, n, hy, t):
    """codae_clip_adam: the flat kernel with no shadow; n % 4 != 0 runs the scalar tail behind the float4 loop.  The buffers
    carry 16 guard elements behind n that must come back untouched."""
    H = HYPERS[hy]
    s = AR.planted_state([(n,)], 500 + n, t == 1, H["wd"])[0]
    guard = np.float32(123.25)
    for branch in CLIPS:
        dev = {k: torch.full((n + 16,), float(guard), dtype=torch.float32, device=DEV) for k in "pgmv"}
        for k in "pgmv":
            dev[k][:n].copy_(torch.from_numpy(s[k]))
        sc = torch.zeros(hip.S_COUNT, dtype=torch.float64, device=DEV)
        clip = clip_values(s["g"])[branch]
        hp = hip.Hyper(H["lr"], H["wd"], H["betas"][0], H["betas"][1], H["eps"], clip, t, 0.0)
        hip.check(hip.lib().codae_clip_adam(hip.ptr(dev["p"]), hip.ptr(dev["g"]), hip.ptr(dev["m"]), hip.ptr(dev["v"]), n, C.byref(hp),
                                            hip.ptr(sc), hip.current_stream()))
        torch.cuda.synchronize()
        scal = sc.cpu()
        gsq = float(scal[hip.S_GRAD_SQ]) + float(scal[hip.S_GRAD_SQ_SLOTS:hip.S_GRAD_SQ_SLOTS + hip.S_N_SLOTS].sum())
        out = {k: dev[k].cpu().numpy() for k in "pgmv"}
        what = "clip_adam n %d %s clip %s" % (n, hy, branch)
        check_update(None, (s["p"], s["g"], s["m"], s["v"]), hp, what, grad_sq=gsq, got=(out["p"][:n], out["m"][:n], out["v"][:n]),
                     branch=branch)
        for k in "pgmv":
            assert (out[k][n:] == guard).all(), "%s: wrote behind n in %s" % (what, k)
        assert np.array_equal(bits(out["g"][:n]), bits(s["g"])), what
