"""A step must not depend on what earlier calls left in the engine's buffers.

Almost every other GPU test builds an engine with max_batch = B on workspaces torch.zeros just handed out and runs one batch.
Real use runs full batches, the ragged last batch of the epoch, an evaluation pass, full batches again, and now and then reloads
good parameters after a step diverged.  The kernels lean on padding (bf16 rows padded to 64, 16-row panels in the chain kernel,
weight gradients that reduce over rows_for(B) rows and need the pad rows of one operand to be exactly zero), and every such
guarantee holds trivially on zero-initialised memory.  The engine has no float atomics, so nothing here needs a tolerance: the
same state and the same batch must give the same BITS whatever ran before.

Part A  (test_probe_does_not_depend_on_history, test_graph_steps_equal_eager_steps)
    H ran a dirtying sequence at max_batch and was then restored to a known state S (the whole flat parameter and Adam vectors
    copied, step_count set, sync_shadows(), zero_metric_sums() - what a caller does when it reloads a checkpoint); F is a newly
    built engine restored to S the same way.  Both run the same probe call; everything it leaves behind is compared with
    torch.equal and must be finite.  The guard `H.acts != F.acts` shows that H really held stale rows the probe did not touch.
    Graph form: the graph entry over a big, a small and a big batch again (capture, two re-captures) against the same three eager
    steps - the header's "Same results as codae_train_step", to the bit.  The one scalar that differs by contract is
    CODAE_S_ADAM_STEP, an INPUT of the graph entry ("written before each codae_train_step_graph launch") that the eager
    entry never touches: it is checked against the step index on the graph side, against zero on the eager side, and every
    other scalar is compared.

Part B  (test_first_use_needs_only_the_documented_zero_bytes)
    include/codae_hip.h, "Buffer contents", lists the borrowed bytes that must be zero before the first call; everything else
    may hold anything.  POISON below is that paragraph in executable form: every byte NOT on the list is filled with 0xFF (NaN as
    bf16 and as fp32, all ones as mask bits) before the parameters are loaded, and a ragged training step plus an evaluation step
    must come out bit-equal to an engine left as allocated.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
LR, WD, CLIP = 1e-3, 1e-4, 1.0


def _square(io, n_layers):
    return [(io, io, l + 1 < n_layers) for l in range(n_layers)]


def _tapered(io, z):
    from oracle import dae_oracle as O
    return O.layer_schedule(io, z, 2, 2, False, "embedding")


NO_CHAIN = {"CODAE_NO_CHAIN": "1"}
# The smallest shapes that reach each code path.  path: what step_path() must report for every batch size used; counts: launches
# per class of one training probe (the engine's launch profiler, as tests/test_gpu_launch_plan.py), so that a case cannot
# silently run on another path; `slabs`: split-K slabs + reduce from this many padded rows on.
STACKS = {
    # persistent chain kernel + one grouped weight-gradient launch
    # widths 192 -> 128 -> 64 -> 128 -> 192 (the reference's 2 + 2 layer stack: six Linears)
    "chain": dict(prec="bf16", sched=lambda: _tapered(192, 64), max_batch=320, probes=(1, 200, 257, 320), path="chain",
                  forms=("train", "eval"), counts={"chain": 1, "gemm_fwd": 0, "gemm_wgrad": 1}),
    # per-layer launches: fused loss, split-K slabs (5 K-tiles at max_batch), weight gradients on the side stream
    "layers": dict(prec="bf16", sched=lambda: _tapered(192, 64), max_batch=320, probes=(1, 200, 257, 320), env=NO_CHAIN,
                   path="layers", forms=("train", "eval", "dropin"), counts={"chain": 0, "loss": 1}, slabs=128),
    # widths 72 -> 56 -> 40 -> 56 -> 72: padded row strides, zero pad columns in every activation buffer
    "padded": dict(prec="bf16", sched=lambda: _tapered(72, 40), max_batch=320, probes=(1, 200, 257, 320), path="layers",
                   forms=("train", "eval", "dropin"), counts={"chain": 0, "loss": 1}),
    # every forward-form launch on the pipelined 256 x 192 tile: fused loss epilogue and 1-bit ReLU masks of gemm_bf16_pipe.hip
    "pipe": dict(prec="bf16", sched=lambda: _square(384, 3), max_batch=520, probes=(300, 513),
                 env=dict(NO_CHAIN, CODAE_GEMM_TILE="x"), path="layers", forms=("train",),
                 counts={"chain": 0, "loss": 1, "gemm_fwd": 2}, slabs=128),
    # 5 x 48 = 240 tiles of 256 x 192: the data-gradient chain, then every weight gradient in one pipelined grouped launch
    "wide": dict(prec="bf16", sched=lambda: _square(1536, 5), max_batch=1280, probes=(1100, 1030), path="layers", forms=("train",),
                 counts={"chain": 0, "loss": 1, "gemm_dgrad": 4, "gemm_wgrad": 5, "slab_reduce": 0}),
    # generic-activation instantiations of the forward and data-gradient GEMMs
    "elu": dict(prec="bf16", sched=lambda: _tapered(192, 64), max_batch=320, probes=(1, 200, 257, 320), path="layers",
                forms=("train",), activation="elu", counts={"chain": 0, "loss": 1}),
    # the gather-noise launcher in front of the per-layer launches; the state's step index feeds the noise counter
    "noise": dict(prec="bf16", sched=lambda: _tapered(192, 64), max_batch=320, probes=(1, 200, 257, 320), env=NO_CHAIN,
                  path="layers", forms=("train",), noise=True, counts={"chain": 0, "gather": 1, "loss": 1}),
    # widths 33 -> 25 -> 17 -> 25 -> 33: the fp32 MFMA kernel, ragged in every dimension
    "f32-native": dict(prec="f32", sched=lambda: _tapered(33, 17), max_batch=100, probes=(1, 37), path="layers",
                       forms=("train", "eval", "dropin"), counts={"chain": 0, "gemm_fwd": 6, "slab_reduce": 0}),
    # widths 768 -> 512 -> 256 -> 512 -> 768: the bf16-plane fp32 GEMMs
    "f32-x3": dict(prec="f32", sched=lambda: _tapered(768, 256), max_batch=500, probes=(333,), path="layers", forms=("train",),
                   counts={"chain": 0, "gemm_fwd": 6}),
}
DIRTY = ("big-train", "big-eval-then-train", "diverged")


@pytest.fixture
def env_toggle():
    """Sets CODAE_* variables (before the engine is created: codae_create snapshots them); restores them afterwards."""
    from codae import hip
    saved = {}

    def set_(name, value):
        saved.setdefault(name, os.environ.get(name))
        os.environ[name] = value
        hip.lib().codae_reload_env()
    yield set_
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    hip.lib().codae_reload_env()


@pytest.fixture(scope="module", autouse=True)
def _release_device_memory():
    yield
    problem.cache_clear()
    _STATE.clear()
    torch.cuda.empty_cache()


class Problem:
    pass


@functools.lru_cache(maxsize=None)
def problem(stack):
    """Schedule, initial parameters, a resident dataset of max_batch + 64 rows (and its copy with one NaN and one +Inf row),
    the slot-mask table and fixed row / mask-id draws, built once per stack."""
    from oracle import dae_oracle as O
    c = STACKS[stack]
    p = Problem()
    p.sched = c["sched"]()
    io = p.sched[0][0]
    assert io % 3 == 0 and p.sched[-1][1] == io
    p.io, p.max_batch = io, c["max_batch"]
    rng = np.random.default_rng(sorted(STACKS).index(stack) + 4100)
    p.params = O.init_params(p.sched, rng)
    n = p.max_batch + 64
    p.n = n
    p.data = torch.tensor(rng.random((n, io), dtype=np.float32), device=DEV)
    bm, _, _ = O.corrupter_tables([{"size": io // 3, "position": s * (io // 3)} for s in range(3)], 1)
    p.table = torch.tensor(bm).to(torch.uint8).to(DEV)

    def draw(B):
        return (torch.tensor(rng.permutation(n)[:B], dtype=torch.int32, device=DEV),
                torch.tensor(rng.integers(0, 3, B), dtype=torch.int32, device=DEV))
    p.big = [draw(p.max_batch) for _ in range(3)]              # the state step / the dirtying steps
    p.probe = {B: draw(B) for B in c["probes"]}
    p.dy = {B: torch.tensor(rng.standard_normal((B, io)).astype(np.float32), device=DEV) for B in c["probes"]}
    # the diverged step gathers these two rows: one element NaN, one +Inf
    p.data_bad = p.data.clone()
    rows = p.big[1][0]
    p.data_bad[int(rows[3]), 5] = float("nan")
    p.data_bad[int(rows[p.max_batch // 2]), io - 2] = float("inf")
    return p


def make_engine(stack):
    from codae.hip.engine import DaeEngine
    c, p = STACKS[stack], problem(stack)
    for k, v in c.get("env", {}).items():
        assert os.environ.get(k) == v, "%s: the switch %s is not set" % (stack, k)
    eng = DaeEngine(p.sched, p.max_batch, c["prec"], DEV, activation=torch.nn.ELU if c.get("activation") == "elu" else None)
    if c.get("noise"):
        from codae.tool import InputNoise
        eng.set_input_noise(InputNoise("gaussian", sigma=0.1))
    for B in c["probes"] + (p.max_batch,):
        assert eng.step_path(B) == c["path"], (stack, B, eng.step_path(B))
    return eng


def rows_for(eng, B):
    from codae.hip import PREC_BF16
    return (B + 63) // 64 * 64 if eng.precision == PREC_BF16 else B


def train(eng, p, draw, data=None):
    rows, mid = draw
    batch = eng.make_batch(p.data if data is None else data, rows, mid, p.table)
    eng.train_step(batch, eng.hyper(LR, WD, clip=CLIP, global_rows=batch.B))


_STATE = {}


def state(stack):
    """S: parameters and Adam moments after one ordinary step from the initial parameters (step index 2 comes next), taken once
    per stack from an engine of its own."""
    if stack not in _STATE:
        p = problem(stack)
        eng = make_engine(stack)
        eng.load_params(p.params)
        train(eng, p, p.big[0])
        torch.cuda.synchronize()
        _STATE[stack] = (eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone(), eng.step_count)
        assert eng.step_count == 1 and float(eng.adam_v.abs().max()) > 0
    return _STATE[stack]


def restore(eng, S):
    """What a caller does to go on from a checkpoint with the engine it has - nothing more."""
    eng.join()
    eng._params.copy_(S[0])
    eng.adam_m.copy_(S[1])
    eng.adam_v.copy_(S[2])
    eng.step_count = S[3]
    eng.sync_shadows()
    eng.zero_metric_sums()


def dirty(eng, p, how):
    if how == "big-train":
        train(eng, p, p.big[1])
        train(eng, p, p.big[2])
    elif how == "big-eval-then-train":
        rows, mid = p.big[2]
        eng.eval_step(eng.make_batch(p.data, rows, mid, p.table))
        train(eng, p, p.big[1])
    else:
        assert how == "diverged"
        train(eng, p, p.big[1], data=p.data_bad)
        torch.cuda.synchronize()
        for l in range(eng.L):          # (a NaN norm gives a NaN clip coefficient: every parameter is NaN - codae_hip.h, point 3)
            assert bool(torch.isnan(eng.weight(l)).all()) and bool(torch.isnan(eng.bias(l)).all()), l
        assert not np.isfinite(eng.read_scalars()[3])


def snapshot(eng, extra=(), grads=True, scalars=True):
    out = {"params": eng.params, "adam_m": eng.adam_m, "adam_v": eng.adam_v}
    if grads:
        out["grads"] = eng.grads
    if scalars:
        out["scalars"] = eng.scalars
    if eng.shadow is not None:
        out["shadow"], out["shadow_t"] = eng.shadow, eng.shadow_t
    out.update(extra)
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in out.items()}


def launch_counts(eng, call):
    """{class: launches} of call() on eng (codae_profile_begin / _end)."""
    from codae import hip
    from codae.hip import KERNEL_CLASSES
    lib, cap = hip.lib(), 256
    hip.check(lib.codae_profile_stride(eng._h, 1))
    hip.check(lib.codae_profile_begin(eng._h, (1 << len(KERNEL_CLASSES)) - 1, cap))
    call()
    kinds, ms, n = (C.c_int32 * cap)(), (C.c_float * cap)(), C.c_int32()
    hip.check(lib.codae_profile_end(eng._h, kinds, ms, cap, C.byref(n)))
    assert 0 < n.value < cap
    names = [KERNEL_CLASSES[kinds[i]] for i in range(n.value)]
    return {k: names.count(k) for k in KERNEL_CLASSES}


def probe(eng, p, form, B):
    """The probe call; {name: tensor} of everything it leaves behind."""
    rows, mid = p.probe[B]
    if form == "train":
        train(eng, p, p.probe[B])
        return snapshot(eng)
    if form == "eval":
        out_y = torch.empty((B, p.io), dtype=torch.float32, device=DEV)
        eng.eval_step(eng.make_batch(p.data, rows, mid, p.table), out_y)
        return snapshot(eng, {"out_y": out_y}, grads=False)      # (an evaluation step leaves the gradients of whatever ran before)
    assert form == "dropin"
    x = p.data[rows.long()].contiguous()
    y = eng.forward(x)
    dx = eng.backward(p.dy[B], need_dx=True)
    return snapshot(eng, {"y": y, "dx": dx}, scalars=False)      # (codae_forward / codae_backward do not touch the scalar block)


def assert_same_bits(got, want, what):
    assert sorted(got) == sorted(want)
    for name in want:
        assert bool(torch.isfinite(want[name]).all()), "%s: %s of the fresh engine is not finite" % (what, name)
        assert bool(torch.isfinite(got[name]).all()), "%s: %s is not finite" % (what, name)
        if not torch.equal(got[name], want[name]):
            d = (got[name].double() - want[name].double()).abs()
            raise AssertionError("%s: %s differs from the fresh engine's in %d of %d elements (largest difference %.3g, first at %d)" % (
                what, name, int((d != 0).sum()), d.numel(), float(d.max()), int((d != 0).nonzero()[0])))


CASES_A = [(s, how, form, B) for s in STACKS for how in DIRTY for form in STACKS[s]["forms"] for B in STACKS[s]["probes"]]


@pytest.mark.parametrize("stack,how,form,B", CASES_A, ids=["%s-%s-%s-B%d" % c for c in CASES_A])
def test_probe_does_not_depend_on_history(stack, how, form, B, env_toggle):
    c = STACKS[stack]
    for k, v in c.get("env", {}).items():
        env_toggle(k, v)
    p, S = problem(stack), state(stack)
    H = make_engine(stack)
    H.load_params(p.params)
    dirty(H, p, how)
    restore(H, S)
    got = probe(H, p, form, B)
    F = make_engine(stack)
    restore(F, S)
    if form == "train":
        counts = launch_counts(F, lambda: train(F, p, p.probe[B]))
        want = snapshot(F)
        for cls, n in c["counts"].items():
            assert counts[cls] == n, (stack, B, cls, counts)
        if "slabs" in c:
            assert (counts["slab_reduce"] > 0) == (rows_for(F, B) >= c["slabs"]), (stack, B, counts)
        assert H.step_count == F.step_count == S[3] + 1
        assert not torch.equal(want["params"], S[0])
    else:
        want = probe(F, p, form, B)
    what = "%s after %s, %s at B = %d" % (stack, how, form, B)
    assert_same_bits(got, want, what)
    assert form == "eval" or float(want["grads"].abs().max()) > 0, what
    # not an empty comparison: H still holds rows of the big batches that the probe did not touch
    if rows_for(H, B) < (p.max_batch + 63) // 64 * 64:
        assert not torch.equal(H.acts, F.acts), what


CASES_G = [(s, B) for s in ("chain", "layers") for B in STACKS[s]["probes"]]


@pytest.mark.parametrize("stack,B", CASES_G, ids=["%s-B%d" % c for c in CASES_G])
def test_graph_steps_equal_eager_steps(stack, B, env_toggle):
    """codae_train_step_graph on a created stream with persistent index buffers (as HipEmbeddingTrainer drives it): max_batch rows
    (capture), B rows (re-capture), max_batch rows (second re-capture), against the same three steps of codae_train_step."""
    from codae.hip import S_ADAM_STEP
    c = STACKS[stack]
    for k, v in c.get("env", {}).items():
        env_toggle(k, v)
    p, S = problem(stack), state(stack)
    steps = [p.big[1], p.probe[B], p.big[2]]
    H, F = make_engine(stack), make_engine(stack)
    restore(H, S)
    restore(F, S)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    idx_buf = torch.zeros(p.max_batch, dtype=torch.int32, device=DEV)
    mid_buf = torch.zeros(p.max_batch, dtype=torch.int32, device=DEV)
    for i, (rows, mid) in enumerate(steps):
        n = int(rows.numel())
        with torch.cuda.stream(stream):
            idx_buf[:n].copy_(rows)
            mid_buf[:n].copy_(mid)
            batch = H.make_batch(p.data, idx_buf[:n], mid_buf[:n], p.table)
            H.train_step(batch, H.hyper(LR, WD, clip=CLIP, global_rows=n), graph=True)
        stream.synchronize()
        train(F, p, (rows, mid))
        got, want = snapshot(H), snapshot(F)
        # the graph entry's input slot (see the module docstring); every other scalar is compared
        assert float(got["scalars"][S_ADAM_STEP]) == S[3] + i + 1 and float(want["scalars"][S_ADAM_STEP]) == 0.0
        got["scalars"][S_ADAM_STEP] = 0.0
        assert_same_bits(got, want, "%s, graph step %d (%d rows)" % (stack, i, n))
        assert float(want["scalars"][3]) > 0
    assert H.step_count == F.step_count == S[3] + 3


# ---- Part B -----------------------------------------------------------------------------------------------------------------
# include/codae_hip.h, codae_buffers, "Buffer contents":
#   "Before the first call these borrowed bytes must be ZERO: (1) params, grads, adam_m and adam_v outside the weight and bias
#    tensors (the padding that rounds every tensor up to 64 floats) ... (2) all of scalars ... (3) only when a layer width is not a
#    multiple of 64: all of acts and dacts (the pad columns ...) and the 64 * maxw elements of shadow_w and shadow_wt behind
#    n_param ...  Everything else may hold anything: ... slabs, bias_parts, the weight and bias tensors inside grads, and - when
#    every width is a multiple of 64 - acts, dacts and the slack behind n_param in both shadows."
# region -> poisoned on stacks whose widths are all multiples of 64 / on the padded stack
POISON = {"acts": (True, False), "dacts": (True, False), "shadow_slack": (True, False),
          "slabs": (True, True), "bias_parts": (True, True), "grad_tensors": (True, True)}
FIRST_USE = {"chain": 200, "layers": 200, "pipe": 300, "wide": 1100, "f32-x3": 333, "padded": 200}


def poison(eng, padded):
    def ff(t):
        t.view(torch.uint8).fill_(0xFF)
    hit = 0
    for region, (on_even, on_padded) in POISON.items():
        if not (on_padded if padded else on_even):
            continue
        if region == "shadow_slack":
            ts = [] if eng.shadow is None else [eng.shadow[eng.n_param:], eng.shadow_t[eng.n_param:]]
        elif region == "grad_tensors":
            ts = [eng.weight_grad(l) for l in range(eng.L)] + [eng.bias_grad(l) for l in range(eng.L)]
        else:
            ts = [getattr(eng, region)]
        for t in ts:
            if t is not None:
                assert t.numel() > 0
                ff(t)
                hit += 1
    return hit


@pytest.mark.parametrize("stack", sorted(FIRST_USE))
def test_first_use_needs_only_the_documented_zero_bytes(stack, env_toggle):
    c = STACKS[stack]
    for k, v in c.get("env", {}).items():
        env_toggle(k, v)
    p, B = problem(stack), FIRST_USE[stack]
    padded = any(k % 64 or n % 64 for k, n, _ in p.sched)
    assert padded == (stack == "padded") and B % 64 != 0 and B in c["probes"]
    def results(eng, extra=()):
        # (the slack behind n_param is no result: it holds the poison, or the zeros of the allocation, as it was handed over)
        out = snapshot(eng, extra)
        for name in ("shadow", "shadow_t"):
            if name in out:
                out[name] = out[name][:eng.n_param]
        return out

    runs = []
    for poisoned in (True, False):
        eng = make_engine(stack)
        if poisoned:
            assert poison(eng, padded) >= 2 * eng.L + 1
            assert bool(torch.isnan(eng.bias_grad(0)).all()) and bool(torch.isnan(eng.bias_parts).all())
        eng.load_params(p.params)
        train(eng, p, p.probe[B])
        after_train = results(eng)
        out_y = torch.empty((B, p.io), dtype=torch.float32, device=DEV)
        rows, mid = p.big[2]
        eng.eval_step(eng.make_batch(p.data, rows[:B].contiguous(), mid[:B].contiguous(), p.table), out_y)
        runs.append((after_train, results(eng, {"out_y": out_y})))
    (pt, pe), (ct, ce) = runs
    assert_same_bits(pt, ct, "%s, first training step on poisoned workspaces" % stack)
    assert_same_bits(pe, ce, "%s, evaluation step on poisoned workspaces" % stack)
    assert float(ct["grads"].abs().max()) > 0 and float(ce["scalars"][0]) > 0
