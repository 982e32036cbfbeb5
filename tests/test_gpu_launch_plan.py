"""Which launches a step makes, in host issue order, on a real MI355X.

The numeric suites would still pass if a branch of the step or backward scheduling quietly fell back to another one (a
grouped weight gradient to per-layer launches, the fused loss to the stand-alone kernel, two streams to one).  The engine's
launch profiler records the class of every profiled launch in the order the host issued it; this file pins that list, for
one shape per scheduling branch, to tests/golden/launch_plan.json.  The fixture was recorded once with record_case() below
on the commit it names and is compared verbatim: a change that leaves the schedule alone passes against it unchanged.

Each shape is the smallest that takes its branch by the conditions in step_plan / grouped_wgrad_strategy, choose_split_k*,
chain_supported and gemm_f32_small (csrc/engine.hip); `counts` restates what the branch means in launches, independently of the
fixture, so that a shape that missed its branch on the recording commit could not have been recorded as if it had taken it.
No numerics are checked here.

The same run also closes the loop with tests/test_step_plan_host.py: the plan the live engine answers for the calls the case made
(codae_debug_step_plan, with the engine's real buffers) must say what the record shows was launched.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
LR, WD, CLIP = 1e-3, 1e-4, 1.0
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_plan.json")

NO_CHAIN = {"CODAE_NO_CHAIN": "1"}
# id: precision, width and depth of the square stack, batch, CODAE_* switches, what is run, step_path, launch counts
CASES = {
    # persistent chain: chain kernel, one grouped weight gradient, bias finish carrying the loss finish, Adam
    "01-bf16-chain": dict(prec="bf16", io=192, L=3, B=96, path="chain",
                          counts={"chain": 1, "gemm_wgrad": 1, "bias_finish": 1, "adam": 1, "gemm_fwd": 0, "loss": 0}),
    # per-layer launches, fused loss, deferral mode 0 (27 small tiles < 128), two streams, unsplit weight gradients
    "02-bf16-layers": dict(prec="bf16", io=192, L=3, B=96, env=NO_CHAIN, path="layers",
                           counts={"gemm_fwd": 2, "loss": 1, "gemm_dgrad": 2, "gemm_wgrad": 3, "slab_reduce": 0, "chain": 0}),
    "03-bf16-single-stream": dict(prec="bf16", io=192, L=3, B=96, env=dict(NO_CHAIN, CODAE_SINGLE_STREAM="1"), path="layers",
                                  counts={"gemm_fwd": 2, "loss": 1, "gemm_dgrad": 2, "gemm_wgrad": 3, "slab_reduce": 0}),
    # stand-alone loss launch: all three layers are plain forward GEMMs
    "04-bf16-unfused-loss": dict(prec="bf16", io=192, L=3, B=96, env=dict(NO_CHAIN, CODAE_NO_FUSED_LOSS="1"), path="layers",
                                 counts={"gemm_fwd": 3, "loss": 1, "gemm_wgrad": 3}),
    # 512 rows = 8 K-tiles, split 8: every weight gradient is followed by a slab reduce
    "05-bf16-split-k": dict(prec="bf16", io=192, L=3, B=512, env=NO_CHAIN, path="layers",
                            counts={"gemm_wgrad": 3, "slab_reduce": 3}),
    # width > 512: no chain; 243 small tiles >= 128, 27 big tiles < 200: mode 2, one grouped launch after the data gradients
    "06-bf16-grouped": dict(prec="bf16", io=576, L=3, B=128, path="layers",
                            counts={"gemm_wgrad": 1, "gemm_dgrad": 2, "slab_reduce": 0, "chain": 0}),
    # 240 big tiles >= 200: mode 1, one pipelined grouped launch reported as 5 weight-gradient records
    "07-bf16-deferred": dict(prec="bf16", io=1536, L=5, B=64, path="layers",
                             counts={"gemm_wgrad": 5, "gemm_dgrad": 4, "slab_reduce": 0}),
    # 17 layers on 16 rotating gradient buffers: per-layer weight gradients, no chain
    "08-bf16-rotating": dict(prec="bf16", io=64, L=17, B=64, path="layers",
                             counts={"gemm_wgrad": 17, "gemm_dgrad": 16, "chain": 0}),
    # a generic activation takes the per-layer launches
    "09-bf16-leaky": dict(prec="bf16", io=192, L=3, B=96, act="leaky", path="layers", counts={"chain": 0, "gemm_wgrad": 3}),
    # so does input noise
    "10-bf16-noise": dict(prec="bf16", io=192, L=3, B=96, noise=True, path="layers", counts={"chain": 0, "gather": 1}),
    # the backward bucket by bucket without joins (what a data-parallel step issues), no communicator needed
    "11-bf16-bucketed": dict(prec="bf16", io=192, L=3, B=96, env=NO_CHAIN, run="bucketed", path="layers",
                             counts={"gemm_wgrad": 3, "gemm_dgrad": 2, "bias_finish": 1, "adam": 1}),
    # eval_step; forward; backward without and with an input gradient
    "12-bf16-dropin": dict(prec="bf16", io=192, L=3, B=96, run="dropin", path="chain",
                           counts={"gemm_fwd": 6, "gemm_wgrad": 6, "gemm_dgrad": 5, "adam": 0}),
    # forward and data gradient through gemm_f32_small, mode 0
    "13-f32-small": dict(prec="f32", io=384, L=3, B=128, path="layers",
                         counts={"gemm_fwd": 3, "gemm_dgrad": 2, "gemm_wgrad": 3, "slab_reduce": 0}),
    # 1280 rows: weight gradients split 5, with slab reduces
    "14-f32-split-k": dict(prec="f32", io=384, L=3, B=1280, path="layers", counts={"gemm_wgrad": 3, "slab_reduce": 3}),
    # 288 tiles >= 256: mode 3, gemm_f32x3_grouped reported as 2 weight-gradient records
    "15-f32-grouped": dict(prec="f32", io=1536, L=2, B=256, path="layers", counts={"gemm_wgrad": 2, "slab_reduce": 0}),
}


@pytest.fixture
def env_toggle():
    """Sets CODAE_* variables (before the engine is created: codae_create snapshots them); restores them afterwards."""
    from codae import hip
    saved = {}

    def set_(name, value):
        saved.setdefault(name, os.environ.get(name))
        os.environ[name] = value
    yield set_
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    hip.lib().codae_reload_env()


PLAN_FIELDS = ["rows", "path", "loss", "loss_finish", "wgrad", "streams", "tail_on_caller", "bias_finish", "norm", "update"]
TRAIN, FORWARD_LOSS, EVAL, BACKWARD, DROPIN_BACKWARD, UPDATE = range(6)           # call kinds of codae_debug_step_plan
LOSS_FUSED, LOSS_IN_CHAIN = 2, 3


def calls_of(case):
    """The calls CASES[case] makes, as codae_debug_step_plan takes them: kind, B, lo, hi, join, dx wanted, out_y given, clipping."""
    c = CASES[case]
    B, L, run = c["B"], c["L"], c.get("run", "train")
    if run == "train":
        return [(TRAIN, B, 0, L, 1, 0, 0, 1)]
    if run == "bucketed":
        return [(FORWARD_LOSS, B, 0, L, 1, 0, 0, 0)] + [(BACKWARD, B, l, l + 1, 0, 0, 0, 0) for l in range(L - 1, -1, -1)] + [(UPDATE, 0, 0, 0, 1, 0, 0, 1)]
    return [(EVAL, B, 0, L, 1, 0, 0, 0), (DROPIN_BACKWARD, B, 0, L, 1, 0, 0, 0), (DROPIN_BACKWARD, B, 0, L, 1, 1, 0, 0)]


def record_case(case, setenv):
    """(step_path, class names of the second step's launches in issue order, the plans of the calls made) of CASES[case]."""
    import bench
    from codae import hip
    from codae.hip import ACT_LEAKY, KERNEL_CLASSES
    from codae.tool import InputNoise
    from codae.train import HipEmbeddingTrainer
    from oracle import dae_oracle as O
    c = CASES[case]
    io, L, B = c["io"], c["L"], c["B"]
    for k, v in c.get("env", {}).items():
        setenv(k, v)
    rng = np.random.default_rng(20260 + int(case[:2]))
    sched = bench.square_schedule(io, (L - 1) // 2, (L - 2) // 2)
    assert len(sched) == L
    S, E = 3, io // 3
    bm, _, _ = O.corrupter_tables([{"size": E, "position": s * E} for s in range(S)], 1)
    data = rng.random((2 * B, io), dtype=np.float32)
    mtu = np.stack([rng.permutation(S) for _ in range(len(data))]).astype(np.int32)
    tr = HipEmbeddingTrainer(sched, torch.tensor(data), torch.tensor(bm).to(torch.uint8), torch.tensor(mtu), LR, WD, CLIP,
                             max_batch=B, precision=c["prec"], device=DEV,
                             activation=(ACT_LEAKY, 0.1, 0.0, 0.0) if c.get("act") == "leaky" else None,
                             input_noise=InputNoise("masking", p=0.25, seed=7) if c.get("noise") else None)
    tr.init_params(seed=1)
    eng, lib = tr.engine, hip.lib()
    idx = torch.tensor(rng.permutation(len(data))[:B], dtype=torch.int32, device=DEV)
    x = torch.tensor(rng.random((B, io), dtype=np.float32), device=DEV)
    dy = torch.tensor(rng.standard_normal((B, io)).astype(np.float32), device=DEV)

    def step():
        run = c.get("run", "train")
        if run == "train":
            tr.train_batch(idx, run=0)
        elif run == "bucketed":
            batch, hyper = tr._batch(idx, 0), eng.hyper(LR, WD, CLIP, global_rows=B)
            eng.step_forward_loss(batch, hyper)
            for l in range(L - 1, -1, -1):
                eng.step_backward(B, l, l + 1, join=False)
            eng.step_update(hyper)
        else:
            eng.eval_step(tr._batch(idx, 0))
            eng.forward(x)
            eng.backward(dy, need_dx=False)
            eng.backward(dy, need_dx=True)

    step()
    cap = 256
    hip.check(lib.codae_profile_stride(eng._h, 1))
    hip.check(lib.codae_profile_begin(eng._h, (1 << len(KERNEL_CLASSES)) - 1, cap))
    step()
    # (DaeEngine.profile_end groups the records by class: read the ordered list from the library)
    kinds, ms, n = (C.c_int32 * cap)(), (C.c_float * cap)(), C.c_int32()
    hip.check(lib.codae_profile_end(eng._h, kinds, ms, cap, C.byref(n)))
    assert 0 < n.value < cap
    path = eng.step_path(B)
    plans = []
    for call in calls_of(case) + [(TRAIN, B, 0, L, 1, 0, 0, 1)]:          # (last: the fused step's, which codae_step_path is about)
        out = (C.c_int32 * len(PLAN_FIELDS))()
        hip.check(lib.codae_debug_step_plan(eng._h, C.byref(eng.bufs), (C.c_int32 * 8)(*call), out, len(PLAN_FIELDS)))
        plans.append(dict(zip(PLAN_FIELDS, list(out)), kind=call[0]))
    torch.cuda.synchronize()
    return path, [KERNEL_CLASSES[kinds[i]] for i in range(n.value)], plans


@pytest.mark.parametrize("case", sorted(CASES))
def test_launch_plan(case, env_toggle):
    with open(FIXTURE) as f:
        want = json.load(f)["cases"][case]
    path, kinds, plans = record_case(case, env_toggle)
    print("MEASURE launch plan %s: %s %s" % (case, path, " ".join(kinds)))
    assert path == CASES[case]["path"], (case, path)
    for cls, n in CASES[case]["counts"].items():
        assert kinds.count(cls) == n, (case, cls, kinds.count(cls), n, kinds)
    assert path == want["step_path"], (case, path, want["step_path"])
    assert kinds == want["kinds"], (case, kinds, want["kinds"])
    # the plan says what was launched, where the record can show it
    L, fused_step, plans = CASES[case]["L"], plans[-1], plans[:-1]
    assert ("chain", "layers")[fused_step["path"] == 0] == path, (case, fused_step, path)
    grouped = {p["wgrad"] != 0 for p in plans if p["kind"] in (TRAIN, BACKWARD, DROPIN_BACKWARD)}
    assert len(grouped) == 1, (case, plans)
    last_dgrad = max(i for i, k in enumerate(["gemm_dgrad"] + kinds) if k == "gemm_dgrad")         # (0: the chain kernel made them all)
    assert grouped.pop() == ("gemm_wgrad" not in kinds[:last_dgrad]), (case, plans, kinds)
    fwd_then_loss = kinds.count("loss") == 1 and kinds[:kinds.index("loss")].count("gemm_fwd") == L - 1
    assert any(p["loss"] == LOSS_FUSED for p in plans) == fwd_then_loss, (case, plans, kinds)
    assert any(p["loss"] == LOSS_IN_CHAIN for p in plans) == (kinds.count("chain") == 1 and "gemm_fwd" not in kinds), (case, plans, kinds)
    assert any(p["update"] != 0 for p in plans) == (kinds.count("adam") == 1), (case, plans, kinds)
