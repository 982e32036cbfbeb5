"""Which launches a call makes, pinned on the host (no GPU).

step_plan (csrc/engine.hip) is the one function that turns an engine, its settings and switches, the buffers and a description of
the call into: chain or per-layer path, the form of the loss and of its finish, the weight-gradient strategy, streams, where the
bias finish goes, who gathers the gradient norm, and the update kernel.  Every entry point asks it once and hands the answer down;
codae_debug_step_plan returns that answer without making a HIP call.  This file creates engines on the CPU, sets settings and
switches, asks, and compares verbatim against tests/golden/step_plan.json.

The fixture was recorded on the commit it names - the last one whose entry points each decided their part for themselves - from a
build of that commit plus a patch that adds only the query: every field computed by calling that commit's own predicates (its
chain-eligibility test and its weight-gradient mode) and by copies of its inline expressions (the fused-loss and folded-finish
tests of the forward, `dual` and the tail test of backward_range, the two "norm from the backward" tests of the fused step, the
tiled-update test).  Regenerate it the same way, never from the code under test:
`python tests/test_step_plan_host.py LIBRARY_OF_THAT_BUILD > tests/golden/step_plan.json`.

`want` restates per case, independently of the fixture, which path / weight-gradient strategy / loss form (and whatever else the
case is about) it is meant to reach, derived by hand from the tile counts as the comments say, so that a shape that missed its
branch on the recording commit could not have been recorded as if it had taken it.

codae_set_slot_contrast is not exercised: turning it on makes a HIP call.
"""
import ctypes as C
import json
import os
import sys

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_plan.json")
FIELDS = ["rows", "path", "loss", "loss_finish", "wgrad", "streams", "tail_on_caller", "bias_finish", "norm", "update"]
SWITCHES = ("CODAE_NO_CHAIN", "CODAE_SINGLE_STREAM", "CODAE_NO_FUSED_LOSS", "CODAE_NO_FOLDED_LOSS_FINISH", "CODAE_NO_FOLDED_BIAS_FINISH",
            "CODAE_NO_DEFER_WGRAD", "CODAE_NO_FUSED_NORM", "CODAE_FLAT_ADAM", "CODAE_TAIL_ON_SIDE", "CODAE_F32_GEMM")
TRAIN, FORWARD_LOSS, EVAL, BACKWARD, DROPIN_BACKWARD, UPDATE = range(6)
LAYERS, CHAIN = 0, 1
NO_LOSS, STANDALONE, FUSED, IN_CHAIN = range(4)
NONE, OWN, CARRIED = range(3)                       # loss_finish; bias_finish: NONE, OWN, FOLDED
FOLDED = 2
PER_LAYER, GROUPED_PIPE, GROUPED_ONE_BARRIER, GROUPED_F32 = range(4)
NO_CLIP, FROM_BACKWARD, FLAT_PASS = range(3)
NO_UPDATE, FLAT, TILED = range(3)

NO_CHAIN = {"CODAE_NO_CHAIN": "1"}
CASES = {}


def case(name, prec, io, L, call, want, env=None, settings=(), max_batch=None):
    """call: (kind, B, layer_lo, layer_hi, join, dx wanted, out_y given, clipping on)"""
    assert name not in CASES, name
    CASES[name] = dict(prec=prec, io=io, L=L, call=list(call), want=want, env=env or {}, settings=list(settings),
                       max_batch=max_batch or call[1] or 64)


def train(B, clip=1): return (TRAIN, B, 0, 0, 1, 0, 0, clip)
def forward_loss(B, out_y=0): return (FORWARD_LOSS, B, 0, 0, 1, 0, out_y, 0)
def evaluate(B, out_y=0): return (EVAL, B, 0, 0, 1, 0, out_y, 0)
def backward(B, lo, hi, join=1): return (BACKWARD, B, lo, hi, join, 0, 0, 0)
def dropin_backward(B, lo, hi, dx): return (DROPIN_BACKWARD, B, lo, hi, 1, dx, 0, 0)
def update(clip=1): return (UPDATE, 0, 0, 0, 1, 0, 0, clip)


# ---- the fifteen shapes of tests/test_gpu_launch_plan.py, with the calls each of them makes
CHAIN_STEP = dict(path=CHAIN, loss=IN_CHAIN, loss_finish=CARRIED, wgrad=GROUPED_ONE_BARRIER, bias_finish=OWN, norm=FROM_BACKWARD, update=TILED)
case("01-bf16-chain", "bf16", 192, 3, train(96), CHAIN_STEP)
# 3 x (3 x 3) tiles of 64 x 64 = 27 < 128: per-layer weight gradients on two streams, layer 0's on the caller's
LAYER_STEP = dict(path=LAYERS, loss=FUSED, loss_finish=CARRIED, wgrad=PER_LAYER, streams=2, tail_on_caller=1, bias_finish=OWN,
                  norm=FROM_BACKWARD, update=TILED)
case("02-bf16-layers", "bf16", 192, 3, train(96), LAYER_STEP, NO_CHAIN)
case("03-bf16-single-stream", "bf16", 192, 3, train(96), dict(LAYER_STEP, streams=1, tail_on_caller=0), dict(NO_CHAIN, CODAE_SINGLE_STREAM="1"))
case("04-bf16-unfused-loss", "bf16", 192, 3, train(96), dict(LAYER_STEP, loss=STANDALONE, loss_finish=OWN), dict(NO_CHAIN, CODAE_NO_FUSED_LOSS="1"))
case("05-bf16-split-k", "bf16", 192, 3, train(512), dict(LAYER_STEP, rows=512), NO_CHAIN)          # (the split is the GEMM's, not the step's)
# 3 x (9 x 9) = 243 small tiles >= 128, 3 x (3 x 3) = 27 big tiles < 200
case("06-bf16-grouped", "bf16", 576, 3, train(128), dict(path=LAYERS, loss=FUSED, wgrad=GROUPED_ONE_BARRIER, tail_on_caller=0, bias_finish=OWN))
# 5 x (6 x 8) = 240 tiles of 256 x 192 >= 200
case("07-bf16-deferred", "bf16", 1536, 5, train(64), dict(path=LAYERS, loss=FUSED, loss_finish=CARRIED, wgrad=GROUPED_PIPE, bias_finish=FOLDED,
                                                        norm=FROM_BACKWARD))
case("08-bf16-rotating", "bf16", 64, 17, train(64), dict(path=LAYERS, wgrad=PER_LAYER, streams=2, tail_on_caller=1))
case("09-bf16-leaky", "bf16", 192, 3, train(96), dict(path=LAYERS, loss=FUSED, wgrad=PER_LAYER), settings=[("act", "leaky")])
case("10-bf16-noise", "bf16", 192, 3, train(96), dict(path=LAYERS, loss=FUSED, wgrad=PER_LAYER), settings=[("noise",)])
case("11-bf16-bucketed-forward", "bf16", 192, 3, forward_loss(96), dict(path=LAYERS, loss=FUSED, loss_finish=OWN, wgrad=0, update=NO_UPDATE), NO_CHAIN)
for l in (2, 1, 0):      # only the last range finishes the biases; no range is joined, none runs layer 0 on the caller's stream
    case("11-bf16-bucketed-backward-%d" % l, "bf16", 192, 3, backward(96, l, l + 1, join=0),
         dict(loss=NO_LOSS, wgrad=PER_LAYER, streams=2, tail_on_caller=0, bias_finish=OWN if l == 0 else NONE, norm=NO_CLIP, update=NO_UPDATE), NO_CHAIN)
case("11-bf16-bucketed-update", "bf16", 192, 3, update(), dict(loss=NO_LOSS, norm=FLAT_PASS, update=TILED), NO_CHAIN)
# the drop-in calls never take the chain, though the fused step of the same engine would
case("12-bf16-dropin-eval", "bf16", 192, 3, evaluate(96), dict(path=LAYERS, loss=STANDALONE, loss_finish=OWN, update=NO_UPDATE))
case("12-bf16-dropin-backward", "bf16", 192, 3, dropin_backward(96, 0, 3, 0), dict(path=LAYERS, wgrad=PER_LAYER, tail_on_caller=0, bias_finish=OWN))
case("12-bf16-dropin-backward-dx", "bf16", 192, 3, dropin_backward(96, 0, 3, 1), dict(path=LAYERS, wgrad=PER_LAYER, tail_on_caller=0, bias_finish=OWN))
F32_STEP = dict(path=LAYERS, loss=STANDALONE, loss_finish=OWN, wgrad=PER_LAYER, norm=FLAT_PASS, update=FLAT)
case("13-f32-small", "f32", 384, 3, train(128), F32_STEP)                                      # 128 rows < 256
case("14-f32-split-k", "f32", 384, 3, train(1280), F32_STEP)                                   # 3 x (3 x 3) = 27 tiles of 128 x 128 < 256
case("15-f32-grouped", "f32", 1536, 2, train(256), dict(F32_STEP, wgrad=GROUPED_F32, bias_finish=OWN))      # 2 x (12 x 12) = 288 >= 256

# ---- one case per setting (on the chain stack of case 01, and where the chain hides the field on the per-layer stack of case 02)
case("set-noise", "bf16", 192, 3, train(96), dict(path=LAYERS, loss=FUSED), settings=[("noise",)])
case("set-emphasis", "bf16", 192, 3, train(96), dict(path=LAYERS, loss=STANDALONE, loss_finish=OWN), settings=[("emphasis",)])
case("set-criterion", "bf16", 192, 3, train(96), dict(path=LAYERS, loss=STANDALONE, loss_finish=OWN), settings=[("criterion",)])
case("set-presence", "bf16", 192, 3, train(96), dict(path=LAYERS, loss=STANDALONE, loss_finish=OWN), settings=[("presence",)])
case("set-presence-eval", "bf16", 192, 3, evaluate(96), dict(path=LAYERS, loss=STANDALONE, loss_finish=OWN), settings=[("presence",)])
case("set-dropout", "bf16", 192, 3, train(96), dict(path=LAYERS, loss=FUSED, loss_finish=CARRIED), settings=[("dropout",)])
case("set-tied-chain", "bf16", 192, 3, train(96), dict(CHAIN_STEP, norm=FLAT_PASS), settings=[("tied",)])
case("set-tied-layers", "bf16", 192, 3, train(96), dict(LAYER_STEP, norm=FLAT_PASS), NO_CHAIN, settings=[("tied",)])
# the optimizer and the weight average ride in the update's launch: they move no field, and these cases pin that
case("set-optimizer", "bf16", 192, 3, train(96), CHAIN_STEP, settings=[("optimizer",)])
case("set-weight-average", "bf16", 192, 3, train(96), CHAIN_STEP, settings=[("average",)])
case("set-weight-average-layers", "bf16", 192, 3, train(96), LAYER_STEP, NO_CHAIN, settings=[("average",)])
case("forward-out-y", "bf16", 192, 3, forward_loss(96, out_y=1), dict(loss=STANDALONE, loss_finish=OWN))      # (the caller takes y: it must be stored)
case("no-transposed-shadow", "bf16", 192, 3, train(96), dict(path=LAYERS, update=FLAT), settings=[("no_shadow_wt",)])

# ---- one case per switch (NO_CHAIN, SINGLE_STREAM and NO_FUSED_LOSS are cases 02 - 04)
case("sw-no-folded-loss-finish", "bf16", 192, 3, train(96), dict(LAYER_STEP, loss_finish=OWN), dict(NO_CHAIN, CODAE_NO_FOLDED_LOSS_FINISH="1"))
case("sw-no-folded-bias-finish", "bf16", 1536, 5, train(64), dict(wgrad=GROUPED_PIPE, bias_finish=OWN), {"CODAE_NO_FOLDED_BIAS_FINISH": "1"})
case("sw-no-defer-wgrad", "bf16", 1536, 5, train(64), dict(wgrad=PER_LAYER, tail_on_caller=1, bias_finish=OWN), {"CODAE_NO_DEFER_WGRAD": "1"})
case("sw-no-fused-norm-chain", "bf16", 192, 3, train(96), dict(CHAIN_STEP, norm=FLAT_PASS), {"CODAE_NO_FUSED_NORM": "1"})
case("sw-no-fused-norm-layers", "bf16", 192, 3, train(96), dict(LAYER_STEP, norm=FLAT_PASS), dict(NO_CHAIN, CODAE_NO_FUSED_NORM="1"))
case("sw-flat-adam", "bf16", 192, 3, train(96), dict(CHAIN_STEP, update=FLAT), {"CODAE_FLAT_ADAM": "1"})
case("sw-tail-on-side", "bf16", 192, 3, train(96), dict(LAYER_STEP, tail_on_caller=0), dict(NO_CHAIN, CODAE_TAIL_ON_SIDE="1"))
case("sw-f32-gemm-native", "f32", 1536, 2, train(256), F32_STEP, {"CODAE_F32_GEMM": "native"})

# ---- both sides of every threshold
case("chain-2048-rows", "bf16", 192, 3, train(2048), dict(path=CHAIN, rows=2048), max_batch=2049)
case("chain-2049-rows", "bf16", 192, 3, train(2049), dict(path=LAYERS, rows=2112), max_batch=2049)
case("small-tiles-108", "bf16", 384, 3, train(64), dict(wgrad=PER_LAYER), NO_CHAIN)                  # 3 x (6 x 6) tiles of 64 x 64 < 128
case("small-tiles-144", "bf16", 384, 4, train(64), dict(wgrad=GROUPED_ONE_BARRIER), NO_CHAIN)        # 4 x 36 >= 128; 4 x (2 x 2) big tiles < 200
case("big-tiles-192", "bf16", 1536, 4, train(64), dict(wgrad=GROUPED_ONE_BARRIER, bias_finish=OWN))  # 4 x 48 < 200; 4 x 576 small tiles
case("big-tiles-240", "bf16", 1536, 5, train(64), dict(wgrad=GROUPED_PIPE, bias_finish=FOLDED))      # 5 x 48 >= 200
case("f32-255-rows", "f32", 1536, 2, train(255), dict(wgrad=PER_LAYER), max_batch=256)
case("f32-256-rows", "f32", 1536, 2, train(256), dict(wgrad=GROUPED_F32), max_batch=256)
# 16 gradient buffers: 15 layers keep one each, 16 rotate.  576 wide: 15 x 81 small tiles >= 128, 15 x 9 = 135 big tiles < 200
case("depth-15", "bf16", 576, 15, train(64), dict(path=LAYERS, wgrad=GROUPED_ONE_BARRIER))
case("depth-16", "bf16", 576, 16, train(64), dict(path=LAYERS, wgrad=PER_LAYER, tail_on_caller=1))
case("depth-1", "bf16", 192, 1, train(64), dict(wgrad=PER_LAYER, tail_on_caller=0, streams=2, bias_finish=OWN), NO_CHAIN)
case("depth-2", "bf16", 1536, 2, train(64), dict(wgrad=GROUPED_ONE_BARRIER, tail_on_caller=0))      # (2 x 576 small tiles; the tail needs 3 layers)
case("clip-off-chain", "bf16", 192, 3, train(96, clip=0), dict(CHAIN_STEP, norm=NO_CLIP))
case("clip-off-layers", "bf16", 192, 3, train(96, clip=0), dict(LAYER_STEP, norm=NO_CLIP), NO_CHAIN)
case("clip-off-update", "f32", 384, 3, update(clip=0), dict(norm=NO_CLIP, update=FLAT))
case("update-f32", "f32", 384, 3, update(), dict(norm=FLAT_PASS, update=FLAT))
# a ranged backward: joined or not, reaching layer 0 or not (the tail needs both, and 3 layers)
RANGE = dict(path=LAYERS, loss=NO_LOSS, wgrad=PER_LAYER, streams=2, norm=NO_CLIP, update=NO_UPDATE)
case("range-0-3-join", "bf16", 192, 3, backward(96, 0, 3, join=1), dict(RANGE, tail_on_caller=1, bias_finish=OWN), NO_CHAIN)
case("range-0-3-async", "bf16", 192, 3, backward(96, 0, 3, join=0), dict(RANGE, tail_on_caller=0, bias_finish=OWN), NO_CHAIN)
case("range-1-3-join", "bf16", 192, 3, backward(96, 1, 3, join=1), dict(RANGE, tail_on_caller=0, bias_finish=OWN), NO_CHAIN)
case("range-1-3-async", "bf16", 192, 3, backward(96, 1, 3, join=0), dict(RANGE, tail_on_caller=0, bias_finish=NONE), NO_CHAIN)
case("range-0-2-join", "bf16", 192, 3, backward(96, 0, 2, join=1), dict(RANGE, tail_on_caller=0, bias_finish=OWN), NO_CHAIN)
# the whole stack joined takes the step's grouped schedule; a part of it, or an unjoined call, does not
case("range-wide-whole", "bf16", 1536, 5, backward(64, 0, 5, join=1), dict(wgrad=GROUPED_PIPE, bias_finish=FOLDED, norm=NO_CLIP))
case("range-wide-async", "bf16", 1536, 5, backward(64, 0, 5, join=0), dict(wgrad=PER_LAYER, bias_finish=OWN))
case("range-wide-part", "bf16", 1536, 5, backward(64, 1, 5, join=1), dict(wgrad=PER_LAYER, bias_finish=OWN))
# drop-in backward of the wide stack: the step's schedule unless an input gradient is asked for
case("dropin-wide", "bf16", 1536, 5, dropin_backward(64, 0, 5, 0), dict(wgrad=GROUPED_PIPE, bias_finish=FOLDED))
case("dropin-wide-dx", "bf16", 1536, 5, dropin_backward(64, 0, 5, 1), dict(wgrad=PER_LAYER, tail_on_caller=0, bias_finish=OWN))


class Engine:
    """An engine created without a device: codae_create and the setters used here make no HIP call."""

    def __init__(self, lib, c):
        from codae import hip
        self.lib, self.hip = lib, hip
        io, L = c["io"], c["L"]
        nb_in, nb_out = (L - 1) // 2, (L - 2) // 2                       # bench.square_schedule
        relu = [1] * nb_in + [0] + [1] * nb_out + [0] if L >= 2 else [0]
        assert len(relu) == L
        self.keep = [(C.c_int32 * L)(*[io] * L), (C.c_int32 * L)(*[io] * L), (C.c_uint8 * L)(*relu)]
        spec = hip.Spec(L, self.keep[0], self.keep[1], self.keep[2], c["max_batch"], hip.PREC_BF16 if c["prec"] == "bf16" else hip.PREC_F32)
        if ("act", "leaky") in c["settings"]:
            self.keep += [(C.c_uint8 * L)(*[hip.ACT_LEAKY if r else hip.ACT_NONE for r in relu]), (C.c_float * (3 * L))(*[0.1, 0.0, 0.0] * L)]
            spec.act_kind, spec.act_param = self.keep[-2], self.keep[-1]
        self.h = C.c_void_p()
        assert lib.codae_create(C.byref(spec), C.byref(self.h)) == 0, lib.codae_last_error()
        # (never read through: dummy non-null members, as the engine fills them - no transposed shadow in fp32)
        some = C.cast((C.c_char * 64)(), C.c_void_p)
        self.keep.append(some)
        wt = some if c["prec"] == "bf16" and ("no_shadow_wt",) not in c["settings"] else None
        self.bufs = hip.Buffers(some, some, some, some, some, some, some, some, some, wt, some)
        for s in c["settings"]:
            getattr(self, "set_" + s[0])(io, L)

    def ok(self, rc):
        assert rc == 0, self.lib.codae_last_error()

    def set_act(self, io, L): pass
    def set_no_shadow_wt(self, io, L): pass

    def set_noise(self, io, L):
        self.ok(self.lib.codae_set_input_noise(self.h, C.byref(self.hip.Noise(self.hip.NOISE_MASKING, 0.25, 0.0, 0.0, 7))))

    def set_emphasis(self, io, L):
        self.ok(self.lib.codae_set_loss_emphasis(self.h, C.byref(self.hip.Emphasis(2.0, 0.5, None))))

    def set_criterion(self, io, L):
        self.ok(self.lib.codae_set_recon_loss(self.h, C.byref(self.hip.ReconLoss(self.hip.LOSS_L1, 0.0, 0.0, 0))))

    def set_presence(self, io, L):
        table = (C.c_uint8 * 12)(*[1] * 12)
        self.keep.append(table)
        self.ok(self.lib.codae_set_slot_presence(self.h, C.cast(table, C.c_void_p), 4, 3))

    def set_dropout(self, io, L):
        p = (C.c_float * (L - 1))(*[0.25] * (L - 1))
        self.ok(self.lib.codae_set_hidden_dropout(self.h, C.byref(self.hip.Dropout(p, L - 1, 11))))

    def set_tied(self, io, L):
        self.ok(self.lib.codae_set_tied_weights(self.h, 1))

    def set_optimizer(self, io, L):
        opt = self.hip.Optimizer(self.hip.OPT_ADAMW, 0, 0.0, 0, self.hip.SCHED_COSINE, 2, 100, 0, 0.1, 0.0, None)
        self.ok(self.lib.codae_set_optimizer(self.h, C.byref(opt)))

    def set_average(self, io, L):
        room = (C.c_char * 64)()
        self.keep.append(room)
        avg = C.c_void_p((C.addressof(room) + 15) // 16 * 16)            # (the setter asks for 16-byte alignment; never read through)
        self.ok(self.lib.codae_set_weight_average(self.h, C.byref(self.hip.WeightAverage(self.hip.AVG_EMA, 0.99, 1, 1, 1, avg))))

    def plan(self, call, capacity=len(FIELDS)):
        out = (C.c_int32 * len(FIELDS))()
        rc = self.lib.codae_debug_step_plan(self.h, C.byref(self.bufs), (C.c_int32 * 8)(*call), out, capacity)
        return rc, dict(zip(FIELDS, list(out)))

    def close(self):
        self.lib.codae_destroy(self.h)


def with_engine(lib, name, f):
    """f(engine) for CASES[name]: its switches set while the engine is created (codae_create reads them) and restored afterwards.
    lib: any ctypes handle of the library (the fixture's recorder passes the recording build's)."""
    c = CASES[name]
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    try:
        os.environ.update(c["env"])
        e = Engine(lib, c)
        try:
            return f(e)
        finally:
            e.close()
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
        lib.codae_reload_env()


def query(lib, name):
    rc, got = with_engine(lib, name, lambda e: e.plan(CASES[name]["call"]))
    assert rc == 0, (name, rc, lib.codae_last_error())
    return got


@pytest.fixture(scope="module")
def lib():
    from codae import hip
    return hip.lib()


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_exactly_the_cases(golden):
    assert golden["commit"] == "4b4c61f" and golden["fields"] == FIELDS
    assert sorted(golden["cases"]) == sorted(CASES)
    for name, g in golden["cases"].items():
        c = CASES[name]
        assert g["call"] == c["call"] and g["env"] == c["env"] and g["settings"] == [list(s) for s in c["settings"]], name
        assert (g["prec"], g["io"], g["L"], g["max_batch"]) == (c["prec"], c["io"], c["L"], c["max_batch"]), name


def test_every_switch_and_field_value_is_reached(golden):
    """The cases name every switch, and the recorded plans take every value of every enumerated field."""
    assert {k for c in CASES.values() for k in c["env"]} == set(SWITCHES)
    seen = {f: {g["plan"][f] for g in golden["cases"].values()} for f in FIELDS}
    assert seen["path"] == {0, 1} and seen["loss"] == {0, 1, 2, 3} and seen["loss_finish"] == {0, 1, 2}
    assert seen["wgrad"] == {0, 1, 2, 3} and seen["streams"] == {1, 2} and seen["tail_on_caller"] == {0, 1}
    assert seen["bias_finish"] == {0, 1, 2} and seen["norm"] == {0, 1, 2} and seen["update"] == {0, 1, 2}


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_matches_the_recorded_decisions(name, lib, golden):
    got = query(lib, name)
    for field, value in CASES[name]["want"].items():
        assert got[field] == value, (name, field, got)
    assert got == golden["cases"][name]["plan"], (name, got, golden["cases"][name]["plan"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_step_path_is_the_plans_path(name, lib):
    """codae_step_path is the `path` of the fused step's plan, whatever call the case itself describes."""
    B = CASES[name]["call"][1] or CASES[name]["max_batch"]

    def both(e):
        rc, got = e.plan(train(B))
        assert rc == 0
        return lib.codae_step_path(e.h, C.byref(e.bufs), B), got["path"]
    path, planned = with_engine(lib, name, both)
    assert path == planned, (name, path, planned)
    if CASES[name]["call"][0] == TRAIN:
        assert "path" not in CASES[name]["want"] or path == CASES[name]["want"]["path"]


def test_query_refuses_a_short_output_a_null_handle_and_a_bad_call(lib):
    def refusals(e):
        call = CASES["02-bf16-layers"]["call"]
        assert e.plan(call)[0] == 0
        assert e.plan(call, capacity=len(FIELDS) - 1)[0] != 0
        out, c8 = (C.c_int32 * len(FIELDS))(), (C.c_int32 * 8)(*call)
        assert lib.codae_debug_step_plan(None, C.byref(e.bufs), c8, out, len(FIELDS)) != 0
        assert lib.codae_debug_step_plan(e.h, None, c8, out, len(FIELDS)) != 0
        assert e.plan([6] + call[1:])[0] != 0                          # unknown kind
        assert e.plan(train(97))[0] != 0                               # more rows than max_batch
        assert e.plan(backward(96, 2, 4))[0] != 0                      # a range outside the stack
        assert e.plan(backward(96, 1, 1))[0] != 0
        assert lib.codae_step_path(None, C.byref(e.bufs), 96) == 0 and lib.codae_step_path(e.h, C.byref(e.bufs), 97) == 0
    with_engine(lib, "02-bf16-layers", refusals)


if __name__ == "__main__":
    # the recorder: LIBRARY = a build of the recording commit plus the patch that adds only the query (see the docstring)
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(ROOT, "mui-deepautoencoder_amd"))
    import torch  # noqa: F401  -- loads the HIP runtime the library links
    from codae import hip as binding
    rec = C.CDLL(sys.argv[1], mode=C.RTLD_GLOBAL)
    for fn, (res, args) in binding.PROTOTYPES.items():
        if hasattr(rec, fn):
            getattr(rec, fn).restype, getattr(rec, fn).argtypes = res, args
    cases = {n: dict(prec=c["prec"], io=c["io"], L=c["L"], max_batch=c["max_batch"], call=c["call"], env=c["env"], settings=c["settings"],
                     plan=query(rec, n)) for n, c in sorted(CASES.items())}
    json.dump(dict(commit="4b4c61f", recorded_with="tests/test_step_plan_host.py on that commit + the query alone", fields=FIELDS,
                   cases=cases), sys.stdout, indent=1)
    sys.stdout.write("\n")
