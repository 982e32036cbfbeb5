"""Which kernel every bf16 GEMM launch takes, pinned on the host (no GPU).

gemm_bf16_plan (csrc/gemm_bf16.hip) is the one function that turns a descriptor into tile, kernel family, stages, loader
layout, epilogue, store policy and grid; gemm_bf16() launches what it says and the engine's partial-sum row counts read the same
answer.  codae_debug_gemm_bf16_plan returns that plan without making a HIP call.  This file compares it, for one descriptor per
branch and both sides of every threshold, verbatim against tests/golden/gemm_bf16_plan.json.

The fixture was recorded on the commit it names - the last one whose launchers decided for themselves - from a dry run of
gemm_bf16(): the template arguments and grid of the launch it would have made, and that commit's gemm_bf16_colsum_rows /
_loss_parts / _takes_relu_bits.  Under CODAE_GEMM_TILE=m and CODAE_GEMM_DBG that commit counted rows and parts for the tile the
automatic choice would have taken, not the one it launched; the fixture keeps its kernel record there and carries the counts that
match the recorded tile (its own answers are kept beside them as `parent_counts`).

`want` restates per case, independently of the fixture, which kernel family and tile the case is meant to reach (and the stages
where that is the point), so that a shape that missed its branch on the recording commit could not have been recorded as if it
had taken it.
"""
import ctypes as C
import json
import os

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_bf16_plan.json")
FIELDS = ["family", "bm", "bn", "stages", "loader", "epi", "dbg", "act", "store_policy", "tiles_m", "tiles_n", "workgroups",
          "colsum_rows", "loss_parts", "takes_relu_bits"]
COUNT_FIELDS = ("colsum_rows", "loss_parts", "takes_relu_bits")
KC, KS = 0, 1
ONE_BARRIER, PIPELINED = 0, 1
PLAIN, WT, BY_SIZE = 0, 1, -1
LEAKY = 2
SWITCHES = ("CODAE_GEMM_TILE", "CODAE_NO_DEEP_SMALL", "CODAE_SMALL_TILE_MAX", "CODAE_SMALL_STAGES", "CODAE_GEMM_DBG", "CODAE_STORE_POLICY")


def desc(M, N, K=384, a=KC, b=KC, f32=0, split=1, act=0, loss=0, bwd=0, cosched=0, policy=WT, ldc=None):
    return [a, b, f32, M, N, K, split, act, loss, bwd, cosched, policy, N if ldc is None else ldc]


def fwd(M, N, K=384, **kw): return desc(M, N, K, **kw)
def dgrad_w(M, N, K=384, **kw): return desc(M, N, K, b=KS, **kw)                    # the data gradient through W itself
def wgrad(N, K, rows, split): return desc(N, K, rows, a=KS, b=KS, f32=1, split=split)
def loss(M, N): return desc(M, N, loss=1, bwd=1)                                      # (the engine hands it the column-sum rows)


CASES = {}


def case(name, d, want, env=None):
    """want: (family, bm, bn) or (family, bm, bn, stages)"""
    assert name not in CASES, name
    CASES[name] = dict(desc=d, want=want, env=env or {})


# ---- forward form (both operands k-contiguous, bf16 output), with and without the backward epilogue
for tag, kw in (("", {}), ("-bwd", dict(bwd=1))):
    case("fwd-96x192-k384" + tag, fwd(96, 192, 384, **kw), (ONE_BARRIER, 64, 64, 4))          # 6 workgroups, 6 K-tiles: four stages
    case("fwd-96x192-k320" + tag, fwd(96, 192, 320, **kw), (ONE_BARRIER, 64, 64, 2))          # 5 K-tiles
    case("fwd-2048x1536" + tag, fwd(2048, 1536, **kw), (ONE_BARRIER, 64, 64, 2))              # 768 workgroups > 256
    case("fwd-3200x1024" + tag, fwd(3200, 1024, **kw), (ONE_BARRIER, 64, 64, 2))              # 200 tiles of 128 x 128: still small
    case("fwd-3328x1024" + tag, fwd(3328, 1024, **kw), (PIPELINED, 128, 192))                 # 208
    case("fwd-4864x1536" + tag, fwd(4864, 1536, **kw), (PIPELINED, 128, 192))                 # 152 tiles of 256 x 192
    case("fwd-5120x1536" + tag, fwd(5120, 1536, **kw), (PIPELINED, 256, 192))                 # 160
# coscheduled: the compiler-scheduled variant only with a backward epilogue, and only on 256 x 192
case("fwd-5120x1536-cosched", fwd(5120, 1536, cosched=1), (PIPELINED, 256, 192))
case("fwd-5120x1536-bwd-cosched", fwd(5120, 1536, bwd=1, cosched=1), (PIPELINED, 256, 192))
case("fwd-4864x1536-bwd-cosched", fwd(4864, 1536, bwd=1, cosched=1), (PIPELINED, 128, 192))
# fp32 output; k-strided B; the weight-gradient form
case("fwd-f32-96x192", fwd(96, 192, f32=1), (ONE_BARRIER, 128, 128, 2))
case("fwd-f32-5120x1536", fwd(5120, 1536, f32=1), (PIPELINED, 256, 192))
case("dgradw-96x192-bwd", dgrad_w(96, 192, bwd=1), (ONE_BARRIER, 128, 128, 2))
case("dgradw-5120x1536-bwd", dgrad_w(5120, 1536, bwd=1), (PIPELINED, 256, 192))
case("dgradw-5120x1536-bwd-cosched", dgrad_w(5120, 1536, bwd=1, cosched=1), (PIPELINED, 256, 192))
for s in (1, 5, 8):
    case("wgrad-192x192-split%d" % s, wgrad(192, 192, 512, s), (ONE_BARRIER, 128, 128, 2))
    # 48 tiles of 256 x 192: unsplit below 160 workgroups, split 5 / 8 above
    case("wgrad-1536x1536-split%d" % s, wgrad(1536, 1536, 512, s), (ONE_BARRIER, 128, 128, 2) if s == 1 else (PIPELINED, 256, 192))
case("wgrad-2560x3072-split1", wgrad(2560, 3072, 512, 1), (PIPELINED, 256, 192))              # 160 unsplit
# ---- fused loss: all three tiles
case("loss-96x192", loss(96, 192), (ONE_BARRIER, 64, 64, 2))
case("loss-3328x1024", loss(3328, 1024), (ONE_BARRIER, 128, 128, 2))
case("loss-8192x1536", loss(8192, 1536), (PIPELINED, 256, 192))
# ---- a generic activation: the one-barrier kernel whatever the size
case("act-96x192-k384", fwd(96, 192, 384, act=LEAKY), (ONE_BARRIER, 64, 64, 4))
case("act-96x192-k320", fwd(96, 192, 320, act=LEAKY, bwd=1), (ONE_BARRIER, 64, 64, 2))
case("act-3328x1024", fwd(3328, 1024, act=LEAKY), (ONE_BARRIER, 128, 128, 4))             # 208 workgroups <= 256
case("act-8192x1536-bwd", fwd(8192, 1536, act=LEAKY, bwd=1), (ONE_BARRIER, 128, 128, 2))
case("act-dgradw-96x192-bwd", dgrad_w(96, 192, act=LEAKY, bwd=1), (ONE_BARRIER, 128, 128, 2))
case("act-f32-96x192", fwd(96, 192, f32=1, act=LEAKY), (ONE_BARRIER, 128, 128, 2))
# ---- store policy: kept, demoted by a row stride of 2^20 elements, plain; and by the output's size (32 MiB)
case("policy-wt-ldc-2p20", fwd(5120, 1536, ldc=1 << 20), (PIPELINED, 256, 192))
case("policy-wt-ldc-below", fwd(5120, 1536, ldc=(1 << 20) - 8), (PIPELINED, 256, 192))
case("policy-plain", fwd(5120, 1536, policy=PLAIN), (PIPELINED, 256, 192))
case("policy-mid-plain", fwd(3328, 1024, policy=PLAIN, bwd=1), (PIPELINED, 128, 192))
case("policy-by-size-16MB", fwd(5120, 1536, policy=BY_SIZE), (PIPELINED, 256, 192))
case("policy-by-size-35MB", fwd(8192, 2112, policy=BY_SIZE), (PIPELINED, 256, 192))
# ---- under switches
for t, big in (("s", None), ("q", (PIPELINED, 256, 192)), ("x", (PIPELINED, 256, 192))):
    env = {"CODAE_GEMM_TILE": t}
    case("tile-%s-fwd-96x192" % t, fwd(96, 192), big or (ONE_BARRIER, 64, 64, 4), env)
    case("tile-%s-fwd-5120x1536-bwd" % t, fwd(5120, 1536, bwd=1), big or (PIPELINED, 128, 192), env)
    case("tile-%s-loss-96x192" % t, loss(96, 192), big or (ONE_BARRIER, 64, 64, 2), env)
    case("tile-%s-loss-8192x1536" % t, loss(8192, 1536), big or (ONE_BARRIER, 128, 128, 2), env)
    case("tile-%s-wgrad-1536x1536-split5" % t, wgrad(1536, 1536, 512, 5), big or (ONE_BARRIER, 128, 128, 2), env)
    case("tile-%s-dgradw-96x192-bwd" % t, dgrad_w(96, 192, bwd=1), big or (ONE_BARRIER, 128, 128, 2), env)
    case("tile-%s-act-96x192" % t, fwd(96, 192, act=LEAKY), (ONE_BARRIER, 64, 64, 4), env)
TILE_M = {"CODAE_GEMM_TILE": "m"}
case("tile-m-fwd-96x192", fwd(96, 192), (PIPELINED, 128, 192), TILE_M)
case("tile-m-fwd-256x1024-bwd", fwd(256, 1024, 1024, bwd=1), (PIPELINED, 128, 192), TILE_M)    # two column-sum rows, not one
case("tile-m-fwd-5120x1536-bwd", fwd(5120, 1536, bwd=1), (PIPELINED, 128, 192), TILE_M)
case("tile-m-loss-96x192", loss(96, 192), (PIPELINED, 256, 192), TILE_M)                      # (no fused loss on 128 x 192)
case("tile-m-loss-8192x1536", loss(8192, 1536), (PIPELINED, 256, 192), TILE_M)
case("tile-m-act-96x192", fwd(96, 192, act=LEAKY), (ONE_BARRIER, 64, 64, 4), TILE_M)
NO_DEEP = {"CODAE_NO_DEEP_SMALL": "1"}
case("no-deep-fwd-96x192", fwd(96, 192), (ONE_BARRIER, 128, 128, 2), NO_DEEP)
case("no-deep-fwd-3328x1024", fwd(3328, 1024), (ONE_BARRIER, 128, 128, 2), NO_DEEP)
case("no-deep-act-96x192", fwd(96, 192, act=LEAKY), (ONE_BARRIER, 128, 128, 2), NO_DEEP)
case("no-deep-loss-96x192", loss(96, 192), (ONE_BARRIER, 128, 128, 2), NO_DEEP)
SMALL0 = {"CODAE_SMALL_TILE_MAX": "0"}
case("small-max0-fwd-96x192", fwd(96, 192), (PIPELINED, 128, 192), SMALL0)
case("small-max0-loss-96x192", loss(96, 192), (ONE_BARRIER, 128, 128, 2), SMALL0)
case("small-max0-act-96x192", fwd(96, 192, act=LEAKY), (ONE_BARRIER, 128, 128, 4), SMALL0)
case("small-stages2-fwd-96x192", fwd(96, 192), (ONE_BARRIER, 64, 64, 2), {"CODAE_SMALL_STAGES": "2"})
case("small-stages2-act-96x192", fwd(96, 192, act=LEAKY), (ONE_BARRIER, 64, 64, 2), {"CODAE_SMALL_STAGES": "2"})
for pol in ("plain", "wt"):
    env = {"CODAE_STORE_POLICY": pol}
    case("store-%s-by-size-16MB" % pol, fwd(5120, 1536, policy=BY_SIZE), (PIPELINED, 256, 192), env)
    case("store-%s-by-size-35MB" % pol, fwd(8192, 2112, policy=BY_SIZE), (PIPELINED, 256, 192), env)
    case("store-%s-by-size-mid" % pol, fwd(3328, 1024, policy=BY_SIZE), (PIPELINED, 128, 192), env)


def query(lib, name):
    """The library's answer for CASES[name] as {field: value}: its switches set for this one call and restored afterwards.
    lib: any ctypes handle of the library (the fixture's recorder passes the recording commit's)."""
    c = CASES[name]
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    try:
        os.environ.update(c["env"])
        assert lib.codae_reload_env() == 0
        d, out = (C.c_int32 * 13)(*c["desc"]), (C.c_int32 * len(FIELDS))()
        rc = lib.codae_debug_gemm_bf16_plan(d, out, len(FIELDS))
        assert rc == 0, (name, rc)
        return dict(zip(FIELDS, list(out)))
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
        lib.codae_reload_env()


@pytest.fixture(scope="module")
def lib():
    from codae import hip
    return hip.lib()


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_exactly_the_cases(golden):
    assert golden["commit"] == "5608f9d" and golden["fields"] == FIELDS
    assert sorted(golden["cases"]) == sorted(CASES)
    for name, g in golden["cases"].items():
        assert g["desc"] == CASES[name]["desc"] and g["env"] == CASES[name]["env"], name
        # the recording commit's own counts differ from the fixture's only under the switch that misled them
        if "parent_counts" in g:
            assert set(CASES[name]["env"]) & {"CODAE_GEMM_TILE"}, name


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_matches_the_recorded_launch(name, lib, golden):
    got, want = query(lib, name), CASES[name]["want"]
    assert (got["family"], got["bm"], got["bn"]) == want[:3], (name, got)
    if len(want) > 3:
        assert got["stages"] == want[3], (name, got)
    assert got == golden["cases"][name]["plan"], (name, got, golden["cases"][name]["plan"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_counts_follow_the_tile(name, lib):
    """What the engine adds up is what the kernel writes: one column-sum row per tile along M, one pair of metric sums per
    workgroup of the fused-loss launch, the grid = tiles x split - whatever the switches."""
    c, got = CASES[name], query(lib, name)
    M, N, split, has_loss = c["desc"][3], c["desc"][4], c["desc"][6], c["desc"][8]
    assert got["tiles_m"] == -(-M // got["bm"]) and got["tiles_n"] == -(-N // got["bn"])
    assert got["workgroups"] == got["tiles_m"] * got["tiles_n"] * split
    assert got["colsum_rows"] == got["tiles_m"]
    assert got["loss_parts"] == (got["tiles_m"] * got["tiles_n"] if has_loss else 0)
    assert (got["epi"] == 3) == bool(has_loss)


def test_forced_mid_tile_leaves_other_forms_to_the_automatic_choice(lib):
    """CODAE_GEMM_TILE=m names an instantiation that exists for the forward form only.  The recording commit sent every other
    form to it as well and its launcher refused them (nothing to record); now they take what they take without the switch."""
    for name in ("fwd-f32-96x192", "fwd-f32-5120x1536", "dgradw-96x192-bwd", "dgradw-5120x1536-bwd", "wgrad-1536x1536-split1",
                 "wgrad-1536x1536-split5"):
        plain = query(lib, name)
        CASES["_forced"] = dict(CASES[name], env={"CODAE_GEMM_TILE": "m"})
        try:
            forced = query(lib, "_forced")
        finally:
            del CASES["_forced"]
        # (the 1-bit mask answer is about the forward form of that output shape, which the switch does move)
        assert {k: v for k, v in forced.items() if k != "takes_relu_bits"} == {k: v for k, v in plain.items() if k != "takes_relu_bits"}, name


def test_the_removed_ablation_switch_is_not_read(lib):
    """CODAE_GEMM_DBG once selected timing builds of the pipelined kernel whose results were wrong by design (family 2).  The
    builds are gone and the variable is not read: the plan under it is the plan without it, field for field."""
    for d in (fwd(96, 192), loss(96, 192), fwd(3328, 1024, bwd=1, policy=PLAIN)):
        CASES["_unset"] = dict(desc=d, want=None, env={})
        CASES["_dbg8"] = dict(desc=d, want=None, env={"CODAE_GEMM_DBG": "8"})
        try:
            unset, dbg8 = query(lib, "_unset"), query(lib, "_dbg8")
        finally:
            del CASES["_unset"], CASES["_dbg8"]
        assert sorted(dbg8) == sorted(FIELDS)
        for f in FIELDS:
            assert dbg8[f] == unset[f], (d, f, dbg8, unset)
        assert dbg8["family"] != 2 and unset["family"] != 2, (d, dbg8)


def test_query_refuses_a_short_output_and_a_bad_shape(lib):
    d, out = (C.c_int32 * 13)(*fwd(96, 192)), (C.c_int32 * len(FIELDS))()
    assert lib.codae_debug_gemm_bf16_plan(d, out, len(FIELDS) - 1) != 0
    d = (C.c_int32 * 13)(*fwd(96, 192, 100))
    assert lib.codae_debug_gemm_bf16_plan(d, out, len(FIELDS)) != 0
