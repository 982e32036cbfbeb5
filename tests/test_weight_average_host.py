"""Host-side tests of the weight average (no device): the bound of tests/average_ref.py is fixed here against an fp32 emulation of
both evaluation orders, codae.tool.WeightAverage states the same definition on host tensors, the setting is validated, and the
header, the binding and the built library carry the two new entries under ABI 11."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import average_ref as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = tuple(range(1, 9)) + (1000,)
# EMA with and without debias, SWA; start 1 and 3; every 1 and 2
CASES = [(kind, debias, start, every) for (kind, debias) in (("ema", True), ("ema", False), ("swa", False))
         for start in (1, 3) for every in (1, 2)]


def tool_of(kind, debias, start, every, decay=0.999):
    from codae.tool import WeightAverage
    return WeightAverage(kind, decay=decay, debias=debias, start=start, every=every)


def test_weight_follows_the_definition():
    for kind, debias, start, every in CASES:
        tool = tool_of(kind, debias, start, every)
        s = AR.setting_of(tool)
        for t in STEPS:
            w = tool.weight(t)
            samples = t >= start and (t - start) % every == 0
            assert (w is not None) == samples, (s, t)
            ref = AR.weight32(s, t)
            assert (ref is None) == (w is None) and (w is None or np.float32(w) == ref), (s, t, w, ref)
            if not samples:
                continue
            n = (t - start) // every
            if kind == "swa":
                assert w == float(np.float32(1.0 / (n + 1)))
            elif n == 0:
                assert w == 1.0
            elif debias:
                assert w == float(np.float32(1.0 - min(s.decay, (1.0 + n) / (10.0 + n))))
            else:
                assert w == float(np.float32(1.0 - s.decay))
    # debias hands over to the decay once (1 + n) / (10 + n) exceeds it: for decay 0.9 that is n = 80 (81 / 90 against fp32 0.9)
    t9 = tool_of("ema", True, 1, 1, decay=0.9)
    assert t9.weight(80) == float(np.float32(1.0 - 80.0 / 89.0)) and t9.weight(82) == float(np.float32(1.0 - float(np.float32(0.9))))
    assert tool_of("off", True, 1, 1).weight(1) is None and tool_of("off", True, 1, 1).is_default and not tool_of("ema", True, 1, 1).is_default


def test_bound_holds_for_both_evaluation_orders_and_for_the_host_update():
    a, p = AR.planted(4099, 11)
    worst = {}
    for kind, debias, start, every in CASES:
        tool = tool_of(kind, debias, start, every)
        s = AR.setting_of(tool)
        for t in STEPS:
            w = AR.weight32(s, t)
            want, tol = AR.step64(a, p, w), AR.bound(a, p)
            got = {order: AR.emulate32(a, p, w, order) for order in ("plain", "fma")}
            got["host"] = tool.update(torch.from_numpy(a.copy()), torch.from_numpy(p.copy()), t).numpy()
            for name, g in got.items():
                r = AR.worst_ratio(g, want, tol)
                worst[name] = max(worst.get(name, 0.0), r)
                assert r <= 1.0, "%r t %d %s: %.3f bounds from the float64 definition" % (s, t, name, r)
                if w is None:
                    assert np.array_equal(g.view(np.uint32), a.view(np.uint32)), "%r t %d %s: avg moved on a non-sampling step" % (s, t, name)
                elif w == np.float32(1):
                    assert np.array_equal(g.view(np.uint32), p.view(np.uint32)), "%r t %d %s: not a bit copy at w32 == 1" % (s, t, name)
    print("MEASURE weight average host: worst |error| / bound  " + "  ".join("%s %.3f" % kv for kv in sorted(worst.items())))
    assert worst["plain"] > 0.05, "the bound is vacuous against the emulation: %r" % (worst,)


def test_host_update_keeps_nan_and_refuses_mismatched_tensors():
    from codae.hip import HipError
    tool = tool_of("ema", False, 1, 1, decay=0.9)
    a, p = torch.zeros(8), torch.ones(8)
    p[3] = float("nan")
    for t in (1, 2):
        out = tool.update(a.clone(), p, t)
        assert torch.isnan(out[3]) and torch.isfinite(torch.cat([out[:3], out[4:]])).all()
    with pytest.raises(HipError):
        tool.update(torch.zeros(8), torch.zeros(9), 1)
    with pytest.raises(HipError):
        tool.update(torch.zeros(8, dtype=torch.float64), torch.zeros(8, dtype=torch.float64), 1)


def test_swa_over_six_snapshots_is_their_mean():
    N = 6
    rng = np.random.default_rng(5)
    snaps = [(rng.standard_normal(1000) * 3).astype(np.float32) for _ in range(N)]
    mean = np.mean(np.stack([x.astype(np.float64) for x in snaps]), axis=0)
    tol = AR.swa_mean_bound(snaps)
    tool = tool_of("swa", False, 1, 1)
    s = AR.setting_of(tool)
    host = torch.full((1000,), 77.0)
    emu = {order: np.full(1000, 77.0, dtype=np.float32) for order in ("plain", "fma")}
    for t, x in enumerate(snaps, start=1):
        tool.update(host, torch.from_numpy(x), t)
        for order in emu:
            emu[order] = AR.emulate32(emu[order], x, AR.weight32(s, t), order)
    emu["host"] = host.numpy()
    for name, g in emu.items():
        r = AR.worst_ratio(g, mean, tol)
        print("MEASURE weight average host: swa over %d snapshots, %s: worst |error| / bound %.3f" % (N, name, r))
        assert r <= 1.0, (name, r)


def test_arguments_are_validated():
    from codae.hip import HipError
    from codae.tool import WeightAverage, weight_average_from_config
    for bad in (dict(decay=1.0), dict(decay=-0.1), dict(decay=float("nan")), dict(decay="0.9"), dict(start=0), dict(start=1.5), dict(every=0),
                dict(every=-2), dict(kind="polyak"), dict(kind=None), dict(debias=1)):
        with pytest.raises(HipError):
            WeightAverage(**bad)
    with pytest.raises(HipError):
        WeightAverage().weight(0)
    with pytest.raises(HipError, match="DECAI"):
        weight_average_from_config({"KIND": "ema", "DECAI": 0.9})
    with pytest.raises(HipError):
        weight_average_from_config({"KIND": "ema", "START": 2, "START_EPOCH": 2}, 10)
    with pytest.raises(HipError):
        weight_average_from_config({"KIND": "ema", "START_EPOCH": 2})
    assert weight_average_from_config(None) is None and weight_average_from_config({}) is None
    w = weight_average_from_config({"KIND": "swa", "START_EPOCH": 3, "EVERY": 2}, batches_per_epoch=10)
    assert (w.kind, w.start, w.every) == ("swa", 21, 2)
    w = WeightAverage("ema", decay=0.99, debias=False, start=4, every=3)
    back = weight_average_from_config(w.as_config())
    assert repr(back) == repr(w) and eval(repr(w), {"WeightAverage": WeightAverage}).as_config() == w.as_config()
    d = WeightAverage()
    assert (d.kind, d.decay, d.debias, d.start, d.every) == ("ema", float(np.float32(0.999)), True, 1, 1)


def test_struct_header_and_library_carry_the_new_entries():
    from codae import hip
    from codae.tool import WeightAverage
    header = open(os.path.join(ROOT, "include", "codae_hip.h")).read()
    assert int(re.search(r"#define CODAE_ABI_VERSION (\d+)", header).group(1)) == 11 == hip.ABI_VERSION
    assert "Weight average" in header
    enums = {k: int(v) for k, v in re.findall(r"\b(CODAE_AVG_[A-Z]+)\s*=\s*(\d+)", header)}
    assert enums == {"CODAE_AVG_OFF": hip.AVG_OFF, "CODAE_AVG_EMA": hip.AVG_EMA, "CODAE_AVG_SWA": hip.AVG_SWA} == \
        {"CODAE_AVG_OFF": 0, "CODAE_AVG_EMA": 1, "CODAE_AVG_SWA": 2}
    body = re.search(r"typedef struct \{([^}]*)\} codae_weight_average;", header).group(1)
    fields = re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", body))
    assert fields == [n for n, _ in hip.WeightAverage._fields_] == ["kind", "decay", "debias", "start", "every", "avg"]
    assert C.sizeof(hip.WeightAverage) == 32 and hip.WeightAverage.avg.offset == 24
    lib = hip.lib()
    assert lib.codae_abi_version() == 11
    for name, n_args in (("codae_set_weight_average", 2), ("codae_weight_average_update", 6)):
        m = re.search(r"\bint %s\(([^)]*)\)" % name, header)
        assert m is not None and m.group(1).count(",") + 1 == n_args == len(hip.PROTOTYPES[name][1]), name
        assert hasattr(lib, name), name
    st = WeightAverage("swa", start=5, every=2).as_struct(None)
    assert (st.kind, st.start, st.every, st.avg) == (hip.AVG_SWA, 5, 2, None)
    st = WeightAverage("ema", decay=0.5, debias=False).as_struct(C.c_void_p(4096))
    assert (st.kind, st.decay, st.debias, st.avg) == (hip.AVG_EMA, 0.5, 0, 4096)


def test_the_setter_refuses_a_bad_struct_and_keeps_the_previous_one():
    """No device: a handle is host memory, and codae_step_update_span refuses, before its first HIP call, exactly while a weight
    average is in force - which tells whether a refused setting replaced the one before it."""
    from codae import hip
    lib = hip.lib()
    ins, outs, relu = (C.c_int32 * 2)(48, 16), (C.c_int32 * 2)(16, 48), (C.c_uint8 * 2)(1, 0)
    spec = hip.Spec(2, ins, outs, relu, 16, hip.PREC_F32)
    h = C.c_void_p()
    assert lib.codae_create(C.byref(spec), C.byref(h)) == 0
    try:
        room = (C.c_float * 64)()
        base = C.addressof(room)
        avg = C.c_void_p(base + (-base) % 16)
        fake = C.c_void_p(4096)             # never dereferenced: the refusal comes first
        bufs = hip.Buffers(fake, fake, fake, fake, None, fake, fake, None, fake, None, fake)
        hyper = hip.Hyper(1e-3, 0.0, 0.9, 0.999, 1e-8, 0.0, 1, 0.0)
        span = lambda: lib.codae_step_update_span(h, C.byref(bufs), C.byref(hyper), 0, 4, None, None)
        S = hip.WeightAverage
        assert lib.codae_set_weight_average(h, C.byref(S(hip.AVG_EMA, 0.9, 1, 1, 1, avg))) == 0
        assert span() == -3 and b"weight average" in lib.codae_last_error()
        refused = {
            "unknown kind": (S(7, 0.9, 0, 1, 1, avg), b"kind"),
            "decay 1": (S(hip.AVG_EMA, 1.0, 0, 1, 1, avg), b"decay"),
            "decay < 0": (S(hip.AVG_EMA, -0.5, 0, 1, 1, avg), b"decay"),
            "decay NaN": (S(hip.AVG_EMA, float("nan"), 0, 1, 1, avg), b"decay"),
            "debias 2": (S(hip.AVG_EMA, 0.9, 2, 1, 1, avg), b"debias"),
            "start 0": (S(hip.AVG_SWA, 0.0, 0, 0, 1, avg), b"start"),
            "every 0": (S(hip.AVG_SWA, 0.0, 0, 1, 0, avg), b"every"),
            "no avg": (S(hip.AVG_SWA, 0.0, 0, 1, 1, None), b"avg"),
            "misaligned avg": (S(hip.AVG_SWA, 0.0, 0, 1, 1, C.c_void_p(avg.value + 4)), b"avg"),
        }
        for name, (st, word) in refused.items():
            assert lib.codae_set_weight_average(h, C.byref(st)) == -1, name
            assert word in lib.codae_last_error(), (name, lib.codae_last_error())
            assert span() == -3, "%s: the refused setting switched the previous one off" % name
        # fields the kind does not read are ignored: SWA with a decay out of range is accepted
        assert lib.codae_set_weight_average(h, C.byref(S(hip.AVG_SWA, 5.0, 9, 2, 3, avg))) == 0
        assert span() == -3
    finally:
        assert lib.codae_destroy(h) == 0


def test_trainer_tool_and_documents_name_the_feature():
    import inspect
    from codae import tool
    from codae.train import DataParallel, HipEmbeddingTrainer
    assert tool.WeightAverage is tool.average.WeightAverage and "weight_average_from_config" in tool.__all__
    sig = inspect.signature(HipEmbeddingTrainer.__init__).parameters
    assert sig["weight_average"].default is None
    for fn, arg, default in ((HipEmbeddingTrainer.eval_batch, "weights", "live"), (HipEmbeddingTrainer.complete, "weights", "live"),
                             (HipEmbeddingTrainer.params, "average", False)):
        assert inspect.signature(fn).parameters[arg].default == default, fn
    for name in ("set_weight_average", "average_params", "load_average", "reset_average"):
        assert callable(getattr(HipEmbeddingTrainer, name)), name
    assert callable(DataParallel._refuse_sharded_average)
    for doc, words in (("README.md", ("Weight averaging", "WEIGHT_AVERAGE")), ("DESIGN.md", ("Weight average", "weight_average_ab.log")),
                       ("INTEGRATION.md", ("codae_set_weight_average", "codae_weight_average_update"))):
        text = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in text, (doc, w)
