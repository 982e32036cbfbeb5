"""The layer-wise trust-ratio kinds (LAMB, LARS) on the host: the bounds of tests/trust_ref.py measured against its fp32
emulation on planted state (as tests/test_optimizer_host.py does for the kinds before them), codae.tool.Optimizer.step() on host
tensors against that emulation, the config round trip, and every refusal that needs no GPU.
"""
import types

import numpy as np
import pytest

import adam_ref as AR
import trust_ref as TR

torch = pytest.importorskip("torch")

HY = dict(lr=1e-3, wd=1e-2, betas=(0.9, 0.999), eps=1e-8)
COSINE = dict(sched="cosine", warmup=100, total=10000, min_factor=0.01)
CASES = {
    "lamb": dict(kind="lamb"),
    "lamb-decay-bias": dict(kind="lamb", decay_bias=True),
    "lars": dict(kind="lars", momentum=0.9),
    "lars-nesterov": dict(kind="lars", momentum=0.9, nesterov=True, trust_coef=0.02),
}
SIZES = (1, 5, 64, 1000, 4099)


def tool_of(case, trust_clip=0.0):
    from codae.tool import LRSchedule, Optimizer
    kw = dict(CASES[case])
    kind = kw.pop("kind")
    return Optimizer(kind, schedule=LRSchedule("cosine", warmup=100, total=10000, min_factor=0.01), trust_clip=trust_clip, **kw)


def hyper_struct(h):
    return types.SimpleNamespace(lr=h.lr, weight_decay=h.wd, beta1=h.b1, beta2=h.b2, eps=h.eps, step=h.t)


def clipped_below(tr, s, h, coef):
    """The setting with trust_clip at half the tensor's own ratio (an fp32 value)."""
    own = TR.step64(s["p"], s["g"], s["m"], s["v"], h, tr, coef)["ratio"]
    return tr._replace(trust_clip=AR._w(0.5 * own))


@pytest.mark.parametrize("matrix", (True, False), ids=("matrix", "bias"))
@pytest.mark.parametrize("t", (1, 1000))
@pytest.mark.parametrize("case", sorted(CASES))
def test_the_emulation_stays_within_three_quarters_of_the_bounds(case, t, matrix):
    worst = {}
    for n in SIZES:
        s = AR.planted_state([(n,)], 4100 + n, t == 1, HY["wd"])[0]
        h = AR.hyper(HY["lr"], HY["wd"], HY["betas"], HY["eps"], t)
        base = TR.trust(**CASES[case], **COSINE)
        for coef in (1.0, 0.01):
            for tr in (base, clipped_below(base, s, h, coef)) if matrix else (base,):
                args = (s["p"], s["g"], s["m"], s["v"], h, tr, np.float32(coef), matrix)
                want, tol, got = TR.step64(*args), TR.bounds(*args), TR.step32_emulated(*args)
                if not matrix:
                    assert want["ratio"] == 1.0 and got["ratio"] == 1.0 and tol["ratio"] == 0.0
                if tr.trust_clip > 0:
                    assert want["ratio"] == tr.trust_clip == float(got["ratio"]), (case, n, want["ratio"], got["ratio"])
                for k, r in TR.worst_ratios(got, want, tol).items():
                    worst[k] = max(worst.get(k, 0.0), r)
    print("MEASURE trust host %s t %d %s: worst |emulation - float64| / bound  %s" % (
        case, t, "matrix" if matrix else "bias", "  ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    for k, r in worst.items():
        assert r <= 0.75, "%s t %d: %s reaches %.3f of its bound" % (case, t, k, r)


def test_the_bias_block_decays_only_when_asked():
    s = AR.planted_state([(257,)], 77, False, HY["wd"])[0]
    h = AR.hyper(HY["lr"], HY["wd"], HY["betas"], HY["eps"], 9)
    for kind in ("lamb", "lars"):
        kw = dict(kind=kind, momentum=0.5 if kind == "lars" else 0.0)
        off = TR.step64(s["p"], s["g"], s["m"], s["v"], h, TR.trust(**kw), 1.0, matrix=False)
        no_wd = TR.step64(s["p"], s["g"], s["m"], s["v"], h._replace(wd=0.0), TR.trust(**kw), 1.0, matrix=False)
        on = TR.step64(s["p"], s["g"], s["m"], s["v"], h, TR.trust(decay_bias=True, **kw), 1.0, matrix=False)
        assert np.array_equal(off["p"], no_wd["p"]) and not np.array_equal(on["p"], off["p"])


@pytest.mark.parametrize("matrix", (True, False), ids=("matrix", "bias"))
@pytest.mark.parametrize("case", sorted(CASES))
def test_optimizer_step_on_host_tensors_is_the_emulation(case, matrix):
    for n, t, coef in ((1, 1, 1.0), (5, 1000, 0.25), (1000, 1, 0.01), (4099, 1000, 1.0)):
        s = AR.planted_state([(n,)], 5200 + n, t == 1, HY["wd"])[0]
        h = AR.hyper(HY["lr"], HY["wd"], HY["betas"], HY["eps"], t)
        for clip in (False, True) if matrix else (False,):
            tr = TR.trust(**CASES[case], **COSINE)
            if clip:
                tr = clipped_below(tr, s, h, coef)
            tool = tool_of(case, tr.trust_clip)
            assert TR.trust_of(tool) == tr
            want = TR.step32_emulated(s["p"], s["g"], s["m"], s["v"], h, tr, np.float32(coef), matrix)
            p, g = torch.from_numpy(s["p"].copy()), torch.from_numpy(s["g"].copy())
            state = {"m": torch.from_numpy(s["m"].copy()), "v": torch.from_numpy(s["v"].copy())}
            out = tool.step(p, g, state, hyper_struct(h), coef=coef, matrix=matrix)
            what = "%s n %d t %d coef %g clip %s" % (case, n, t, coef, clip)
            assert out is p and np.float32(state["ratio"]) == want["ratio"], (what, state["ratio"], want["ratio"])
            assert np.array_equal(p.numpy().view(np.uint32), want["p"].view(np.uint32)), what
            assert np.array_equal(state["m"].numpy().view(np.uint32), want["m"].view(np.uint32)), what
            if tr.kind == "lamb":
                assert np.array_equal(state["v"].numpy().view(np.uint32), want["v"].view(np.uint32)), what
            else:
                assert np.array_equal(state["v"].numpy().view(np.uint32), s["v"].view(np.uint32)), what + ": v moved under lars"
            assert np.array_equal(g.numpy().view(np.uint32), s["g"].view(np.uint32)), what


def test_edge_ratios_of_the_restatement_and_of_step():
    h = AR.hyper(HY["lr"], 0.0, HY["betas"], HY["eps"], 3)
    z = np.zeros(33, dtype=np.float32)
    p = np.linspace(-2, 2, 33).astype(np.float32)
    for case in ("lamb", "lars"):
        tr = TR.trust(**CASES[case])
        # an all-zero matrix: ratio 1
        assert TR.step32_emulated(z, z, z, z, h, tr, 1.0)["ratio"] == 1.0
        # g = 0, m = 0, wd = 0: ratio 1 and p bit for bit
        out = TR.step32_emulated(p, z, z, np.abs(p), h, tr, 1.0)
        assert out["ratio"] == 1.0 and np.array_equal(out["p"].view(np.uint32), p.view(np.uint32))
        t = torch.from_numpy(p.copy())
        st = {"m": torch.zeros(33), "v": torch.from_numpy(np.abs(p))}
        tool_of(case).step(t, torch.zeros(33), st, hyper_struct(h))
        assert st["ratio"] == 1.0 and np.array_equal(t.numpy().view(np.uint32), p.view(np.uint32))
        # a NaN gradient element without clipping: a NaN norm, ratio 1, the NaN stays where it is
        g = np.full(33, 0.5, dtype=np.float32)
        g[7] = np.nan
        out = TR.step32_emulated(p, g, z, z, h, tr, 1.0)
        assert out["ratio"] == 1.0 and np.isnan(out["p"][7]) and np.isfinite(np.delete(out["p"], 7)).all()


def test_config_round_trip_repr_and_struct():
    from codae import hip
    from codae.tool import LRSchedule, Optimizer
    from codae.tool.optimizer import KINDS, optimizer_from_config
    assert KINDS["lamb"] == hip.OPT_LAMB == 3 and KINDS["lars"] == hip.OPT_LARS == 4
    for o in (Optimizer("lamb", trust_clip=10.0, decay_bias=True, schedule=LRSchedule("cosine", warmup=5, total=50)),
              Optimizer("lars", momentum=0.9, nesterov=True, trust_coef=0.02, trust_clip=2.5),
              Optimizer("LAMB")):
        again = optimizer_from_config(o.as_config())
        assert again.as_config() == o.as_config() and TR.trust_of(again) == TR.trust_of(o) and repr(again) == repr(o)
        assert o.is_trust and not o.is_default and o.kind in repr(o) and "trust_clip" in repr(o)
        st = o.as_struct(None, 1 << 20)
        assert (st.kind, st.trust_ws, st.decay_bias) == (KINDS[o.kind], 1 << 20, int(o.decay_bias))
        assert np.float32(st.trust_clip) == np.float32(o.trust_clip) and np.float32(st.trust_coef) == np.float32(o.trust_coef)
    o = optimizer_from_config({"KIND": "lars", "MOMENTUM": 0.9, "TRUST_COEF": 0.001, "TRUST_CLIP": 0.0, "DECAY_BIAS": False})
    assert (o.kind, o.momentum, o.trust_coef) == ("lars", AR._w(0.9), AR._w(0.001))
    # the kinds before keep their block and their struct: nothing of the new fields shows
    old = Optimizer("adamw")
    assert set(old.as_config()) == {"KIND", "AMSGRAD", "MOMENTUM", "NESTEROV", "SCHEDULE"} and not old.is_trust
    st = old.as_struct(None)
    assert (st.trust_clip, st.trust_coef, st.decay_bias, st.trust_ws) == (0.0, 0.0, 0, None)
    import ctypes as C
    assert C.sizeof(hip.Optimizer) == 72 and hip.Optimizer.trust_ws.offset == 64 and hip.Optimizer.vmax.offset == 40


def test_refusals_on_the_host():
    from codae.hip import HipError
    from codae.tool import Optimizer
    from codae.tool.optimizer import optimizer_from_config
    for kind in ("lamb", "lars"):
        with pytest.raises(HipError, match="amsgrad"):
            Optimizer(kind, amsgrad=True, momentum=0.5)
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(HipError, match="trust_clip"):
                Optimizer(kind, momentum=0.5, trust_clip=bad)
        with pytest.raises(HipError, match="decay_bias"):
            Optimizer(kind, momentum=0.5, decay_bias=1)
    for bad in (0.0, -1e-3, float("nan"), float("inf")):
        with pytest.raises(HipError, match="trust_coef"):
            Optimizer("lars", momentum=0.9, trust_coef=bad)
    with pytest.raises(HipError, match="nesterov"):
        Optimizer("lars", nesterov=True)
    with pytest.raises(HipError, match="TRUST_RATIO"):
        optimizer_from_config({"KIND": "lamb", "TRUST_RATIO": 1.0})


def test_the_library_refuses_what_the_header_says(tmp_path):
    """check_optimizer through codae_trust_update: the checks run before anything is launched, so no GPU is needed."""
    import ctypes as C
    from codae import hip
    lib = hip.lib()
    hp = hip.Hyper(1e-3, 1e-2, 0.9, 0.999, 1e-8, 0.0, 1, 0.0)
    S = hip.Optimizer
    fake = C.c_void_p(1 << 20)           # never dereferenced: every call below is refused by its argument checks

    def st(kind, ams=0, mu=0.0, clip=0.0, coef=1e-3, decay=0):
        s = S(kind, ams, mu, 0, 0, 0, 0, 1, 0.0, 1.0, None)
        s.trust_clip, s.trust_coef, s.decay_bias = clip, coef, decay
        return s

    def call(s, n=64, ws=fake, ws_bytes=1 << 16):
        return lib.codae_trust_update(fake, fake, fake, fake, n, C.byref(hp), C.byref(s), fake, ws, ws_bytes, None)
    refused = {"amsgrad with lamb": st(3, ams=1), "amsgrad with lars": st(4, ams=1), "trust_clip < 0": st(3, clip=-1.0),
               "trust_clip NaN": st(3, clip=float("nan")), "trust_clip inf": st(4, clip=float("inf")), "trust_coef 0": st(4, coef=0.0),
               "trust_coef < 0": st(4, coef=-1.0), "trust_coef NaN": st(4, coef=float("nan")), "decay_bias 2": st(3, decay=2),
               "another kind": st(1)}
    for name, s in refused.items():
        assert call(s) == -1, name                                   # CODAE_E_INVALID
    assert call(st(3), ws=None) == -1 and call(st(3), ws=C.c_void_p((1 << 20) + 4)) == -1
    assert call(st(3), n=4097, ws_bytes=256 + 16) == -1              # two partial pairs needed
    assert lib.codae_trust_ws_bytes_flat(4096) == 256 + 16 and lib.codae_trust_ws_bytes_flat(4097) == 256 + 32
    assert lib.codae_trust_ws_bytes(None) == 0
    # the entry without a work space refuses the two kinds
    assert lib.codae_optimizer_update(fake, fake, fake, fake, None, 64, C.byref(hp), C.byref(st(3)), fake, None) == -1


def test_sharded_data_parallel_refuses_a_trust_kind():
    """DataParallel(sharded=True) around an engine whose optimizer is lamb / lars: HipError when it is built and at the next step
    when the kind is set afterwards (no GPU, no process group needed: the refusal comes first)."""
    from codae.hip import HipError
    from codae.tool import Optimizer
    from codae.train import DataParallel

    class Eng:
        L, tied_weights = 2, False
        w_off, b_off, n_param = [0, 64], [128], 256
        optimizer = None

    for kind, kw in (("lamb", {}), ("lars", dict(momentum=0.9))):
        eng = Eng()
        eng.optimizer = Optimizer(kind, **kw)
        with pytest.raises(HipError, match="%s: the sharded update is not supported: a matrix's norm spans shards" % kind):
            DataParallel(eng, n_buckets=2, sharded=True)
        assert not DataParallel(eng, n_buckets=2, sharded=False).sharded
        # set behind an existing sharded object: refused before the step does anything
        eng = Eng()
        dp = DataParallel(eng, n_buckets=2, sharded=True)
        with pytest.raises(HipError, match="norm spans shards"):
            dp._refuse_sharded_trust(Optimizer(kind, **kw))
        eng.optimizer = Optimizer(kind, **kw)
        with pytest.raises(HipError, match="norm spans shards"):
            dp.train_step(None, None, 0)
    eng = Eng()
    eng.optimizer = Optimizer("adamw")
    assert DataParallel(eng, n_buckets=2, sharded=True).sharded
