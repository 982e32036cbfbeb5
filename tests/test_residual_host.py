"""CPU-only tests of residual connections (include/codae_hip.h, "Residual connections"): which layers codae.tool.Residual accepts
and how a refusal names the layer, config parsing, its torch forward against a hand-written case and against the float64
statement of tests/residual_ref.py (values and autograd), the checkpoint's record of the skipped layers, the header / binding
agreement, and - through codae_debug_step_plan, on an engine created without a device - the step plan with a skip set and cleared."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import residual_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RELU = (1, 0.0, 0.0, 0.0)
NONE = (0, 0.0, 0.0, 0.0)


def square(L, io=1536):
    """the benchmark's square stack: ReLU behind every layer but the code layer and the last"""
    nb_in, nb_out = (L - 1) // 2, (L - 2) // 2
    relu = [True] * nb_in + [False] + [True] * nb_out + [False]
    return [io] * L, [io] * L, relu


def test_hidden_on_the_headline_stack_is_layers_1_to_8():
    from codae.tool import Residual
    ins, outs, relu = square(10)
    flags = Residual("hidden").resolve(ins, outs, relu)
    assert [l for l, f in enumerate(flags) if f] == [1, 2, 3, 4, 5, 6, 7, 8]
    # C5: 6 x 1024
    ins, outs, relu = square(6, 1024)
    assert Residual().resolve(ins, outs, relu) == [0, 1, 1, 1, 1, 0]
    # "hidden" passes over what cannot take a skip instead of refusing it: the narrowing and the widening layer, an ELU layer
    acts = [RELU, RELU, (4, 1.0, 1.0, 1.0), NONE, RELU, NONE]
    assert Residual("hidden").resolve([48, 48, 48, 48, 16, 48], [48, 48, 48, 16, 48, 48], acts) == [0, 1, 0, 0, 0, 0]
    assert repr(Residual("hidden")) == "Residual('hidden')" and repr(Residual([2, 1])) == "Residual([1, 2])"
    assert Residual([]).is_off and not Residual("hidden").is_off


def test_refusals_name_the_layer_and_the_reason():
    from codae.hip import HipError
    from codae.tool import Residual
    ins, outs = [48, 48, 16, 48], [48, 16, 48, 48]
    acts = [RELU, NONE, RELU, NONE]
    assert Residual([0]).resolve(ins, outs, acts) == [1, 0, 0, 0]              # layer 0 may be listed when it is square
    with pytest.raises(HipError, match=r"layer 1: .*equal widths \(48 -> 16\)"):
        Residual([0, 1]).resolve(ins, outs, acts)
    with pytest.raises(HipError, match=r"layer 3: the last layer"):
        Residual([3]).resolve(ins, outs, acts)
    with pytest.raises(HipError, match=r"layer 4: the stack has 4 layers"):
        Residual([4]).resolve(ins, outs, acts)
    elu = [RELU, (4, 1.0, 1.0, 1.0), NONE]
    with pytest.raises(HipError, match=r"layer 1: .*none, ReLU or LeakyReLU \(got ELU\)"):
        Residual([1]).resolve([24, 24, 24], [24, 24, 24], elu)
    assert Residual([1]).resolve([24, 24, 24], [24, 24, 24], [RELU, (2, 0.1, 0.0, 0.0), NONE]) == [0, 1, 0]
    for bad in ("all", 3, [1, 1], [-1], [True], [1.5]):
        with pytest.raises(HipError):
            Residual(bad)


def test_config_block():
    from codae.hip import HipError
    from codae.tool import residual_from_config
    assert residual_from_config(None) is None and residual_from_config({}) is None
    assert residual_from_config({"LAYERS": "hidden"}).layers == "hidden"
    assert residual_from_config({"LAYERS": [2, 1]}).layers == (1, 2)
    with pytest.raises(HipError, match="unknown key.*LAYER"):
        residual_from_config({"LAYERS": "hidden", "LAYER": 1})
    with pytest.raises(HipError, match="unknown key.*SKIP"):
        residual_from_config({"SKIP": 1})
    with pytest.raises(HipError, match="mapping"):
        residual_from_config("hidden")
    with pytest.raises(HipError, match="hidden"):
        residual_from_config({"LAYERS": "every"})


def test_forward_against_a_hand_written_two_layer_case():
    from codae.tool import Residual
    x = torch.tensor([[1.0, -2.0], [0.5, 3.0]], dtype=torch.float64)
    W0 = torch.tensor([[1.0, 1.0], [-1.0, 0.0]], dtype=torch.float64)
    b0 = torch.tensor([0.5, 0.25], dtype=torch.float64)
    W1 = torch.tensor([[2.0, 0.0], [0.0, -1.0]], dtype=torch.float64)
    b1 = torch.tensor([0.0, 1.0], dtype=torch.float64)
    # row 0: z0 = (-0.5, -0.75) -> relu (0, 0) -> + x = (1, -2) -> y = (2, 3)
    # row 1: z0 = (4, -0.25) -> relu (4, 0) -> + x = (4.5, 3) -> y = (9, -2)
    y = Residual([0]).forward(x, [W0, W1], [b0, b1], [True, False])
    assert torch.equal(y, torch.tensor([[2.0, 3.0], [9.0, -2.0]], dtype=torch.float64))
    # without the skip: relu (0, 0) -> (0, 1); (4, 0) -> (8, 1)
    y = Residual([]).forward(x, [W0, W1], [b0, b1], [True, False])
    assert torch.equal(y, torch.tensor([[0.0, 1.0], [8.0, 1.0]], dtype=torch.float64))
    # a dropout factor multiplies a_0 before the skip is added: row 1, (4 * 2, 0) + x = (8.5, 3) -> (17, -2)
    f = torch.tensor([[2.0, 2.0], [2.0, 0.0]], dtype=torch.float64)
    y = Residual([0]).forward(x, [W0, W1], [b0, b1], [True, False], dropout_factors=[f])
    assert torch.equal(y, torch.tensor([[2.0, 3.0], [17.0, -2.0]], dtype=torch.float64))


@pytest.mark.parametrize("acts,names", [([True, True, False, True, False], ["relu", "relu", None, "relu", None]),
                                        ([(2, 0.1, 0, 0), (2, 0.1, 0, 0), NONE, (2, 0.1, 0, 0), NONE], [("leaky", 0.1)] * 2 + [None, ("leaky", 0.1), None])],
                         ids=["relu", "leaky"])
def test_forward_and_its_autograd_match_the_float64_statement(acts, names):
    from codae.tool import Residual
    rng = np.random.default_rng(5)
    L, w, B = 5, 12, 9
    params = [(rng.standard_normal((w, w)).astype(np.float32) * 0.4, rng.standard_normal(w).astype(np.float32) * 0.1) for _ in range(L)]
    c = rng.standard_normal((B, w)).astype(np.float32)
    x = rng.standard_normal((B, w)).astype(np.float32)
    factors = [None, np.where(rng.random((B, w)) < 0.5, 0.0, 2.0).astype(np.float32), None, None]
    for layers in ([1, 2, 3], [1], [0, 2]):
        skips = [1 if l in layers else 0 for l in range(L)]
        grads, loss, y = RR.gradients(params, names, skips, c, RR.mse(x), factors)
        Ws = [torch.tensor(p[0].astype(np.float64), requires_grad=True) for p in params]
        bs = [torch.tensor(p[1].astype(np.float64), requires_grad=True) for p in params]
        yt = Residual(layers).forward(torch.tensor(c.astype(np.float64)), Ws, bs, acts,
                                      dropout_factors=[None if f is None else torch.tensor(f.astype(np.float64)) for f in factors])
        assert np.allclose(yt.detach().numpy(), y, rtol=1e-12, atol=1e-12)
        lt = ((yt - torch.tensor(x.astype(np.float64))) ** 2).sum() / x.size
        assert abs(float(lt.detach()) - loss) <= 1e-12 * abs(loss)
        lt.backward()
        for l in range(L):
            assert np.allclose(Ws[l].grad.numpy(), grads[l][0], rtol=1e-10, atol=1e-13), (layers, "dW", l)
            assert np.allclose(bs[l].grad.numpy(), grads[l][1], rtol=1e-10, atol=1e-13), (layers, "db", l)
    # the skips change the function
    y_off = RR.forward(params, names, [0] * L, c)[0]
    assert np.abs(y_off - y).max() > 1e-3


def test_reference_finite_difference_and_bf16_variant():
    """the hand-written backward of tests/residual_ref.py against a central difference of its own forward; its bf16 variant stays
    within bf16's grid of the float64 one and packs the mask bits in the forward GEMM's order"""
    rng = np.random.default_rng(6)
    L, w, B = 4, 8, 5
    params = [(rng.standard_normal((w, w)).astype(np.float32) * 0.5, rng.standard_normal(w).astype(np.float32) * 0.1) for _ in range(L)]
    names = [("leaky", 0.2), ("leaky", 0.2), ("leaky", 0.2), None]
    skips = [0, 1, 1, 0]
    c = rng.standard_normal((B, w)).astype(np.float32)
    x = rng.standard_normal((B, w)).astype(np.float32)
    grads, loss, _ = RR.gradients(params, names, skips, c, RR.mse(x))
    for l, i, j in ((0, 1, 2), (1, 0, 0), (2, 3, 5), (3, 7, 7)):
        eps = 1e-3                                               # (exact in fp32: the statement reads fp32 parameters)
        vals = []
        for sgn in (1, -1):
            p2 = [(W.copy(), b.copy()) for W, b in params]
            p2[l][0][i, j] = np.float32(p2[l][0][i, j] + sgn * eps)
            vals.append((RR.gradients(p2, names, skips, c, RR.mse(x))[1], float(p2[l][0][i, j])))
        fd = (vals[0][0] - vals[1][0]) / (vals[0][1] - vals[1][1])
        assert abs(fd - grads[l][0][i, j]) <= 2e-4 * max(1.0, abs(fd)), (l, fd, grads[l][0][i, j])
    gb, lb, _ = RR.gradients(params, names, skips, c, RR.mse(x), bf16=True)
    assert abs(lb - loss) <= 0.05 * loss
    for l in range(L):
        assert np.linalg.norm(gb[l][0] - grads[l][0]) <= 0.05 * np.linalg.norm(grads[l][0])
    a = np.array([[1.0, -1.0, 0.0, -0.0, 2.0, np.nan, -np.nan, 3.0, 5.0]], dtype=np.float32)
    a[0, 5] = np.uint32(0x7FC00000).view(np.float32)
    a[0, 6] = np.uint32(0xFFC00000).view(np.float32)
    assert RR.packed_mask(a).tolist() == [[0b10110001, 0b00000001]]


def test_checkpoint_meta_round_trip_and_mismatch():
    import json
    from codae.tool.residual import Residual, meta_mismatch
    meta = json.loads(json.dumps({"schedule": [[24, 24, True]] * 4, "residual": [1, 2]}))
    assert meta_mismatch(meta, [1, 2]) is None and meta_mismatch(meta, (2, 1)) is None
    assert Residual(meta["residual"]).layers == (1, 2)
    why = meta_mismatch(meta, [])
    assert "residual" in why and "[1, 2]" in why and "none" in why
    assert "[1]" in meta_mismatch(meta, [1])
    # a file written before the key existed has no skips: it loads into a trainer without them, and only into such a one
    old = {"schedule": [[24, 24, True]] * 4}
    assert meta_mismatch(old, []) is None and meta_mismatch({"residual": None}, None) is None
    assert "none" in meta_mismatch(old, [2]) and "[2]" in meta_mismatch(old, [2])
    # the trainer's own structure check and record, on a stand-in for the engine (no device): _state_meta writes the skipped layers,
    # _check_structure accepts its own record and refuses every other set of skips, naming the piece
    import types
    from codae.hip import HipError
    from codae.train import HipEmbeddingTrainer

    def trainer(layers):
        eng = types.SimpleNamespace(
            schedule=[(24, 24, True)] * 3 + [(24, 24, False)], step_count=2, n_param=2400, precision=0, activation=None, tied_weights=False,
            residual_layers=list(layers), optimizer=None, weight_average=None, adam_vmax=None, weight_avg=None, input_noise=None,
            loss_emphasis=None, hidden_dropout=None, recon_loss=None, slot_contrast=None, slot_presence=None,
            state_tensors=lambda: {}, averaging=lambda: False)
        t = HipEmbeddingTrainer.__new__(HipEmbeddingTrainer)
        t.engine, t.lr, t.weight_decay, t.clip = eng, 1e-3, 1e-4, 1.0
        return t
    written = json.loads(json.dumps(trainer([1, 2])._state_meta()))
    assert written["residual"] == [1, 2] and json.loads(json.dumps(trainer([])._state_meta()))["residual"] is None
    trainer([2, 1])._check_structure("ck", {}, written, False, need=())
    for other in ([], [1], [1, 2, 0]):
        with pytest.raises(HipError, match=r"load\(ck\): residual: .*\[1, 2\]"):
            trainer(other)._check_structure("ck", {}, written, False, need=())
    no_key = {k: v for k, v in written.items() if k != "residual"}
    trainer([])._check_structure("ck", {}, no_key, False, need=())
    with pytest.raises(HipError, match="residual"):
        trainer([1])._check_structure("ck", {}, no_key, False, need=())


def test_header_constants_agree_with_the_binding():
    from codae import hip
    header = open(os.path.join(ROOT, "include", "codae_hip.h")).read()
    K = {k: int(v) for k, v in re.findall(r"\b(CODAE_K_[A-Z0-9_]+)\s*=\s*(\d+)", header)}
    assert K["CODAE_K_COUNT"] == 11 == len(hip.KERNEL_CLASSES) and K["CODAE_K_DROPOUT"] == 10
    assert int(re.search(r"#define CODAE_ABI_VERSION (\d+)", header).group(1)) == 11 == hip.ABI_VERSION
    for fn in ("codae_set_residual", "codae_residual_ws_bytes", "codae_residual_fwd", "codae_residual_bwd", "codae_residual_blocks"):
        assert fn in hip.PROTOTYPES and fn + "(" in header
    assert "Residual connections" in header
    assert [n for n, _ in hip.ResidualFlags._fields_] == ["n", "on"] and C.sizeof(hip.ResidualFlags) == 16
    lib = hip.lib()
    assert lib.codae_abi_version() == 11
    assert [lib.codae_residual_blocks(b) for b in (0, 1, 64, 65, 130, 8192)] == [0, 1, 1, 2, 3, 128]
    makefile = open(os.path.join(ROOT, "mui-deepautoencoder_amd", "csrc", "Makefile")).read()
    assert "residual.hip" in re.search(r"^SRCS := (.*)$", makefile, re.M).group(1).split()


# ---- the step plan and the setter, on an engine created without a device -------------------------------------------------------

N_FIELDS = 10             # CODAE_STEP_PLAN_FIELDS
PATH = 1                  # index of `path`; 1 = the persistent chain, 0 = the per-layer launches
TRAIN_96 = (0, 96, 0, 0, 1, 0, 0, 1)


class Engine:
    """codae_create and the setters used here make no HIP call (tests/test_step_plan_host.py)."""

    def __init__(self, io, L, prec="bf16", acts=None, widths=None, max_batch=96):
        from codae import hip
        self.hip, self.lib, self.L = hip, hip.lib(), L
        ins = widths[:-1] if widths else [io] * L
        outs = widths[1:] if widths else [io] * L
        nb_in, nb_out = (L - 1) // 2, (L - 2) // 2
        relu = [1] * nb_in + [0] + [1] * nb_out + [0]
        self.keep = [(C.c_int32 * L)(*ins), (C.c_int32 * L)(*outs), (C.c_uint8 * L)(*relu)]
        spec = hip.Spec(L, self.keep[0], self.keep[1], self.keep[2], max_batch, hip.PREC_BF16 if prec == "bf16" else hip.PREC_F32)
        if acts is not None:
            self.keep += [(C.c_uint8 * L)(*[a[0] for a in acts]), (C.c_float * (3 * L))(*[float(v) for a in acts for v in a[1:]])]
            spec.act_kind, spec.act_param = self.keep[-2], self.keep[-1]
        self.h = C.c_void_p()
        assert self.lib.codae_create(C.byref(spec), C.byref(self.h)) == 0, self.lib.codae_last_error()
        some = C.cast((C.c_char * 64)(), C.c_void_p)
        self.keep.append(some)
        self.bufs = hip.Buffers(some, some, some, some, some, some, some, some, some, some if prec == "bf16" else None, some)

    def flags(self, layers):
        arr = (C.c_uint8 * self.L)(*[1 if l in layers else 0 for l in range(self.L)])
        self.keep.append(arr)
        return self.hip.ResidualFlags(self.L, arr)

    def set(self, layers, ws_bytes=None):
        """-> (rc, needed bytes); the work space is host memory nobody reads through"""
        st = self.flags(layers)
        need = int(self.lib.codae_residual_ws_bytes(self.h, C.byref(st)))
        if need < 0:
            return self.lib.codae_set_residual(self.h, C.byref(st), None, 0), need
        room = (C.c_char * (max(need, 16) + 16))()
        self.keep.append(room)
        ws = C.c_void_p((C.addressof(room) + 15) // 16 * 16)
        return self.lib.codae_set_residual(self.h, C.byref(st), ws, need if ws_bytes is None else ws_bytes), need

    def plan(self, call=TRAIN_96):
        out = (C.c_int32 * N_FIELDS)()
        assert self.lib.codae_debug_step_plan(self.h, C.byref(self.bufs), (C.c_int32 * 8)(*call), out, N_FIELDS) == 0, self.lib.codae_last_error()
        return list(out)

    def error(self):
        return self.lib.codae_last_error().decode()

    def close(self):
        self.lib.codae_destroy(self.h)


@pytest.fixture
def no_switches(monkeypatch):
    from codae import hip
    for k in list(os.environ):
        if k.startswith("CODAE_"):
            monkeypatch.delenv(k)
    hip.lib().codae_reload_env()
    yield
    hip.lib().codae_reload_env()


def test_a_skip_takes_the_narrow_stack_off_the_chain_and_clearing_it_restores_the_plan(no_switches):
    e = Engine(192, 3)
    try:
        before = e.plan()
        assert before[PATH] == 1                                  # 3 x 192 at 96 rows: the persistent chain kernel
        assert e.lib.codae_step_path(e.h, C.byref(e.bufs), 96) == 1
        rc, need = e.set([1])
        assert rc == 0, e.error()
        # G [96][192] fp32; layer 1 is the code layer (no activation): no mask
        assert need == 96 * 192 * 4
        with_skip = e.plan()
        assert with_skip[PATH] == 0 and e.lib.codae_step_path(e.h, C.byref(e.bufs), 96) == 0
        # what it has without the chain kernel today (tests/test_step_plan_host.py, "02-bf16-layers"): nothing else moves
        os.environ["CODAE_NO_CHAIN"] = "1"
        try:
            ref = Engine(192, 3)
            assert with_skip == ref.plan()
            ref.close()
        finally:
            del os.environ["CODAE_NO_CHAIN"]
            e.lib.codae_reload_env()
        # cleared three ways: the plan it has today, field for field
        for clear in (lambda: e.lib.codae_set_residual(e.h, None, None, 0), lambda: e.set([])[0]):
            assert e.set([1])[0] == 0 and e.plan()[PATH] == 0
            assert clear() == 0, e.error()
            assert e.plan() == before
        # an evaluation, a ranged backward and the update keep their plans with the skip on
        others = [(2, 96, 0, 0, 1, 0, 0, 0), (3, 96, 1, 3, 0, 0, 0, 0), (5, 0, 0, 0, 1, 0, 0, 1)]
        plain = [e.plan(c) for c in others]
        assert e.set([1])[0] == 0
        assert [e.plan(c) for c in others] == plain
    finally:
        e.close()


def test_the_setter_refuses_what_the_definition_excludes_and_keeps_the_previous_setting(no_switches):
    INVALID, UNSUPPORTED = -1, -3
    leaky = (2, 0.1, 0.0, 0.0)
    softplus = (5, 1.0, 20.0, 0.0)
    e = Engine(0, 5, "f32", acts=[leaky, softplus, NONE, leaky, NONE], widths=[24, 24, 24, 16, 16, 24])
    try:
        rc, need = e.set([0, 3])
        assert rc == 0, e.error()
        # G [96][24] fp32 = 9216, then a mask of ceil(24 / 8) = 3 and one of 2 bytes per row, each rounded up to 256 bytes
        assert need == 9216 + 512 + 256
        assert e.plan()[PATH] == 0
        for layers, code, words in (([1], UNSUPPORTED, ("layer 1", "none, ReLU or LeakyReLU")), ([2], UNSUPPORTED, ("layer 2", "equal widths", "24 -> 16")),
                                    ([4], UNSUPPORTED, ("layer 4", "last layer"))):
            rc, need = e.set(layers)
            assert (rc, need) == (code, -1), (layers, rc, need)
            for w in words:
                assert w in e.error(), (layers, e.error())
        st = e.flags([0])
        st.n = 4
        assert e.lib.codae_set_residual(e.h, C.byref(st), None, 0) == INVALID and "4 flags for 5 layers" in e.error()
        assert e.set([0], ws_bytes=64)[0] == INVALID and "work space" in e.error()
        st = e.flags([0])
        assert e.lib.codae_set_residual(e.h, C.byref(st), C.c_void_p(8), 1 << 20) == INVALID        # (misaligned; never read through)
        # all-zero flags need no work space at all
        st = e.flags([])
        assert e.lib.codae_residual_ws_bytes(e.h, C.byref(st)) == 0 and e.lib.codae_residual_ws_bytes(e.h, None) == 0
    finally:
        e.close()
