"""CPU-only tests of the slot contrast (include/codae_hip.h, "Slot contrast"): the float64 reference against a finite difference
of its own loss, codae.tool.SlotContrast.loss and its autograd gradient against the reference, the candidate sampling, validation
and config parsing, and the header / binding / INTEGRATION.md agreement."""
import os
import re

import numpy as np
import pytest
import torch

import contrast_ref as CR
import emphasis_ref as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EEDC0DE12345678
STEP = 5


def _case(io=24, S=3, dup=True):
    """emphasis_ref.problem(io) (N = 120, B = 33); dup: dataset rows 100 .. 104 repeat the slot-0 and slot-2 items of the first
    five batch rows, so that `distinct` leaves out candidates that the row rule keeps."""
    p = ER.problem(io)
    data = p["data"].copy()
    E = io // S
    if dup:
        for i in range(5):
            data[100 + i, 0:E] = data[p["rows"][i], 0:E]
            data[100 + i, 2 * E:3 * E] = data[p["rows"][i], 2 * E:3 * E]
    return p, data


def test_reference_gradient_is_the_finite_difference_of_its_loss_io24_k5():
    """Central differences in float64, h = 1e-6 |y|: rtol 1e-6 of the largest gradient (the loss is smooth: second-order error h^2)."""
    p, data = _case(24)
    rows, y = p["rows"][:6], p["y"][:6].astype(np.float64)
    x = data[rows]
    W = np.random.default_rng(1).uniform(0.5, 2.0, (6, 3))
    kw = dict(step=STEP, S=3, K=5, tau=0.5, scale=np.float32(1.0 / 18), seed=SEED, W=W)
    ref = CR.terms(data, x, y.astype(np.float32), rows, **kw)
    y32 = y.astype(np.float32).astype(np.float64)

    def loss(yy):
        return CR.loss_value(data, x, yy, rows, **kw)

    assert loss(y32) == ref["loss"]
    g = np.zeros_like(y32)
    for i in range(y32.shape[0]):
        for c in range(y32.shape[1]):
            h = 1e-6 * max(abs(y32[i, c]), 0.1)
            a, b = y32.copy(), y32.copy()
            a[i, c] += h
            b[i, c] -= h
            g[i, c] = (loss(a) - loss(b)) / (2 * h)
    err = np.abs(g - ref["dy"]).max()
    print("finite difference: worst error %.3e of largest gradient %.3e" % (err, np.abs(ref["dy"]).max()))
    assert err <= 1e-6 * np.abs(ref["dy"]).max()
    assert np.abs(ref["dy"]).max() > 1e-3


@pytest.mark.parametrize("distinct", [True, False], ids=["distinct", "rows"])
def test_loss_and_autograd_gradient_match_the_reference_b33_io24_k33(distinct):
    """fp32 torch on the host against the float64 reference: rtol 1e-5 of the largest gradient, 1e-5 relative on the loss."""
    from codae.tool import SlotContrast
    p, data = _case(24)
    rows, y = p["rows"], p["y"]
    x = data[rows]
    W = np.random.default_rng(2).uniform(0.5, 2.0, (33, 24)).astype(np.float32)
    Wm = W.astype(np.float64).reshape(33, 3, 8).mean(-1)
    c = SlotContrast(negatives=33, temperature=0.1, weight=0.7, seed=SEED, distinct=distinct)
    scale = np.float32(c.weight / (33 * 3))
    ids = CR.item_ids(data, 3) if distinct else None
    ref = CR.terms(data, x, y, rows, STEP, 3, 33, 0.1, scale, SEED, W=Wm, item_id=ids)
    left = ref["left_out"]
    assert left.any() and not left.all(axis=2).any()
    out = torch.tensor(y, requires_grad=True)
    loss = c.loss(torch.tensor(x), out, rows, STEP, torch.tensor(data), weight=torch.tensor(W), n_slots=3)
    loss.backward()
    print("loss", float(loss), ref["loss"])
    assert abs(float(loss) - ref["loss"]) <= 1e-5 * abs(ref["loss"])
    err = np.abs(out.grad.numpy() - ref["dy"]).max()
    assert err <= 1e-5 * np.abs(ref["dy"]).max(), err
    if distinct:      # the duplicated items make the two rules differ
        other = CR.terms(data, x, y, rows, STEP, 3, 33, 0.1, scale, SEED, W=Wm, item_id=None)
        assert (other["left_out"] != left).any() and abs(other["loss"] - ref["loss"]) > 1e-6 * ref["loss"]


def test_zero_target_and_all_left_out_give_nothing_io24():
    from codae.tool import SlotContrast
    p, data = _case(24, dup=False)
    data[:, 8:16] = 0.0                                   # slot 1 of every row: no positive anywhere
    rows, y = p["rows"], p["y"]
    ref = CR.terms(data, data[rows], y, rows, STEP, 3, 5, 0.1, 1.0, SEED)
    assert (ref["l"][:, 1] == 0).all() and (ref["dy"][:, 8:16] == 0).all() and (ref["l"][:, 0] > 0).all()
    c = SlotContrast(negatives=5, seed=SEED)
    out = torch.tensor(y, requires_grad=True)
    c.loss(torch.tensor(data[rows]), out, rows, STEP, torch.tensor(data), n_slots=3).backward()
    assert (out.grad[:, 8:16] == 0).all()
    # K = 1 and the only candidate is the row itself: l = 0, gradient 0
    one = CR.candidate_rows(STEP, 0, 1, SEED, 120)[0]
    r1 = CR.terms(data, data[[one]], y[:1], [one], STEP, 3, 1, 0.1, 1.0, SEED)
    assert r1["left_out"][0, 0, 0] and r1["l"][0, 0] == 0 and (r1["dy"][0, 0:8] == 0).all()


def test_candidate_rows_are_the_references_sampling():
    from codae.tool import SlotContrast
    pool = np.arange(7, 120, 3)
    for K in (1, 5, 33, 130, 4096):
        for step, slot in ((1, 0), (5, 2), (2 ** 31 + 3, 127)):
            c = SlotContrast(negatives=K, seed=SEED)
            assert (c.candidate_rows(step, slot, 120) == CR.candidate_rows(step, slot, K, SEED, 120)).all()
            cp = SlotContrast(negatives=K, seed=SEED, candidates=pool)
            got = cp.candidate_rows(step, slot, 120)
            assert (got == CR.candidate_rows(step, slot, K, SEED, 120, pool)).all() and np.isin(got, pool).all()
    a = SlotContrast(negatives=130, seed=SEED)
    assert (a.candidate_rows(1, 0, 120) != a.candidate_rows(2, 0, 120)).any()          # per step
    assert (a.candidate_rows(1, 0, 120) != a.candidate_rows(1, 1, 120)).any()          # per slot
    assert len(np.unique(a.candidate_rows(1, 0, 120))) < 130                          # with replacement
    assert a.candidate_rows(1, 0, 120).min() >= 0 and a.candidate_rows(1, 0, 120).max() < 120


def test_validation():
    from codae.hip import HipError
    from codae.tool import SlotContrast
    c = SlotContrast()
    assert (c.negatives, c.temperature, c.weight, c.seed, c.distinct) == (256, float(np.float32(0.1)), 1.0, 0, True) and not c.is_default
    assert SlotContrast(weight=0).is_default
    bad = [dict(negatives=0), dict(negatives=4097), dict(negatives=2.5), dict(negatives=True), dict(temperature=0.005),
           dict(temperature=float("nan")), dict(temperature=float("inf")), dict(temperature="0.1"), dict(weight=-0.5),
           dict(weight=float("nan")), dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.5), dict(distinct=1),
           dict(candidates=[]), dict(candidates=[-1, 2]), dict(candidates=[[1, 2]]), dict(candidates=[0.5])]
    for kw in bad:
        with pytest.raises(HipError):
            SlotContrast(**kw)
    with pytest.raises(HipError, match="outside"):
        SlotContrast(candidates=[0, 120]).candidate_rows(1, 0, 120)
    for n in (None, 0, 129, 2.5):
        with pytest.raises(HipError):
            c.as_struct(n, 120)
    x = torch.zeros(4, 6)
    with pytest.raises(HipError, match="divide"):
        c.loss(x, x, [0, 1, 2, 3], 1, torch.zeros(9, 6), n_slots=4)
    with pytest.raises(HipError, match="shape"):
        c.loss(x, x[:, :3], [0, 1, 2, 3], 1, torch.zeros(9, 6), n_slots=3)
    with pytest.raises(HipError, match="columns"):
        c.loss(x, x, [0, 1, 2, 3], 1, torch.zeros(9, 5), n_slots=3)
    with pytest.raises(HipError, match="at most"):
        c.loss(torch.zeros(2, 1025), torch.zeros(2, 1025), [0, 1], 1, torch.zeros(9, 1025), n_slots=1)


def test_as_struct_carries_the_header_fields():
    from codae.tool import SlotContrast
    st = SlotContrast(negatives=33, temperature=0.5, weight=0.25, seed=SEED).as_struct(3, 120)
    assert (st.n_slots, st.n_neg, st.tau, st.weight, st.seed, st.n_rows, st.n_pool, st.ws_bytes) == (3, 33, 0.5, 0.25, SEED, 120, 0, 0)
    assert st.pool is None and st.item_id is None and st.ws is None


def test_config_parser():
    from codae.hip import HipError
    from codae.tool.contrast import contrast_from_config
    assert contrast_from_config(None) is None and contrast_from_config({}) is None
    c = contrast_from_config({"NEGATIVES": 64, "TEMPERATURE": 0.2, "WEIGHT": 0.5, "SEED": 9, "DISTINCT": False})
    assert (c.negatives, c.temperature, c.weight, c.seed, c.distinct) == (64, float(np.float32(0.2)), 0.5, 9, False)
    assert contrast_from_config({"WEIGHT": 2.0}).negatives == 256
    for block in ({"NEGATIVES": 64, "TAU": 0.2}, "on", {"NEGATIVES": 0}, {"TEMPERATURE": 0.001}, {"CANDIDATES": [1]}):
        with pytest.raises(HipError):
            contrast_from_config(block)


def test_trainer_and_tool_export_the_contrast():
    import inspect
    import codae.tool
    from codae.hip.engine import DaeEngine
    from codae.train import HipEmbeddingTrainer
    assert "SlotContrast" in codae.tool.__all__
    assert inspect.signature(HipEmbeddingTrainer.__init__).parameters["contrast"].default is None
    assert callable(HipEmbeddingTrainer.set_contrast) and callable(DaeEngine.set_slot_contrast)


def test_header_binding_and_integration_doc_agree_on_the_new_names():
    import ctypes as C
    from codae import hip
    from codae.tool import contrast as T
    header = open(os.path.join(ROOT, "include", "codae_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert int(re.search(r"#define CODAE_ABI_VERSION (\d+)", header).group(1)) == 11 == hip.ABI_VERSION      # new entries only
    assert int(re.search(r"CODAE_K_COUNT = (\d+)", header).group(1)) == 11 == len(hip.KERNEL_CLASSES)
    assert len(re.findall(r"\bCODAE_LOSS_[A-Z0-9_]+\s*=", header)) == 5                                       # not a sixth kind
    assert "Slot contrast" in header
    body = re.search(r"typedef struct \{([^}]*)\} codae_slot_contrast;", header).group(1)
    fields = re.findall(r"^\s*(?:const\s+)?(int32_t\*|int32_t|int64_t|uint64_t|float|void\*)\s+(\w+);", body, flags=re.M)
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float, "int32_t*": C.c_void_p,
             "void*": C.c_void_p}
    assert [(n, ctype[t]) for t, n in fields] == list(hip.SlotContrast._fields_)
    assert len(fields) == 11
    for fn in ("codae_set_slot_contrast", "codae_slot_contrast_ws_bytes", "codae_slot_contrast_prepare", "codae_slot_contrast_fwd_bwd",
               "codae_slot_contrast_blocks"):
        assert re.search(r"\b%s\s*\(" % fn, header) and fn in hip.PROTOTYPES and fn in doc, fn
        assert hasattr(hip.lib(), fn), fn
    for word in ("codae_slot_contrast", "SlotContrast", "CONTRAST", "NEGATIVES", "TEMPERATURE"):
        assert word in doc, word
    for name in ("codae_slot_contrast_fwd_bwd", "codae_slot_contrast_prepare", "codae_slot_contrast_ws_bytes"):
        proto = re.search(r"\b%s\(([^;]*)\);" % name, header).group(1)
        assert len(proto.split(",")) == len(hip.PROTOTYPES[name][1]), name
    assert (T.MAX_NEG, T.MAX_SLOTS, T.MAX_E, T.COS_EPS) == (4096, 128, 1024, CR.EPS)
    # the work space grows with S, K and E alone
    lib = hip.lib()
    assert lib.codae_slot_contrast_ws_bytes(3, 33, 8, 1) == 2 * 3 * 64 * 32 * 2 + 3 * 64 * 4
    assert lib.codae_slot_contrast_ws_bytes(3, 33, 8, 0) == 2 * 3 * 64 * 32 * 4 + 3 * 64 * 4
    assert lib.codae_slot_contrast_ws_bytes(3, 4097, 8, 1) == -1 and lib.codae_slot_contrast_ws_bytes(3, 33, 1025, 1) == -1
    assert lib.codae_slot_contrast_blocks(33) == 2 and lib.codae_slot_contrast_blocks(1) == 1
