"""CPU-only tests of the training criterion (include/codae_hip.h, "Training criterion"): codae.tool.ReconstructionLoss validation
and config parsing, ReconstructionLoss.loss and its autograd gradient against tests/recon_loss_ref.py, the reference against
torch's own l1_loss / smooth_l1_loss / huber_loss / cosine_similarity, and the header / binding / INTEGRATION.md agreement."""
import os
import re

import numpy as np
import pytest
import torch

import emphasis_ref as ER
import recon_loss_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASKING = ("masking", dict(p=0.25), ER.SEED)
ALPHA, BETA, SLOT_W = 3.0, 0.5, (0.5, 1.0, 2.0)
IO, S = 48, 3
CASES = [("l1", {}), ("smooth_l1", dict(beta=0.5)), ("huber", dict(delta=0.75)), ("slot_cosine", {}), ("slot_cosine", dict(mse_weight=0.25))]
IDS = ["l1", "smooth_l1", "huber", "slot_cosine", "slot_cosine+mse"]


def _case():
    """B = 33, io = 48, S = 3, step 5, MASKING(0.25); the target of row 2 has slot 1 all zeros."""
    p = ER.problem(IO)
    x = p["data"][p["rows"]].copy()
    x[2, 16:32] = 0.0
    keep = p["table"][p["mask_id"]]
    w = ER.weights(ER.corrupted(keep, p["rows"], 5, MASKING), ALPHA, BETA, np.repeat(np.float32(SLOT_W), IO // S))
    return x, p["y"], keep, w


def _ref(kind, kw, x, y, keep, w, inv_n):
    return RR.loss_terms(kind, x, y, keep, w, inv_n, param=kw.get("beta", kw.get("delta")), mse_weight=kw.get("mse_weight", 0.0), S=S)


def test_the_fixture_discriminates_b33_io48():
    """Both branches of SmoothL1 (beta 0.5) and Huber (delta 0.75) are taken by a large share of the elements, no |d| is so small
    that sign(d) is in doubt, and |cos| stays away from 1."""
    x, y, keep, w = _case()
    d = np.abs(x.astype(np.float64) - y)
    print("min |d| %.2e  |d| < 0.5: %.2f  |d| <= 0.75: %.2f" % (d.min(), (d < 0.5).mean(), (d <= 0.75).mean()))
    assert d.min() > 1e-6 and 0.1 < (d < 0.5).mean() < 0.9 and 0.1 < (d <= 0.75).mean() < 0.9
    cos = _ref("slot_cosine", {}, x, y, keep, None, 1.0)["cos"]
    print("max |cos| %.3f" % np.abs(cos).max())
    assert np.abs(cos).max() < 0.75 and cos[2, 1] == 0.0                  # (0.71 here: 1 - cos keeps at least two of its bits)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("kind,kw", CASES, ids=IDS)
def test_loss_and_autograd_gradient_match_the_reference_b33_io48(kind, kw, weighted):
    """float64 torch against float64 numpy: 1e-12 relative on the loss, 1e-12 of the largest gradient on every element."""
    from codae.tool import ReconstructionLoss
    x, y, keep, w = _case()
    if not weighted:
        w = None
    ref = _ref(kind, kw, x, y, keep, w, np.float32(1.0 / x.size))
    inv = float(np.float32(1.0 / x.size))
    rows = 1.0 / (inv * IO)                                  # the rows that give exactly the fp32 inv_n the reference rounds to
    crit = ReconstructionLoss(kind, **kw)
    out = torch.tensor(y, dtype=torch.float64, requires_grad=True)
    loss = crit.loss(torch.tensor(x, dtype=torch.float64), out, weight=None if w is None else torch.tensor(w), n_slots=S, global_rows=rows)
    loss.backward()
    assert abs(float(loss) - ref["loss"]) <= 1e-12 * abs(ref["loss"]), (float(loss), ref["loss"])
    g = out.grad.numpy()
    assert np.abs(g - ref["dy"]).max() <= 1e-12 * np.abs(ref["dy"]).max(), np.abs(g - ref["dy"]).max()
    if kind == "slot_cosine" and not kw:
        assert (g[2, 16:32] == 0).all()                      # the zero target slot: gradient 0, term W


def test_mse_kind_is_the_emphasised_mse_b33_io48():
    from codae.tool import ReconstructionLoss
    x, y, keep, w = _case()
    ref = ER.loss_terms(x, y, keep, w, 1.0 / x.size)
    got = ReconstructionLoss().loss(torch.tensor(x, dtype=torch.float64), torch.tensor(y, dtype=torch.float64), weight=torch.tensor(w))
    assert abs(float(got) - ref["wsum"] / x.size) <= 1e-12 * ref["wsum"] / x.size


def test_the_reference_is_torchs_definition_b33_io48():
    """tests/recon_loss_ref.py against the installed torch's functional losses and their autograd, in float64."""
    import torch.nn.functional as F
    x, y, keep, w = _case()
    y = y.copy()
    y[5, 0:16] = 0.0                                          # an all-zero output slot too
    tx, tw = torch.tensor(x, dtype=torch.float64), torch.tensor(w)
    inv = float(np.float32(1.0 / x.size))
    for kind, kw in CASES:
        ty = torch.tensor(y, dtype=torch.float64, requires_grad=True)
        if kind == "l1":
            loss = (tw * F.l1_loss(ty, tx, reduction="none")).sum() * inv
        elif kind == "smooth_l1":
            loss = (tw * F.smooth_l1_loss(ty, tx, reduction="none", beta=kw["beta"])).sum() * inv
        elif kind == "huber":
            loss = (tw * F.huber_loss(ty, tx, reduction="none", delta=kw["delta"])).sum() * inv
        else:
            cos = F.cosine_similarity(tx.reshape(-1, S, IO // S), ty.reshape(-1, S, IO // S), dim=-1, eps=1e-8)
            W = tw.reshape(-1, S, IO // S).mean(-1)
            loss = (W * (1 - cos)).sum() * (IO // S) * inv + kw.get("mse_weight", 0.0) * (tw * (tx - ty) ** 2).sum() * inv
        loss.backward()
        ref = _ref(kind, kw, x, y, keep, w, inv)
        assert abs(float(loss) - ref["loss"]) <= 1e-12 * abs(ref["loss"]), (kind, float(loss), ref["loss"])
        err = np.abs(ty.grad.numpy() - ref["dy"]).max()
        assert err <= 1e-12 * np.abs(ref["dy"]).max(), (kind, err)


def test_validation():
    from codae.hip import HipError
    from codae.tool import ReconstructionLoss
    c = ReconstructionLoss()
    assert c.kind == "mse" and c.is_default and c.mse_weight == 0.0
    assert not ReconstructionLoss("l1").is_default
    assert ReconstructionLoss("smooth_l1").beta == 1.0 and ReconstructionLoss("huber", delta=2).delta == 2.0
    assert ReconstructionLoss("slot_cosine", mse_weight=0.1).mse_weight == float(np.float32(0.1))
    bad = [dict(kind="cosine"), dict(kind=3), dict(kind="smooth_l1", beta=0.0), dict(kind="smooth_l1", beta=float("nan")),
           dict(kind="huber", delta=-1.0), dict(kind="huber", delta=float("inf")), dict(kind="huber", beta=1.0), dict(kind="l1", delta=1.0),
           dict(kind="l1", mse_weight=0.5), dict(kind="mse", mse_weight=0.5), dict(kind="slot_cosine", mse_weight=-0.1),
           dict(kind="slot_cosine", mse_weight=float("nan")), dict(kind="huber", delta="1")]
    for kw in bad:
        with pytest.raises(HipError):
            ReconstructionLoss(**kw)
    cos = ReconstructionLoss("slot_cosine")
    for n in (None, 0, 129, 2.5):
        with pytest.raises(HipError):
            cos.as_struct(n)
    x = torch.zeros(4, 6)
    with pytest.raises(HipError, match="divide"):
        cos.loss(x, x, n_slots=4)
    with pytest.raises(HipError, match="n_slots"):
        cos.loss(x, x)
    with pytest.raises(HipError, match="shape"):
        cos.loss(x, x[:, :3], n_slots=3)


def test_as_struct_carries_the_header_fields():
    from codae import hip
    from codae.tool import ReconstructionLoss
    st = ReconstructionLoss("slot_cosine", mse_weight=0.25).as_struct(3)
    assert (st.kind, st.param, st.mse_weight, st.n_slots) == (hip.LOSS_SLOT_COSINE, 0.0, 0.25, 3)
    st = ReconstructionLoss("smooth_l1", beta=0.5).as_struct()
    assert (st.kind, st.param, st.mse_weight, st.n_slots) == (hip.LOSS_SMOOTH_L1, 0.5, 0.0, 0)
    st = ReconstructionLoss("huber", delta=0.75).as_struct(3)
    assert (st.kind, st.param, st.n_slots) == (hip.LOSS_HUBER, 0.75, 0)
    assert ReconstructionLoss().as_struct().kind == hip.LOSS_MSE and ReconstructionLoss("l1").as_struct().kind == hip.LOSS_L1


def test_config_parser():
    from codae.hip import HipError
    from codae.tool.recon_loss import recon_loss_from_config
    assert recon_loss_from_config(None) is None and recon_loss_from_config({}) is None
    c = recon_loss_from_config({"KIND": "slot_cosine", "MSE_WEIGHT": 0.1})
    assert c.kind == "slot_cosine" and c.mse_weight == float(np.float32(0.1))
    assert recon_loss_from_config({"KIND": "smooth_l1", "BETA": 0.5}).beta == 0.5
    assert recon_loss_from_config({"KIND": "huber", "DELTA": 1.0}).delta == 1.0
    assert recon_loss_from_config({"KIND": "mse"}).is_default
    for block in ({"KIND": "l1", "GAMMA": 1}, {"BETA": 0.5}, {"KIND": "huber", "BETA": 0.5}, "l1", {"KIND": "l2"}, {"KIND": "l1", "MSE_WEIGHT": 1.0}):
        with pytest.raises(HipError):
            recon_loss_from_config(block)


def test_trainer_and_tool_export_the_criterion():
    import inspect
    import codae.tool
    from codae.hip.engine import DaeEngine
    from codae.train import HipEmbeddingTrainer
    assert "ReconstructionLoss" in codae.tool.__all__
    assert inspect.signature(HipEmbeddingTrainer.__init__).parameters["criterion"].default is None
    assert callable(HipEmbeddingTrainer.set_criterion) and callable(DaeEngine.set_recon_loss)


def test_header_binding_and_integration_doc_agree_on_the_new_names():
    import ctypes as C
    from codae import hip
    header = open(os.path.join(ROOT, "include", "codae_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert int(re.search(r"#define CODAE_ABI_VERSION (\d+)", header).group(1)) == 11 == hip.ABI_VERSION
    assert int(re.search(r"CODAE_K_COUNT = (\d+)", header).group(1)) == 11 == len(hip.KERNEL_CLASSES)
    enum = {k: int(v) for k, v in re.findall(r"\b(CODAE_LOSS_[A-Z0-9_]+)\s*=\s*(-?\d+)", header)}
    assert enum == {"CODAE_LOSS_MSE": hip.LOSS_MSE, "CODAE_LOSS_L1": hip.LOSS_L1, "CODAE_LOSS_SMOOTH_L1": hip.LOSS_SMOOTH_L1,
                    "CODAE_LOSS_HUBER": hip.LOSS_HUBER, "CODAE_LOSS_SLOT_COSINE": hip.LOSS_SLOT_COSINE}
    from codae.tool.recon_loss import COS_EPS, KINDS
    assert {"CODAE_LOSS_" + k.upper(): v for k, v in KINDS.items()} == enum
    assert float(re.search(r"#define CODAE_COS_EPS ([0-9.e+-]+)f", header).group(1)) == COS_EPS == RR.EPS
    body = re.search(r"typedef struct \{([^}]*)\} codae_recon_loss;", header).group(1)
    fields = re.findall(r"\b(int32_t|float)\s+(\w+);", body)
    ctype = {"int32_t": C.c_int32, "float": C.c_float}
    assert [(n, ctype[t]) for t, n in fields] == list(hip.ReconLoss._fields_)
    for fn in ("codae_set_recon_loss", "codae_recon_loss_fwd_bwd", "codae_recon_loss_blocks"):
        assert re.search(r"\b%s\s*\(" % fn, header) and fn in hip.PROTOTYPES and fn in doc, fn
        assert hasattr(hip.lib(), fn), fn
    for word in ("codae_recon_loss", "CODAE_LOSS_SLOT_COSINE", "CODAE_COS_EPS", "ReconstructionLoss", "CRITERION"):
        assert word in doc, word
    # the launcher's binding has one ctypes argument per C parameter
    proto = re.search(r"int codae_recon_loss_fwd_bwd\(([^;]*)\);", header).group(1)
    assert len(proto.split(",")) == len(hip.PROTOTYPES["codae_recon_loss_fwd_bwd"][1])
