"""codae.tool.Norm on the host (no GPU): which layers it resolves to and what it refuses, the config block, the checkpoint record,
and Norm.forward with its autograd gradients against torch.nn.functional.layer_norm / an explicit RMS expression in float64 and
against the hand-written statement the GPU tests use (tests/norm_ref.py)."""
import math

import numpy as np
import pytest

import norm_ref as NR

torch = pytest.importorskip("torch")
LEAKY = 0.1


def _tools():
    from codae.hip import HipError
    from codae.tool import Norm, Residual, norm_from_config
    return Norm, Residual, norm_from_config, HipError


def test_resolve_hidden_lists_layer0_and_tapers():
    Norm, _, _, _ = _tools()
    sq = ([24] * 4, [24] * 4)
    assert Norm().resolve(*sq, [True, True, True, False]) == [1, 1, 1, 0]            # "hidden" takes layer 0 as well
    assert Norm("rms").resolve(*sq, [True, True, True, False]) == [1, 1, 1, 0]
    assert Norm(layers=[0]).resolve(*sq, [True] * 3 + [False]) == [1, 0, 0, 0]
    assert Norm(layers=[2, 1]).resolve(*sq, [True] * 3 + [False]) == [0, 1, 1, 0]
    assert Norm(layers=[]).resolve(*sq, [True] * 3 + [False]) == [0, 0, 0, 0] and Norm(layers=[]).is_off
    taper = ([48, 24, 16, 24], [24, 16, 24, 48])
    assert Norm().resolve(*taper, [True, False, True, False]) == [1, 1, 1, 0]         # no equal widths needed; none on the code layer
    assert Norm(layers=[1]).resolve(*taper, [True, False, True, False]) == [0, 1, 0, 0]
    # "hidden" leaves out what cannot take a norm: an ELU layer (kind 4), the last layer
    assert Norm().resolve(*sq, [1, (4, 1.0, 1.0, 1.0), (2, LEAKY, 0, 0), 0]) == [1, 0, 1, 0]
    assert repr(Norm("rms", layers=[1], eps=1e-6)) == "Norm('rms', layers=[1], eps=1e-06)"


def test_refusals_name_the_layer_and_the_reason():
    Norm, _, _, HipError = _tools()
    sq = ([24] * 4, [24] * 4)
    with pytest.raises(HipError, match=r"layer 3: the last layer's output is the reconstruction"):
        Norm(layers=[3]).resolve(*sq, [True] * 3 + [False])
    with pytest.raises(HipError, match=r"layer 1: a normalised layer's activation must be none, ReLU or LeakyReLU \(got ELU\)"):
        Norm(layers=[1]).resolve(*sq, [1, (4, 1.0, 1.0, 1.0), 1, 0])
    with pytest.raises(HipError, match=r"layer 7: the stack has 4 layers"):
        Norm(layers=[7]).resolve(*sq, [True] * 3 + [False])
    with pytest.raises(HipError, match="3 activations"):
        Norm().resolve(*sq, [True] * 3)
    with pytest.raises(HipError, match="kind must be 'layer' or 'rms'"):
        Norm("batch")
    with pytest.raises(HipError, match="listed twice"):
        Norm(layers=[1, 1])
    with pytest.raises(HipError, match="integers >= 0"):
        Norm(layers=[-1])
    with pytest.raises(HipError, match="'hidden' or a list"):
        Norm(layers="all")


@pytest.mark.parametrize("eps", [0.0, -1e-5, float("nan"), float("inf"), -float("inf"), "x"])
def test_eps_must_be_finite_and_positive(eps):
    Norm, _, _, HipError = _tools()
    with pytest.raises(HipError, match="eps"):
        Norm(eps=eps)


def test_config_block():
    Norm, _, norm_from_config, HipError = _tools()
    assert norm_from_config(None) is None and norm_from_config({}) is None
    n = norm_from_config({"KIND": "layer", "LAYERS": "hidden", "EPS": "1e-5"})       # (a YAML loader reads 1e-5 as a string)
    assert (n.kind, n.layers, n.eps) == ("layer", "hidden", 1e-5)
    n = norm_from_config({"KIND": "RMS", "LAYERS": [0, 2], "EPS": 1e-6})
    assert (n.kind, n.layers, n.eps) == ("rms", (0, 2), 1e-6)
    n = norm_from_config({"KIND": "rms"})
    assert (n.kind, n.layers, n.eps) == ("rms", "hidden", 1e-5)
    with pytest.raises(HipError, match=r"NORM: unknown key\(s\) GAIN"):
        norm_from_config({"KIND": "layer", "GAIN": True})
    with pytest.raises(HipError, match="must be a mapping"):
        norm_from_config("layer")
    with pytest.raises(HipError, match="eps"):
        norm_from_config({"EPS": 0})


def test_checkpoint_record_and_mismatch():
    from codae.tool.norm import meta_mismatch, meta_record, norm_from_meta
    Norm, _, _, _ = _tools()
    n = Norm("rms", eps=1e-6)
    rec = meta_record(n, [0, 1, 2])
    assert rec == {"kind": "rms", "eps": 1e-6, "layers": [0, 1, 2]}
    assert meta_record(None, []) is None and meta_record(n, []) is None               # off: no key is written
    assert meta_mismatch({"norm": rec}, n, [0, 1, 2]) is None
    assert meta_mismatch({}, None, []) is None and meta_mismatch({"norm": None}, Norm(layers=[]), []) is None
    assert "norm: none" in meta_mismatch({"norm": rec}, None, [])                     # written with, loaded without
    assert "this trainer has norm: rms norm" in meta_mismatch({}, n, [0, 1, 2])       # and the other way round
    assert meta_mismatch({"norm": rec}, Norm("layer", eps=1e-6), [0, 1, 2]) is not None
    assert meta_mismatch({"norm": rec}, Norm("rms", eps=1e-5), [0, 1, 2]) is not None
    assert meta_mismatch({"norm": rec}, n, [0, 1]) is not None
    back = norm_from_meta({"norm": rec})
    assert (back.kind, back.eps, back.layers) == ("rms", 1e-6, (0, 1, 2)) and norm_from_meta({}) is None


# ---- Norm.forward and its gradients ---------------------------------------------------------------------------------------------

def _stack(widths, acts, seed):
    rng = np.random.default_rng(seed)
    params = [((rng.standard_normal((n, k)) / math.sqrt(k)).astype(np.float32), (rng.standard_normal(n) * 0.05).astype(np.float32))
              for k, n in zip(widths[:-1], widths[1:])]
    x = rng.random((19, widths[0])).astype(np.float32)
    c = x.copy()
    c[:, : widths[0] // 3] = 0
    return params, x, c


def _torch_reference(params, acts, skips, norms, kind, eps, c):
    """the same network from torch's own layer_norm / an explicit RMS expression, float64, with autograd"""
    F = torch.nn.functional
    ws = [torch.tensor(w, dtype=torch.float64, requires_grad=True) for w, _ in params]
    bs = [torch.tensor(b, dtype=torch.float64, requires_grad=True) for _, b in params]
    h = torch.tensor(c, dtype=torch.float64)
    for l in range(len(params)):
        z = h @ ws[l].t() + bs[l]
        a = z if acts[l] is None else (torch.relu(z) if acts[l] == "relu" else F.leaky_relu(z, float(np.float32(acts[l][1]))))
        s = a + h if skips[l] else a
        if norms[l]:
            e = float(np.float32(eps))
            s = F.layer_norm(s, (s.shape[1],), eps=e) if kind == "layer" else s * torch.rsqrt((s * s).mean(dim=1, keepdim=True) + e)
        h = s
    return h, ws, bs


CASES = [
    ("L4-relu-hidden", [24] * 5, ["relu"] * 3 + [None], [0] * 4, "hidden"),
    ("L5-leaky-hidden-skips", [24] * 6, [("leaky", LEAKY)] * 4 + [None], [0, 1, 1, 1, 0], "hidden"),
    ("L4-relu-layer0", [24] * 5, ["relu"] * 3 + [None], [0] * 4, [0]),
    ("L5-some-both", [24] * 6, ["relu"] * 4 + [None], [0, 1, 0, 1, 0], [1, 2]),
    ("taper", [48, 24, 16, 24, 48], ["relu", None, "relu", None], [0] * 4, "hidden"),
]


@pytest.mark.parametrize("kind", ["layer", "rms"])
@pytest.mark.parametrize("name,widths,acts,skips,layers", CASES, ids=[c[0] for c in CASES])
def test_forward_and_autograd_match_torch_and_the_hand_written_statement(name, widths, acts, skips, layers, kind):
    Norm, Residual, _, _ = _tools()
    eps = 1e-5
    params, x, c = _stack(widths, acts, seed=len(name))
    L = len(params)
    norm = Norm(kind, layers=layers, eps=eps)
    codes = [(0 if a is None else 1 if a == "relu" else 2, 0.0 if a in (None, "relu") else a[1], 0.0, 0.0) for a in acts]
    flags = norm.resolve(widths[:-1], widths[1:], codes)
    res = Residual([l for l, s in enumerate(skips) if s]) if any(skips) else None
    # torch's layer_norm, autograd
    y_t, ws, bs = _torch_reference(params, acts, skips, flags, kind, eps, c)
    xt = torch.tensor(x, dtype=torch.float64)
    loss_t = ((y_t - xt) ** 2).mean()
    loss_t.backward()
    # Norm.forward, autograd
    w2 = [torch.tensor(w, dtype=torch.float64, requires_grad=True) for w, _ in params]
    b2 = [torch.tensor(b, dtype=torch.float64, requires_grad=True) for _, b in params]
    y_n = norm.forward(torch.tensor(c, dtype=torch.float64), w2, b2, codes, residual=res)
    loss_n = ((y_n - xt) ** 2).mean()
    loss_n.backward()
    assert torch.allclose(y_n, y_t, rtol=1e-10, atol=1e-12)
    for l in range(L):
        assert torch.allclose(w2[l].grad, ws[l].grad, rtol=1e-8, atol=1e-12), ("dW", l)
        assert torch.allclose(b2[l].grad, bs[l].grad, rtol=1e-8, atol=1e-12), ("db", l)
    # the hand-written float64 statement the GPU tests compare the engine with
    grads, loss, y = NR.gradients(params, acts, skips, flags, kind, eps, c, NR.mse(x))
    assert abs(loss - loss_t.item()) <= 1e-12 * abs(loss)
    assert np.allclose(y, y_t.detach().numpy(), rtol=1e-10, atol=1e-12)
    for l in range(L):
        assert np.allclose(grads[l][0], ws[l].grad.numpy(), rtol=1e-8, atol=1e-12), ("dW", l)
        assert np.allclose(grads[l][1], bs[l].grad.numpy(), rtol=1e-8, atol=1e-12), ("db", l)
    # ... and the norm does something
    off = NR.gradients(params, acts, skips, [0] * L, kind, eps, c, NR.mse(x))[1]
    assert abs(off - loss) > 1e-3 * off


@pytest.mark.parametrize("kind", ["layer", "rms"])
def test_the_rounded_restatement_stays_near_the_float64_statement(kind):
    """For scale ("Normalisation"): the relative L2 distance per gradient tensor between the restatement with
    the bf16 engine's roundings and the float64 statement.  A measurement with a sanity interval, not a tolerance: bf16 keeps 8
    significant bits per store and a rounding can flip a ReLU unit near zero, so the two are percents apart, but they are the same
    network - neither equal (the roundings are there) nor unrelated (a relative distance near 1)."""
    widths, acts = [24] * 5, ["relu"] * 3 + [None]
    params, x, c = _stack(widths, acts, seed=3)
    a = NR.gradients(params, acts, [0] * 4, [1, 1, 1, 0], kind, 1e-5, c, NR.mse(x))[0]
    b = NR.gradients(params, acts, [0] * 4, [1, 1, 1, 0], kind, 1e-5, c, NR.mse(x), bf16=True)[0]
    worst = 0.0
    for (aw, ab), (bw, bb) in zip(a, b):
        worst = max(worst, np.linalg.norm(aw - bw) / np.linalg.norm(aw), np.linalg.norm(ab - bb) / np.linalg.norm(ab))
    print("MEASURE %s: rounded restatement vs float64 statement, worst relative L2 of a gradient tensor %.3e" % (kind, worst))
    assert 1e-5 < worst < 0.5


def test_dead_row_and_engine_roundings_of_the_reference():
    z = np.zeros((2, 8), dtype=np.float32)
    for kind in ("layer", "rms"):
        xh, r = NR.normalise64(z, kind, 1e-5)
        assert (xh == 0).all() and np.allclose(r, 1 / math.sqrt(np.float32(1e-5)))
        xh, r = NR.normalise_engine(z, kind, 1e-5, True)
        assert (xh == 0).all() and not np.signbit(xh).any()
