"""CPU-only tests of the `activation` argument: which torch modules map to which engine activation (CODAE_ACT_*), which
are refused at model construction, and a numpy restatement of the kernels' forward / derivative-from-output formulas
(csrc/codae_common.h act_fwd / act_dy_from_y) against float64 torch autograd."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
nn = torch.nn


def _hip():
    from codae import hip
    return hip


# (factory, expected (kind name, p0, p1, p2)); factories as users write them: the class itself (called as activation(True),
# the reference's idiom) or a lambda taking `inplace`
def _cases():
    from codae.model.activation import SELU_ALPHA, SELU_SCALE
    return [
        (nn.ReLU, ("RELU", 0, 0, 0)),
        (nn.LeakyReLU, ("LEAKY", 1.0, 0, 0)),                         # negative_slope=True
        (lambda inplace: nn.LeakyReLU(0.2, inplace), ("LEAKY", 0.2, 0, 0)),
        (lambda inplace: nn.LeakyReLU(0.0, inplace), ("LEAKY", 0.0, 0, 0)),
        (nn.ReLU6, ("RELU6", 0, 0, 0)),
        (nn.ELU, ("ELU", 1.0, 1.0, 1.0)),                             # alpha=True
        (lambda inplace: nn.ELU(0.5, inplace), ("ELU", 1.0, 0.5, 1.0)),
        (nn.CELU, ("ELU", 1.0, 1.0, 1.0)),
        (lambda inplace: nn.CELU(2.0, inplace), ("ELU", 1.0, 2.0, 0.5)),
        (nn.SELU, ("ELU", SELU_SCALE, SELU_ALPHA, 1.0)),
        (nn.Softplus, ("SOFTPLUS", 1.0, 20.0, 0)),                    # beta=True
        (lambda inplace: nn.Softplus(2.0, 10.0), ("SOFTPLUS", 2.0, 10.0, 0)),
        (nn.Hardsigmoid, ("HARDSIGMOID", 0, 0, 0)),
    ]


def test_every_supported_module_maps_to_its_kind_and_parameters():
    hip = _hip()
    from codae.model.activation import as_engine_act, from_factory
    for factory, (name, p0, p1, p2) in _cases():
        got = from_factory(factory)
        assert got[0] == getattr(hip, "ACT_" + name), (factory, got)
        assert np.allclose(got[1:], (p0, p1, p2), rtol=1e-12, atol=0), (factory, got)
        assert as_engine_act(factory(True)) == got
    assert from_factory(None) is None


@pytest.mark.parametrize("bad", [nn.SiLU, nn.Mish, nn.Hardswish, lambda inplace: nn.LeakyReLU(-0.1),
                                 lambda inplace: nn.Tanhshrink(),
                                 "subclass"])
def test_unsupported_activations_are_refused_at_model_construction(bad):
    from codae.hip import HipError
    from codae.model import EmbeddingDenoisingAutoencoder, MixedVariableDenoisingAutoencoder
    if bad == "subclass":
        class MyReLU(nn.ReLU):          # exact type match: a subclass may compute something else
            pass
        bad = MyReLU
    with pytest.raises(HipError, match="supported: ReLU"):
        EmbeddingDenoisingAutoencoder(48, 16, 16, 2, 2, False, activation=bad)
    with pytest.raises(HipError, match="not supported"):
        MixedVariableDenoisingAutoencoder([], 48, 16, torch.device("cpu"), 2, 2, False, activation=bad)


@pytest.mark.parametrize("factory", [nn.ELU, nn.SELU, nn.Softplus, lambda inplace: nn.LeakyReLU(0.1, inplace)])
def test_models_hand_their_activation_to_the_engine(factory):
    from codae.model import EmbeddingDenoisingAutoencoder, MixedVariableDenoisingAutoencoder
    from codae.model.activation import from_factory
    want = from_factory(factory)
    m = EmbeddingDenoisingAutoencoder(48, 16, 16, 2, 2, False, activation=factory)
    assert m._acts == [want if r else (0, 0.0, 0.0, 0.0) for _, _, r in m._schedule]
    mm = MixedVariableDenoisingAutoencoder([], 48, 16, torch.device("cpu"), 2, 2, False, activation=factory)
    assert mm._acts == [want if r else (0, 0.0, 0.0, 0.0) for _, _, r in mm._schedule]
    # the default (ReLU) keeps the engine's ReLU flags: no activation spec at all
    assert EmbeddingDenoisingAutoencoder(48, 16, 16, 2, 2, False)._acts is None
    assert EmbeddingDenoisingAutoencoder(48, 16, 16, 2, 2, False, activation=nn.ReLU)._acts is None


# ---- numpy restatement of act_fwd / act_dy_from_y (fp32 arithmetic, as the kernels do it) ----------------------------
def np_fwd(kind, p, v):
    hip = _hip()
    v = v.astype(np.float32)
    p = [np.float32(x) for x in p]
    with np.errstate(over="ignore"):
        if kind == hip.ACT_RELU:
            return np.where(v > 0, v, np.float32(0))
        if kind == hip.ACT_LEAKY:
            return np.where(v > 0, v, v * p[0])
        if kind == hip.ACT_RELU6:
            return np.clip(v, np.float32(0), np.float32(6))
        if kind == hip.ACT_ELU:
            return np.where(v > 0, v * p[0], np.expm1(v * p[2]) * (p[1] * p[0]))
        if kind == hip.ACT_SOFTPLUS:
            return np.where(v * p[0] > p[1], v, np.log1p(np.exp(v * p[0])) / p[0])
        if kind == hip.ACT_HARDSIGMOID:
            return np.clip(v + np.float32(3), np.float32(0), np.float32(6)) * np.float32(1.0 / 6.0)
    return v


def np_dy_from_y(kind, p, y):
    hip = _hip()
    y = y.astype(np.float32)
    p = [np.float32(x) for x in p]
    one, zero = np.float32(1), np.float32(0)
    if kind == hip.ACT_RELU:
        return np.where(y > 0, one, zero)
    if kind == hip.ACT_LEAKY:
        return np.where(y > 0, one, p[0])
    if kind == hip.ACT_RELU6:
        return np.where((y > 0) & (y < 6), one, zero)
    if kind == hip.ACT_ELU:
        return np.where(y > 0, p[0], p[2] * (y + p[1] * p[0]))
    if kind == hip.ACT_SOFTPLUS:
        return np.where(y * p[0] > p[1], one, -np.expm1(-y * p[0]))
    if kind == hip.ACT_HARDSIGMOID:
        return np.where((y > 0) & (y < 1), np.float32(1.0 / 6.0), zero)
    return np.ones_like(y)


def _grid():
    v = np.concatenate([np.linspace(-12, 12, 481), [0.0, -0.0, 6.0, 3.0, -3.0, 1e-3, -1e-3, 5.999, 6.001],
                        np.random.default_rng(0).normal(0, 4, 300)])
    # Softplus threshold neighbourhood (beta 1 threshold 20, beta 2 threshold 10: v * beta around the threshold)
    v = np.concatenate([v, 20 + np.linspace(-0.5, 0.5, 21), 5 + np.linspace(-0.25, 0.25, 21)])
    return v.astype(np.float32)


@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("i", range(13))
def test_formulas_match_float64_autograd(i, inplace):
    from codae.model.activation import from_factory
    factory, _ = _cases()[i]
    kind, p0, p1, p2 = from_factory(factory)
    mod = factory(True)
    if hasattr(mod, "inplace"):
        mod.inplace = inplace
    v = _grid()
    # float64 torch: forward and autograd derivative (in place: the module overwrites its input, autograd then takes
    # the derivative from the OUTPUT, as the engine does)
    x = torch.tensor(v, dtype=torch.float64, requires_grad=True)
    h = x * 1.0
    y = mod(h)
    y.backward(torch.ones_like(y))
    y64, d64 = y.detach().numpy(), x.grad.numpy()
    y32 = np_fwd(kind, (p0, p1, p2), v)
    assert np.allclose(y32, y64, rtol=1e-5, atol=1e-6), np.abs(y32 - y64).max()
    d32 = np_dy_from_y(kind, (p0, p1, p2), y32)
    # exact boundaries: ReLU-type kinks at 0 and 6 (and Hardsigmoid's +-3) take torch's one-sided choice; elsewhere the
    # derivative from the fp32 output matches float64 to fp32 rounding (Softplus near its threshold: 1 - 2e-9 vs 1)
    hip = _hip()
    piecewise = kind in (hip.ACT_RELU, hip.ACT_LEAKY, hip.ACT_RELU6, hip.ACT_HARDSIGMOID)
    kink = np.isin(v, [0.0, 6.0, 3.0, -3.0]) & piecewise
    assert np.allclose(d32[~kink], d64[~kink], rtol=1e-4, atol=2e-6), np.abs(d32 - d64)[~kink].max()
    assert np.array_equal(d32[kink], d64[kink].astype(np.float32)), (v[kink], d32[kink], d64[kink])


def test_header_activation_constants_equal_the_bindings():
    hip = _hip()
    header = open(os.path.join(ROOT, "include", "codae_hip.h")).read()
    A = {k: int(v) for k, v in re.findall(r"\b(CODAE_ACT_[A-Z0-9_]+)\s*=\s*(-?\d+)", header)}
    names = ("NONE", "RELU", "LEAKY", "RELU6", "ELU", "SOFTPLUS", "HARDSIGMOID")
    assert set(A) == {"CODAE_ACT_" + n for n in names}
    for n in names:
        assert getattr(hip, "ACT_" + n) == A["CODAE_ACT_" + n], n
    assert [f for f, _ in hip.Spec._fields_][-2:] == ["act_kind", "act_param"]
    for fn in ("codae_linear_act_f32", "codae_dgrad_act_f32", "codae_linear_act_bf16", "codae_dgrad_act_bf16"):
        assert fn in hip.PROTOTYPES and fn + "(" in header


def test_engine_activation_argument_resolves_per_layer():
    """DaeEngine(activation=) -> per-layer spec without a device: the resolution helper alone."""
    from codae.hip.engine import DaeEngine
    eng = DaeEngine.__new__(DaeEngine)
    eng.schedule = [(48, 48, True), (48, 16, False), (16, 48, True), (48, 48, False)]
    eng.L = 4
    hip = _hip()
    assert eng._layer_acts(None) is None
    acts = eng._layer_acts(nn.ELU)
    assert [a[0] for a in acts] == [hip.ACT_ELU, 0, hip.ACT_ELU, 0]
    acts = eng._layer_acts((hip.ACT_LEAKY, 0.1, 0, 0))
    assert [a[0] for a in acts] == [hip.ACT_LEAKY, 0, hip.ACT_LEAKY, 0] and acts[0][1] == 0.1
