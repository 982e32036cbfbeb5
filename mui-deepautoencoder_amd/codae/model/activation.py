"""The `activation` argument of the model classes, as the HIP engine runs it.

The reference constructors call `activation(True)` once per hidden Linear (embedding_denoising_autoencoder.py:63-126);
`as_engine_act` maps the module that call built to (CODAE_ACT_* kind, p0, p1, p2) of include/codae_hip.h, or raises.
Only monotone activations are accepted: the engine keeps each layer's OUTPUT for the backward and takes the derivative
from it (what torch's in-place backward of these modules does).  SiLU, Mish, Hardswish are not monotone - the output does
not determine the input - and a negative LeakyReLU slope is refused by torch's in-place form too.  Types are matched
exactly: a subclass may change the function.
"""
import torch

from ..hip import ACT_ELU, ACT_HARDSIGMOID, ACT_LEAKY, ACT_RELU, ACT_RELU6, ACT_SOFTPLUS, HipError

# torch.nn.SELU's constants (torch/csrc/api/include/torch/nn/functional/activation.h, aten Activation.cpp)
SELU_ALPHA = 1.6732632423543772848170429916717
SELU_SCALE = 1.0507009873554804934193349852946

SUPPORTED = ("ReLU", "LeakyReLU (negative_slope >= 0)", "ReLU6", "ELU", "CELU", "SELU", "Softplus", "Hardsigmoid")


def _refuse(module, why):
    raise HipError("activation %s is not supported by the HIP engine (%s); supported: %s"
                   % (type(module).__name__, why, ", ".join(SUPPORTED)))


def as_engine_act(module):
    """(kind, p0, p1, p2) of a built activation module; HipError for anything the engine cannot run."""
    t = type(module)
    nn = torch.nn
    if t is nn.ReLU:
        return (ACT_RELU, 0.0, 0.0, 0.0)
    if t is nn.LeakyReLU:
        s = float(module.negative_slope)
        if not s >= 0.0:
            _refuse(module, "negative_slope %g < 0: the output does not determine the input" % s)
        return (ACT_LEAKY, s, 0.0, 0.0)
    if t is nn.ReLU6:
        return (ACT_RELU6, 0.0, 0.0, 0.0)
    if t is nn.ELU:
        a = float(module.alpha)
        if not a > 0.0:
            _refuse(module, "alpha %g <= 0" % a)
        return (ACT_ELU, 1.0, a, 1.0)
    if t is nn.CELU:
        a = float(module.alpha)
        if not a > 0.0:
            _refuse(module, "alpha %g <= 0" % a)
        return (ACT_ELU, 1.0, a, 1.0 / a)
    if t is nn.SELU:
        return (ACT_ELU, SELU_SCALE, SELU_ALPHA, 1.0)
    if t is nn.Softplus:
        b = float(module.beta)
        if not b > 0.0:
            _refuse(module, "beta %g <= 0" % b)
        return (ACT_SOFTPLUS, b, float(module.threshold), 0.0)
    if t is nn.Hardsigmoid:
        return (ACT_HARDSIGMOID, 0.0, 0.0, 0.0)
    if t in (nn.SiLU, nn.Mish, nn.Hardswish):
        _refuse(module, "not monotone: the saved output does not determine the derivative")
    _refuse(module, "unknown activation module")


def from_factory(activation):
    """The engine tuple of what activation(True) builds (the reference's call), or None for None."""
    if activation is None:
        return None
    return as_engine_act(activation(True))
