"""CPU-only tests of hidden dropout (include/codae_hip.h, "Hidden dropout"): codae.tool.HiddenDropout.factor against the
independent statement in tests/dropout_ref.py bit for bit, the separation of the streams, the dropped share, validation and
config parsing, and the header's constants against the binding."""
import math
import os
import re

import numpy as np
import pytest

import dropout_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x0123456789ABCDEF
ROWS = np.random.default_rng(11).permutation(120)[:33].astype(np.int32)       # permuted dataset rows of a batch of 33


@pytest.mark.parametrize("width", [21, 24])
@pytest.mark.parametrize("layer", [0, 1, 2])
@pytest.mark.parametrize("step", [1, 5])
def test_factor_equals_the_reference_bit_for_bit_b33(width, layer, step):
    from codae.tool import HiddenDropout
    p = [0.5, 0.25, 0.1][layer]
    d = HiddenDropout([0.5, 0.25, 0.1], seed=SEED)
    got = d.factor(ROWS, layer, width, step)
    ref = DR.factor(ROWS, layer, width, step, SEED, p)
    assert got.dtype == np.float32 and got.shape == (33, width)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert set(np.unique(got)) == {np.float32(0), np.float32(1.0 / (1.0 - float(np.float32(p))))}
    # a scalar p means the same value on every layer; torch rows give a torch tensor
    import torch
    one = HiddenDropout(p, seed=SEED).factor(torch.tensor(ROWS), layer, width, step)
    assert isinstance(one, torch.Tensor) and one.dtype == torch.float32 and np.array_equal(one.numpy().view(np.uint32), ref.view(np.uint32))
    # the factor belongs to the dataset row, not to the position in the batch
    perm = np.random.default_rng(step).permutation(33)
    assert np.array_equal(d.factor(ROWS[perm], layer, width, step), got[perm])


def test_the_stream_changes_with_layer_step_and_seed_and_is_not_the_noise_stream():
    from codae.tool import HiddenDropout
    from codae.tool.noise import noise_words
    d = HiddenDropout(0.5, seed=SEED)
    base = d.words(ROWS, 0, 24, 5)
    assert np.array_equal(base, DR.words(ROWS, 0, 24, 5, SEED))
    others = {"layer": d.words(ROWS, 1, 24, 5), "step": d.words(ROWS, 0, 24, 6), "seed": HiddenDropout(0.5, seed=SEED + 1).words(ROWS, 0, 24, 5),
              "noise": noise_words(ROWS, 24, 5, SEED)}
    for name, w in others.items():
        same = float((w == base).mean())
        assert same < 0.01, (name, same)
    # ... and the factors differ with them (p = 0.5: about half the elements flip)
    f0 = d.factor(ROWS, 0, 24, 5)
    for f in (d.factor(ROWS, 1, 24, 5), d.factor(ROWS, 0, 24, 6), HiddenDropout(0.5, seed=SEED + 1).factor(ROWS, 0, 24, 5)):
        assert 0.3 < float((f != f0).mean()) < 0.7


def test_dropped_share_of_120_x_192_at_p_025_is_within_four_sigma():
    """n = 23040 elements, p = 0.25: sigma = sqrt(p (1 - p) / n) = 0.00285.  The seed is one for which the REFERENCE's share lies
    inside (chosen on the reference alone); the tool must then agree with the reference exactly."""
    from codae.tool import HiddenDropout
    n, p = 120 * 192, 0.25
    rows = np.arange(120)
    ref = DR.dropped(rows, 1, 192, 3, 7, p)
    share = float(ref.mean())
    sigma = math.sqrt(p * (1 - p) / n)
    print("reference share", share, "sigma", sigma)
    assert abs(share - p) <= 4 * sigma
    got = HiddenDropout(p, seed=7).factor(rows, 1, 192, 3) == 0
    assert np.array_equal(got, ref)


def test_validation_and_depth_resolution():
    from codae.hip import HipError
    from codae.tool import HiddenDropout
    d = HiddenDropout(0.1, seed=3)
    assert d.p == float(np.float32(0.1)) and d.seed == 3 and not d.is_identity
    assert d.per_layer(4) == [float(np.float32(0.1))] * 3
    assert HiddenDropout(0).is_identity and HiddenDropout([0, 0.0]).is_identity
    assert HiddenDropout([0.5, 0, 0.25]).per_layer(4) == [0.5, 0.0, 0.25]
    with pytest.raises(HipError, match="2 probabilities for 3 hidden outputs"):
        HiddenDropout([0.5, 0.25]).per_layer(4)
    for bad, word in [(1.0, "outside"), (-0.1, "outside"), (float("nan"), "not finite"), (float("inf"), "not finite"), ("0.5", "number"),
                      (True, "number"), ([0.5, 1.5], "p\\[1\\]"), ([], "empty"), ([0.5, None], "p\\[1\\]")]:
        with pytest.raises(HipError, match=word):
            HiddenDropout(bad)
    for seed in (-1, 2 ** 64, 1.5, True):
        with pytest.raises(HipError, match="seed"):
            HiddenDropout(0.5, seed=seed)
    with pytest.raises(HipError, match="step"):
        d.factor(ROWS, 0, 24, -1)
    with pytest.raises(HipError, match="layer 3"):
        HiddenDropout([0.5, 0.5, 0.5]).factor(ROWS, 3, 24, 1)
    assert HiddenDropout.threshold(0.25) == 2 ** 30 and HiddenDropout.threshold(0.0) == 0
    assert HiddenDropout.threshold(0.1) == DR.threshold(0.1) and HiddenDropout.scale(0.1) == DR.scale(0.1)


def test_config_parsing_refuses_unknown_keys():
    from codae.hip import HipError
    from codae.tool.dropout import hidden_dropout_from_config
    assert hidden_dropout_from_config(None) is None and hidden_dropout_from_config({}) is None
    d = hidden_dropout_from_config({"P": 0.5, "SEED": 3})
    assert (d.p, d.seed) == (0.5, 3)
    d = hidden_dropout_from_config({"P": [0, 0.5, 0]})
    assert d.p == (0.0, 0.5, 0.0) and d.seed == 0
    with pytest.raises(HipError, match="unknown key.*RATE"):
        hidden_dropout_from_config({"P": 0.5, "RATE": 0.1})
    with pytest.raises(HipError, match="P is missing"):
        hidden_dropout_from_config({"SEED": 1})
    with pytest.raises(HipError, match="mapping"):
        hidden_dropout_from_config([0.5])
    with pytest.raises(HipError, match="outside"):
        hidden_dropout_from_config({"P": 1.0})


def test_header_constants_agree_with_the_binding():
    import ctypes as C
    from codae import hip
    header = open(os.path.join(ROOT, "include", "codae_hip.h")).read()
    K = {k: int(v) for k, v in re.findall(r"\b(CODAE_K_[A-Z0-9_]+)\s*=\s*(\d+)", header)}
    assert K["CODAE_K_DROPOUT"] == 10 == hip.KERNEL_CLASSES.index("dropout") and K["CODAE_K_COUNT"] == 11 == len(hip.KERNEL_CLASSES)
    assert int(re.search(r"#define CODAE_ABI_VERSION (\d+)", header).group(1)) == 11 == hip.ABI_VERSION
    for fn in ("codae_set_hidden_dropout", "codae_dropout_fwd", "codae_dropout_bwd", "codae_dropout_blocks"):
        assert fn in hip.PROTOTYPES and fn + "(" in header
    assert [n for n, _ in hip.Dropout._fields_] == ["p", "n", "seed"] and C.sizeof(hip.Dropout) == 24
    lib = hip.lib()
    assert lib.codae_abi_version() == 11
    assert [lib.codae_dropout_blocks(b) for b in (0, 1, 64, 65, 70, 8192)] == [0, 1, 1, 2, 2, 128]


def test_the_whole_array_philox_of_the_reference_is_its_plain_one():
    rows = np.array([0, 1, 5, 299, 2999, 2 ** 31 - 1], dtype=np.int32)
    for layer, width, step, seed in ((0, 1, 0, 0), (1, 21, 5, 0x0123456789ABCDEF), (254, 40, 2 ** 31 - 1, 2 ** 64 - 1)):
        assert np.array_equal(DR.words_vec(rows, layer, width, step, seed), DR.words(rows, layer, width, step, seed))
