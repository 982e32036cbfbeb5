"""CPU-only tests of the input noise (include/codae_hip.h, "Input noise"): the generator's known answers, the statistics
of the definition, codae.tool.InputNoise on host tensors against tests/noise_ref.py, and argument validation."""
import math

import numpy as np
import pytest
import torch

import noise_ref as R

KAT = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    """Random123's known-answer vectors for Philox4x32-10, for the reference and for the package's host generator."""
    from codae.tool.noise import philox4x32_10
    assert " ".join("%08x" % int(w) for w in R.philox(counter, key)) == want
    assert " ".join("%08x" % int(w) for w in philox4x32_10(counter, key)) == want


def test_statistics_of_the_definition():
    """256 x 512 elements, seed 20260, step 1; every bound is six standard deviations of the estimator."""
    B, io, seed, step = 256, 512, 20260, 1
    N = B * io
    rows = np.arange(B)
    n = R.unit_normals(rows, io, step, seed)
    assert abs(n.mean()) < 6 / math.sqrt(N), n.mean()
    assert abs(n.var() - 1) < 6 * math.sqrt(2 / N), n.var()
    x = np.full((B, io), 0.5, dtype=np.float32)
    m = R.corrupt(x, rows, step, "masking", seed=seed, p=0.25)
    assert set(np.unique(m)) == {np.float32(0), np.float32(0.5)}
    assert abs((m == 0).mean() - 0.25) < 6 * math.sqrt(0.25 * 0.75 / N)
    sp = R.corrupt(x, rows, step, "salt_pepper", seed=seed, p=0.1, lo=-1.0, hi=2.0)
    hit = sp != 0.5
    assert abs(hit.mean() - 0.1) < 6 * math.sqrt(0.1 * 0.9 / N)
    assert set(np.unique(sp[hit])) == {np.float32(-1), np.float32(2)}
    assert abs((sp[hit] == -1).mean() - 0.5) < 6 * math.sqrt(0.25 / hit.sum())
    # another step or another seed is another stream
    w = R.words(rows, io, step, seed)
    assert (w != R.words(rows, io, step + 1, seed)).mean() > 0.999
    assert (w != R.words(rows, io, step, seed + 1)).mean() > 0.999


def _problem(io, B=67, n_rows=300, S=None):
    rng = np.random.default_rng(io)
    x = rng.standard_normal((B, io)).astype(np.float32)
    rows = rng.permutation(n_rows)[:B]
    keep = np.ones((B, io), dtype=np.float32)
    width = max(1, io // 4)
    for b in range(B):                       # one blanked span per row (the Corrupter's whole-slot blank)
        s = int(rng.integers(0, io - width + 1))
        keep[b, s:s + width] = 0
    return x, rows, keep


@pytest.mark.parametrize("io", [48, 44, 11])
@pytest.mark.parametrize("kind,kw", [("masking", dict(p=0.25)), ("salt_pepper", dict(p=0.1, lo=-0.75, hi=1.5)),
                                     ("gaussian", dict(sigma=0.3))])
def test_apply_on_host_tensors_equals_the_reference(io, kind, kw):
    from codae.tool import InputNoise
    x, rows, keep = _problem(io)
    seed, step = 0x0123456789ABCDEF, 7
    noise = InputNoise(kind, seed=seed, **kw)
    for mask in (None, keep):
        got = noise.apply(torch.from_numpy(x), torch.from_numpy(rows), step,
                          mask=None if mask is None else torch.from_numpy(mask))
        assert got.dtype == torch.float32 and tuple(got.shape) == x.shape
        got = got.numpy()
        if kind == "gaussian":
            ref, mag = R.corrupt(x, rows, step, kind, seed=seed, keep=mask, **kw)
            assert (np.abs(got - ref) <= R.gaussian_tol(mag, kw["sigma"])).all(), np.abs(got - ref).max()
            assert (got != x)[keep != 0].mean() > 0.99
        else:
            ref = R.corrupt(x, rows, step, kind, seed=seed, keep=mask, **kw)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
            assert (got != x).any()
        if mask is not None:
            assert (got[mask == 0] == 0).all()
    # keyed by the dataset row: another batch order gives the same rows
    perm = np.random.default_rng(1).permutation(len(rows))
    a = noise.apply(torch.from_numpy(x), rows, step).numpy()
    b = noise.apply(torch.from_numpy(x[perm]), rows[perm], step).numpy()
    assert np.array_equal(a[perm].view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("args,kw,word", [
    (("uniform",), dict(p=0.1), "kind"),
    (("gaussian",), dict(), "sigma"),
    (("gaussian",), dict(sigma=-1.0), "sigma"),
    (("gaussian",), dict(sigma=float("nan")), "sigma"),
    (("gaussian",), dict(sigma=0.1, p=0.5), " p"),
    (("masking",), dict(), "p is missing"),
    (("masking",), dict(p=1.5), "p ="),
    (("masking",), dict(p=float("inf")), "p ="),
    (("salt_pepper",), dict(p=0.1, lo=0.0), "hi"),
    (("salt_pepper",), dict(p=0.1, lo=float("nan"), hi=1.0), "lo"),
    (("masking",), dict(p=0.1, seed=-1), "seed"),
    (("masking",), dict(p=0.1, seed=2 ** 64), "seed"),
])
def test_argument_validation(args, kw, word):
    from codae.hip import HipError
    from codae.tool import InputNoise
    with pytest.raises(HipError, match=word):
        InputNoise(*args, **kw)


def test_parameters_are_the_fp32_values_of_the_c_struct():
    from codae.tool import InputNoise
    n = InputNoise("salt_pepper", p=0.1, lo=0.3, hi=0.7, seed=2 ** 64 - 1)
    assert n.p == float(np.float32(0.1)) and n.threshold == R.threshold(0.1) == 429496736
    st = n.as_struct()
    assert (st.kind, st.p0, st.p1, st.p2, st.seed) == (3, n.p, n.lo, n.hi, 2 ** 64 - 1)
    assert InputNoise("masking", p=1.0).threshold == 2 ** 32 and InputNoise("masking", p=0.0).threshold == 0
    x = torch.ones(4, 8)
    assert (InputNoise("masking", p=1.0).apply(x, range(4), 1) == 0).all()
    assert torch.equal(InputNoise("masking", p=0.0).apply(x, range(4), 1), x)
    assert torch.equal(InputNoise("gaussian", sigma=0.0).apply(x, range(4), 1), x)


def test_apply_rejects_mismatched_arguments():
    from codae.hip import HipError
    from codae.tool import InputNoise
    n = InputNoise("masking", p=0.5)
    x = torch.zeros(4, 8)
    with pytest.raises(HipError, match="rows"):
        n.apply(x, [0, 1, 2], 1)
    with pytest.raises(HipError, match="mask shape"):
        n.apply(x, range(4), 1, mask=torch.ones(4, 7))
    with pytest.raises(HipError, match="step"):
        n.apply(x, range(4), -1)
    with pytest.raises(HipError, match=r"\[B, io\]"):
        n.apply(torch.zeros(8), range(4), 1)


def test_config_block_parser():
    from codae.hip import HipError
    from codae.tool.noise import input_noise_from_config
    assert input_noise_from_config(None) is None and input_noise_from_config({}) is None
    g = input_noise_from_config({"KIND": "gaussian", "SIGMA": 0.05, "SEED": 3})
    assert (g.kind, g.sigma, g.seed) == ("gaussian", float(np.float32(0.05)), 3)
    m = input_noise_from_config({"KIND": "Masking", "P": 0.25})
    assert (m.kind, m.p, m.seed) == ("masking", 0.25, 0)
    data = torch.tensor([[-2.0, 0.5], [0.25, 3.0]])
    sp = input_noise_from_config({"KIND": "salt_pepper", "P": 0.1}, data)
    assert (sp.lo, sp.hi) == (-2.0, 3.0)                       # LO / HI default to the resident data's min / max
    sp = input_noise_from_config({"KIND": "salt_pepper", "P": 0.1, "LO": 0.0}, data)
    assert (sp.lo, sp.hi) == (0.0, 3.0)
    for block, word in (({"KIND": "uniform", "P": 0.1}, "kind"), ({"KIND": "gaussian"}, "sigma"),
                        ({"KIND": "masking", "SIGMA": 0.1}, "sigma"), ({"P": 0.1}, "KIND"),
                        ({"KIND": "masking", "P": 0.1, "RATE": 2}, "RATE"), ("gaussian", "mapping"),
                        ({"KIND": "salt_pepper", "P": 0.1}, "lo")):
        with pytest.raises(HipError, match=word):
            input_noise_from_config(block)
