"""CPU-only tests of tied weights (include/codae_hip.h, "Tied weights"): which layers pair up and which stacks are refused, the torch
twins of the fold and the mirror against autograd through a shared nn.Parameter (tests/tied_ref.py), the C header / ctypes
surface, and the training config key."""
import os
import re

import numpy as np
import pytest
import torch

import tied_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stack(nb_in, nb_out, z, io=192, steep=False):
    from codae.model.schedule import linear_stack
    enc, dec = linear_stack(io, z, nb_in, nb_out, steep, False)
    return enc + dec


def test_pairs_of_the_square_and_taper_stacks():
    from codae.tool import TiedWeights
    for z in (192, 64):                                     # 4 + 4: square (z = io) and taper
        sched = _stack(4, 4, z)
        assert len(sched) == 10
        assert TiedWeights.pairs(sched) == [(0, 9), (1, 8), (2, 7), (3, 6), (4, 5)]
        for l, m in TiedWeights.pairs(sched):
            assert sched[l][0] == sched[m][1] and sched[l][1] == sched[m][0]
    wide = [(192, 192, True), (192, 128, True), (128, 64, False), (64, 128, True), (128, 192, True), (192, 192, False)]
    assert TiedWeights.pairs(wide) == [(0, 5), (1, 4), (2, 3)]
    w_off = TR.flat_layout(wide)[0]
    assert TiedWeights.flat_pairs(wide, w_off) == [(w_off[0], w_off[5], 192, 192), (w_off[1], w_off[4], 128, 192), (w_off[2], w_off[3], 64, 128)]
    assert TiedWeights.free_parameter_count(wide) == 192 * 192 + 192 * 128 + 128 * 64 + sum(s[1] for s in wide)


def test_pairs_of_an_odd_stack_leave_the_middle_layer_free():
    from codae.tool import TiedWeights
    odd = [(72, 40, True), (40, 24, True), (24, 24, False), (24, 40, True), (40, 72, False)]
    assert TiedWeights.pairs(odd) == [(0, 4), (1, 3)]
    assert TiedWeights.free_parameter_count(odd) == 72 * 40 + 40 * 24 + 24 * 24 + 40 + 24 + 24 + 40 + 72
    assert TiedWeights.pairs([(8, 8, False)]) == []
    assert bool(TR.free_mask(odd)[TR.flat_layout(odd)[0][2]])           # the middle matrix is a free tensor


def test_an_asymmetric_stack_is_refused_naming_the_pair():
    from codae.hip import HipError
    from codae.tool import TiedWeights
    sched = _stack(3, 4, 64)                               # nb_input_layer != nb_output_layer, taper
    with pytest.raises(HipError) as e:
        TiedWeights.pairs(sched)
    msg = str(e.value)
    assert msg.startswith("tied weights: layers ") and "are not mirror images" in msg
    l, m = (int(v) for v in re.search(r"layers (\d+) and (\d+)", msg).groups())
    assert l + m == len(sched) - 1 and (sched[l][0] != sched[m][1] or sched[l][1] != sched[m][0])
    assert "(%d -> %d against %d -> %d)" % (sched[l][0], sched[l][1], sched[m][0], sched[m][1]) in msg
    # the library's own wording (csrc/engine.hip) is this wording
    src = open(os.path.join(ROOT, "mui-deepautoencoder_amd", "csrc", "engine.hip")).read()
    assert "tied weights: layers %d and %d are not mirror images (%d -> %d against %d -> %d)" in src


@pytest.mark.parametrize("name", ["taper", "odd", "partial"])
def test_folded_untied_gradient_is_the_shared_parameter_gradient(name):
    """Autograd through one nn.Parameter used twice (TiedModel) against TiedWeights.fold of the gradients of the same stack with a
    parameter per layer, float64: equal to rounding (one add per element: 2^-52 relative to the two terms' magnitudes)."""
    from codae.tool import TiedWeights
    sched = {"taper": [(48, 48, True), (48, 32, True), (32, 16, False), (16, 32, True), (32, 48, True), (48, 48, False)],
             "odd": [(24, 16, True), (16, 8, True), (8, 8, False), (8, 16, True), (16, 24, False)],
             "partial": [(72, 72, True), (72, 40, False), (40, 72, True), (72, 72, False)]}[name]
    params = TR.tied_init(sched, 11)
    g = torch.Generator().manual_seed(3)
    x = torch.rand((19, sched[0][0]), generator=g, dtype=torch.float64)
    fmask = (torch.rand((19, sched[0][0]), generator=g) > 0.3).to(torch.float64)
    tied, untied = TR.TiedModel(sched, params), TR.TiedModel(sched, params, tied=False)
    assert torch.equal(tied.flat_params(), untied.flat_params())
    lt, lu = tied.loss(x, fmask), untied.loss(x, fmask)
    assert float(lt.detach()) == float(lu.detach())
    lt.backward(); lu.backward()
    want, raw = tied.flat_grads(), untied.flat_grads()
    w_off = TR.flat_layout(sched)[0]
    got = TiedWeights.fold(raw, sched, w_off)
    assert got is not raw and float(raw.abs().max()) > 0
    for l, m in TiedWeights.pairs(sched):
        k, n = sched[l][0], sched[l][1]
        a, b = raw[w_off[l]:w_off[l] + n * k].view(n, k), raw[w_off[m]:w_off[m] + n * k].view(k, n)
        tol = 2.0 ** -52 * (a.abs() + b.t().abs())
        e = (got[w_off[l]:w_off[l] + n * k].view(n, k) - want[w_off[l]:w_off[l] + n * k].view(n, k)).abs()
        assert bool((e <= tol).all()), (name, l, float(e.max()))
        dec = got[w_off[m]:w_off[m] + n * k]
        assert bool((dec == 0).all()) and not bool(torch.signbit(dec).any()), (name, m)
    free = torch.from_numpy(TR.free_mask(sched))
    untouched = free.clone()
    for l, _ in TiedWeights.pairs(sched):
        untouched[w_off[l]:w_off[l] + sched[l][0] * sched[l][1]] = False
    assert torch.equal(got[untouched], raw[untouched]) and torch.equal(got[untouched], want[untouched])     # middle matrix, biases
    # the norm of the folded vector is clip_grad_norm_'s of the shared parameters
    total = torch.nn.utils.clip_grad_norm_(list(tied.parameters()), 1e9)
    assert abs(float(got.pow(2).sum().sqrt()) - float(total)) <= 1e-12 * float(total)
    # and the mirror twin rebuilds the decoder from the encoder, whatever the decoder ranges held
    p = tied.flat_params()
    junk = p.clone()
    for _, m in TiedWeights.pairs(sched):
        junk[w_off[m]:w_off[m] + sched[m][0] * sched[m][1]] = 7.0
    back = TiedWeights.mirror(junk, sched, w_off)
    assert torch.equal(back, p) and back is not junk and float(junk.max()) == 7.0


def test_fold_and_mirror_twins_keep_fp32_bits_and_take_custom_offsets():
    from codae.tool import TiedWeights
    sched = [(8, 16, True), (16, 8, False)]
    w_off = [128, 0]                                       # decoder first
    g = torch.arange(256, dtype=torch.float32) * 0.37 - 11.0
    out = TiedWeights.fold(g, sched, w_off)
    enc, dec = g[128:256].view(16, 8), g[0:128].view(8, 16)
    assert torch.equal(out[128:256].view(16, 8), enc + dec.t()) and bool((out[0:128] == 0).all())
    m = TiedWeights.mirror(g, sched, w_off)
    assert torch.equal(m[0:128].view(8, 16), enc.t()) and torch.equal(m[128:], g[128:])


def test_header_and_binding_have_the_three_new_entries():
    from codae import hip
    header = open(os.path.join(ROOT, "include", "codae_hip.h")).read()
    assert int(re.search(r"#define CODAE_ABI_VERSION (\d+)", header).group(1)) == 11 == hip.ABI_VERSION      # new entries only
    for fn, n_args in (("codae_set_tied_weights", 2), ("codae_tie_fold", 4), ("codae_tie_mirror", 6)):
        proto = re.search(r"\bint %s\s*\(([^;]*)\);" % fn, header)
        assert proto is not None and fn in hip.PROTOTYPES, fn
        assert len(proto.group(1).split(",")) == n_args == len(hip.PROTOTYPES[fn][1]), fn
    assert "/* Tied weights (" in header and "codae_tie_pair;" in header
    import ctypes as C
    assert C.sizeof(hip.TiePair) == 24 and [n for n, _ in hip.TiePair._fields_] == ["enc_off", "dec_off", "rows", "cols"]
    if os.path.exists(hip.LIB_PATH):
        lib = hip.lib()
        assert all(hasattr(lib, fn) for fn in ("codae_set_tied_weights", "codae_tie_fold", "codae_tie_mirror"))


def test_config_key_parses():
    from codae.hip import HipError
    from codae.tool import TiedWeights
    import yaml
    assert TiedWeights.from_config(yaml.safe_load("HIP: {TIED_WEIGHTS: true}")["HIP"].get("TIED_WEIGHTS")) is True
    assert TiedWeights.from_config(yaml.safe_load("HIP: {TIED_WEIGHTS: false}")["HIP"]["TIED_WEIGHTS"]) is False
    assert TiedWeights.from_config(yaml.safe_load("HIP: {PRECISION: bf16}")["HIP"].get("TIED_WEIGHTS")) is False
    for bad in ("yes please", 1, [True]):
        with pytest.raises(HipError, match="TIED_WEIGHTS"):
            TiedWeights.from_config(bad)
    src = open(os.path.join(ROOT, "mui-deepautoencoder_amd", "script", "train_dae_on_embedding.py")).read()
    assert 'get("TIED_WEIGHTS")' in src and "tied_weights=tied_weights" in src


def test_sharded_data_parallel_refuses_a_tied_engine():
    """DataParallel(sharded=True) around an engine with tying on: HipError naming the pair (no GPU, no process group needed: the
    refusal comes first)."""
    from codae.hip import HipError
    from codae.train import DataParallel

    class Eng:
        L, tied_weights = 6, True
        w_off, b_off, n_param = [0, 64, 128, 192, 256, 320], [384], 448

    with pytest.raises(HipError, match=r"tied weights: the sharded update is not supported: the tied layers 0 and 5"):
        DataParallel(Eng(), n_buckets=2, sharded=True)
    dp = DataParallel(Eng(), n_buckets=2, sharded=False)
    assert not dp.sharded
