"""CPU-only tests of tests/adam_ref.py, the reference tests/test_gpu_optimizer.py holds every optimizer-update path to.

The formula: adam_step64 with clip_coef32 against float64 torch.optim.Adam after torch.nn.utils.clip_grad_norm_, five steps with
betas (0.8, 0.95), eps 1e-6, weight decay 1e-2, to 1e-12.  clip_coef32 is three fp32 operations where torch's coefficient is
float64, so on an arbitrary gradient the two coefficients differ by up to 4 u = 2.4e-7 relative (asserted below on its own) and
the parameters by lr times that.  The clipped steps therefore use gradients of norm 2^20 (to float64 rounding): sum g^2 rounds
to exactly 2^40 in fp32, its root is exact, 2^20 + 1e-6 rounds back to 2^20 and max_norm / 2^20 is exact, which leaves the 1e-6
of the denominator (9.5e-13 relative) as the only difference from torch's coefficient.

The bounds: the fp32 emulation of the kernel's arithmetic (adam_step32_emulated) must stay inside bounds() on the planted
generator with room to spare - worst |error| / bound <= 0.75 - over the hyper sets, step counts and clip coefficients of the GPU
test.  Measured: 0.50 for p, 0.41 for m, 0.37 for v.
"""
import numpy as np
import pytest
import torch

import adam_ref as AR

HYPERS = {"a": dict(lr=1e-3, wd=1e-2, betas=(0.9, 0.999), eps=1e-8),
          "b": dict(lr=3e-2, wd=0.0, betas=(0.8, 0.95), eps=1e-6),
          "c": dict(lr=1e-5, wd=1e-4, betas=(0.9, 0.999), eps=1e-8)}
STEPS = (1, 2, 7, 1000)
SHAPES = [(136, 192), (72, 136), (40, 72), (4099,), (1,), (5,)]


def test_clip_coef32_is_the_float64_coefficient_to_fp32_rounding():
    rng = np.random.default_rng(5)
    for _ in range(200):
        gsq = float(10.0 ** rng.uniform(-12, 12))
        max_norm = float(np.float32(10.0 ** rng.uniform(-3, 3)))
        want = min(1.0, max_norm / (np.sqrt(gsq) + 1e-6))
        got = AR.clip_coef32(gsq, max_norm)
        assert got.dtype == np.float32 and abs(float(got) - want) <= 4 * AR.U * want, (gsq, max_norm)
    assert AR.clip_coef32(123.0, 0.0) == 1 and AR.clip_coef32(123.0, -1.0) == 1
    assert AR.clip_coef32(0.0, 1.0) == 1 and AR.clip_coef32(float("inf"), 1.0) == 0
    assert np.isnan(AR.clip_coef32(float("nan"), 1.0))            # (torch.clamp(max=1) of a NaN: NaN)


def test_adam_step64_with_clip_coef32_is_torch_adam_after_clip_grad_norm():
    lr, wd, betas, eps, max_norm = 1e-2, 1e-2, (0.8, 0.95), 1e-6, 1.0
    rng = np.random.default_rng(11)
    n = 257
    p32 = rng.standard_normal(n).astype(np.float32)
    ref = torch.nn.Parameter(torch.tensor(p32.astype(np.float64)))
    # torch's float64 Adam takes the hyperparameters the struct holds: the fp32 values, widened
    h1 = AR.hyper(lr, wd, betas, eps, 1)
    opt = torch.optim.Adam([ref], lr=h1.lr, betas=(h1.b1, h1.b2), eps=h1.eps, weight_decay=h1.wd)
    p, m, v = p32.astype(np.float64), np.zeros(n), np.zeros(n)
    branches = []
    for t in range(1, 6):
        g = rng.standard_normal(n)
        g *= (2.0 ** 20 if t % 2 else 0.25) / np.linalg.norm(g)          # clipped on the odd steps, untouched on the even ones
        ref.grad = torch.tensor(g)
        total = float(torch.nn.utils.clip_grad_norm_([ref], max_norm))
        opt.step()
        coef = AR.clip_coef32(float((g * g).sum()), max_norm)
        assert abs(total - np.linalg.norm(g)) <= 1e-12 * total
        branches.append(bool(coef < 1))
        p, m, v = AR.adam_step64(p, g, m, v, AR.hyper(lr, wd, betas, eps, t), coef)           # (float64 state carried on)
        err = float(np.abs(p - ref.detach().numpy()).max())
        print("step %d coef %.9g  max |p - torch| %.3g" % (t, float(coef), err))
        assert err <= 1e-12, t
    assert branches == [True, False, True, False, True]


def test_the_emulated_fp32_update_stays_inside_the_bounds():
    worst = np.zeros(3)
    for name, hy in sorted(HYPERS.items()):
        for t in STEPS:
            state = AR.planted_state(SHAPES, 100 + t, t == 1, hy["wd"])
            h = AR.hyper(hy["lr"], hy["wd"], hy["betas"], hy["eps"], t)
            for coef in (1.0, 0.0123):
                for s in state:
                    args = (s["p"], s["g"], s["m"], s["v"], h, np.float32(coef))
                    r = AR.worst_ratios(AR.adam_step32_emulated(*args), AR.adam_step64(*args), AR.bounds(*args)[:3])
                    worst = np.maximum(worst, r)
    print("MEASURE emulation worst |error| / bound: p %.3f  m %.3f  v %.3f" % tuple(worst))
    assert np.isfinite(worst).all() and worst.max() <= 0.75, worst


def test_the_planted_state_has_what_it_promises():
    wd = 1e-2
    s = AR.planted_state([(136, 192)], 7, False, wd)[0]
    p, g, m, v = (s[k].reshape(-1).astype(np.float64) for k in "pgmv")
    assert (g[::7] == 0).all() and (v >= 0).all() and (v > 0).any()
    lg = np.log10(np.abs(g[g != 0]))
    assert lg.min() < -8 and lg.max() > 4 and np.log10(np.abs(p)).min() < -3.5 and np.log10(np.abs(p)).max() > 2
    i = np.arange(0, g.size, 11)
    i = i[i % 7 != 0]
    cancel = np.abs(g[i] + AR.hyper(0, wd).wd * p[i]) / np.abs(g[i])
    assert cancel.max() < 8e-3 and cancel.min() < 1e-6                 # (decay against gradient: at most 7e-3 of either survives)
    z = AR.planted_state([(5,), (64, 64)], 7, True, wd)
    assert all((t["m"] == 0).all() and (t["v"] == 0).all() for t in z) and z[1]["p"].shape == (64, 64)
    again = AR.planted_state([(136, 192)], 7, False, wd)[0]
    assert all(np.array_equal(s[k], again[k]) for k in "pgmv")
