"""The reference side of the non-finite contract, on the CPU: the helpers of nonfinite_ref.py on hand-made arrays, the
planting design's class map in three arithmetics, what torch's clipped Adam step does to a diverged model (so that the GPU
tests compare against torch and not against constants), and the oracle's clip against torch's."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import nonfinite_ref as R  # noqa: E402

nan, inf = float("nan"), float("inf")


def test_classes_on_a_hand_made_array():
    a = np.array([[0.0, -inf, inf], [nan, 3e38, -0.0]])
    assert R.classes(a).tolist() == [[0, 1, 2], [3, 0, 0]]
    assert R.classes(torch.tensor(a, dtype=torch.float32)).tolist() == [[0, 1, 2], [3, 0, 0]]
    assert R.classes(torch.tensor([nan, inf]).bfloat16()).tolist() == [3, 2]


def test_assert_same_accepts_equal_classes_and_rejects_every_swap():
    ref = np.array([1.0, nan, inf, -inf, 0.0])
    R.assert_same(ref.copy(), ref, 0, 0)
    R.assert_same(np.array([1.0 + 1e-7, nan, inf, -inf, 1e-9]), ref, 1e-6, 1e-8)
    for k, wrong in [(1, 0.0), (1, inf), (2, nan), (2, -inf), (2, 3e38), (3, inf), (0, nan), (4, -inf)]:
        got = ref.copy()
        got[k] = wrong
        with pytest.raises(AssertionError):
            R.assert_same(got, ref, 1e-3, 1e-3)
    with pytest.raises(AssertionError):                       # a 0 where the reference is NaN: what a v_max ReLU writes
        R.assert_same(np.zeros(2), np.array([nan, 0.0]), 1e-3, 1e-3)
    with pytest.raises(AssertionError):                       # finite entries out of tolerance
        R.assert_same(np.array([1.1, nan]), np.array([1.0, nan]), 1e-3, 1e-3)


def test_assert_same_allows_nan_and_only_nan_under_the_mask():
    ref = np.array([inf, -inf, 2.0, inf])
    allow = np.array([True, True, False, False])
    R.assert_same(np.array([nan, -inf, 2.0, inf]), ref, 0, 0, allow_nan_at=allow)
    with pytest.raises(AssertionError):
        R.assert_same(np.array([0.0, -inf, 2.0, inf]), ref, 0, 0, allow_nan_at=allow)     # finite is not allowed there
    with pytest.raises(AssertionError):
        R.assert_same(np.array([inf, -inf, 2.0, nan]), ref, 0, 0, allow_nan_at=allow)     # NaN outside the mask


@pytest.mark.parametrize("M,N,K", R.PLANT_SHAPES)
def test_planted_forward_has_one_class_map_in_float64_fp32_and_permuted_bf16(M, N, K):
    m64, m32, mbf, touched = R.forward_class_maps(M, N, K)
    assert np.array_equal(m64, m32) and np.array_equal(m64, mbf)
    assert not (m64[~touched] != R.FINITE).any()              # nothing outside the touched mask is non-finite
    assert not (m64[touched] == R.FINITE).any()               # nothing inside it is finite before the activation


def test_torch_activations_keep_nan_and_map_inf():
    nn = torch.nn
    v = torch.tensor([nan, inf, -inf], dtype=torch.float64)
    assert R.classes(nn.ReLU()(v)).tolist() == [3, 2, 0]
    for m in (nn.ReLU6(), nn.LeakyReLU(0.1), nn.ELU(), nn.CELU(0.7), nn.SELU(), nn.Softplus(), nn.Hardsigmoid()):
        assert R.classes(m(v))[0] == R.NAN, m


def test_plant_backward_relu_gradient_is_a_select():
    rng = np.random.default_rng(1)
    dy = rng.standard_normal((5, 4)); W = rng.standard_normal((4, 6)); h = rng.standard_normal((5, 6))
    tdx, tdw = R.plant_backward(dy, W)
    dx = R.dgrad_relu_ref(dy, W, h)
    assert (dx[h <= 0] == 0).all() and np.isnan(dx[4][h[4] > 0]).all() and np.isinf(dx[0, :5][h[0, :5] > 0]).all()
    assert not (R.classes(R.dgrad_relu_ref(dy, W))[~tdx] != 0).any()
    # torch's autograd agrees (threshold_backward selects)
    v = torch.tensor(h, requires_grad=True)
    torch.relu(v).backward(torch.tensor(R.dgrad_relu_ref(dy, W)))
    assert np.array_equal(R.classes(v.grad), R.classes(dx))
    dW, db = R.wgrad_ref(dy, rng.standard_normal((5, 6)))
    assert not (R.classes(dW)[~tdw] != 0).any() and np.isnan(dW[2]).all() and np.isinf(dW[0]).all()
    assert np.isnan(db[2]) and db[0] == inf


@pytest.mark.parametrize("scenario", R.SCENARIOS)
def test_reference_step_fp32_goes_all_nan(scenario):
    r = R.reference_step(scenario, torch.float32)
    assert not np.isfinite(r["loss"])
    assert (r["loss"] == inf) == (scenario == "S4")
    for w, b in r["params"]:
        assert np.isnan(w).all() and np.isnan(b).all()


def test_reference_step_control_is_finite_and_float64_does_not_overflow_at_3e38():
    for dtype in (torch.float32, torch.float64):
        r = R.reference_step(None, dtype)
        assert np.isfinite(r["loss"]) and all(np.isfinite(w).all() and np.isfinite(b).all() for w, b in r["params"])
    assert np.isfinite(R.reference_step("S6", torch.float64)["loss"])
    for s in ("S1", "S2", "S3", "S4", "S5"):
        assert not np.isfinite(R.reference_step(s, torch.float64)["loss"])


@pytest.mark.parametrize("case", ["nan", "inf", "overflow"])
def test_oracle_clip_grad_norm_equals_torch(case):
    from oracle import dae_oracle as O
    rng = np.random.default_rng(3)
    grads = [(rng.standard_normal((4, 3)).astype(np.float32), rng.standard_normal(4).astype(np.float32)),
             (rng.standard_normal((2, 4)).astype(np.float32), rng.standard_normal(2).astype(np.float32))]
    if case == "nan":
        grads[0][0][1, 2] = nan
    elif case == "inf":
        grads[1][1][0] = inf
    else:
        for gw, gb in grads:
            gw[:] = 3e19
            gb[:] = 3e19                                       # finite; the sum of squares is 9e38 per element: above fp32's range
    ps = [torch.nn.Parameter(torch.zeros(a.shape)) for pair in grads for a in pair]
    for p, a in zip(ps, [a for pair in grads for a in pair]):
        p.grad = torch.tensor(a.copy())
    total = torch.nn.utils.clip_grad_norm_(ps, 1.0)
    clipped, o_total = O.clip_grad_norm(grads, 1.0)
    assert np.array_equal(R.classes(np.float64(o_total)), R.classes(total))
    got = [a for pair in clipped for a in pair]
    for p, a in zip(ps, got):
        R.assert_same(a, p.grad, 1e-6, 0)
    if case == "nan":
        assert all(np.isnan(a).all() for a in got)
    elif case == "overflow":
        assert all((a == 0).all() for a in got)
