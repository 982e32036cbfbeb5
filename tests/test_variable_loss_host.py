"""codae.tool.VariableLoss on the host: its torch statement of the mixed-variable criterion and its autograd against the oracle's
combined_mean / combined_mean_grad_y (the reference's CombinedCriterion(reduction="mean"), metering.py:155-180), predict, the
constructor's validation, and the exactly reconstructed regression variable (0 * inf = NaN, as torch's autograd of sqrt(mse))."""
import numpy as np
import pytest

from golden_util import Golden, close
from oracle import dae_oracle as O

torch = pytest.importorskip("torch")

# io 56: one-hots of 2, 3 and 40 columns, regressions of 1, 5 and 5
ARCH_B = [{"position": 0, "size": 2, "type": "classification"}, {"position": 2, "size": 1, "type": "regression"},
          {"position": 3, "size": 3, "type": "classification"}, {"position": 6, "size": 5, "type": "regression"},
          {"position": 11, "size": 40, "type": "classification"}, {"position": 51, "size": 5, "type": "regression"}]
WEIGHT_B = [0.5, 1.0, 2.0, 0.25, 1.5, 1.0]


def rows_for(arch, B, seed):
    """Clean rows (one-hot in the classification variables, uniform elsewhere) and an output of the same shape."""
    rng = np.random.default_rng(seed)
    io = arch[-1]["position"] + arch[-1]["size"]
    x = rng.random((B, io), dtype=np.float32)
    for v in arch:
        if v["type"] == "classification":
            p, s = v["position"], v["size"]
            x[:, p:p + s] = 0
            x[np.arange(B), p + rng.integers(0, s, B)] = 1
    y = (x + rng.normal(0, 0.5, (B, io))).astype(np.float32)
    return x, y


def _cases():
    g = Golden("abalone_k2")
    return [("abalone", g.meta["arch"], g.meta["weight"]), ("synthetic", ARCH_B, WEIGHT_B)]


@pytest.mark.parametrize("name,arch,weight", _cases(), ids=[c[0] for c in _cases()])
def test_loss_and_autograd_match_the_oracle(name, arch, weight):
    from codae.tool import VariableLoss
    vl = VariableLoss(arch, weight)
    for B in (1, 7, 64):
        x, y = rows_for(arch, B, 3 + B)
        ty = torch.tensor(y, requires_grad=True)
        loss = vl.loss(torch.tensor(x), ty)
        loss.backward()
        assert close(loss.item(), O.combined_mean(arch, weight, x, y)), (name, B)
        assert close(ty.grad.numpy(), O.combined_mean_grad_y(arch, weight, x, y)), (name, B)


def test_default_weight_is_one_and_struct_carries_the_table():
    from codae import hip
    from codae.tool import VariableLoss
    vl = VariableLoss(ARCH_B)
    assert vl.n_var == 6 and vl.io == 56 and np.array_equal(vl.weight, np.ones(6, dtype=np.float32))
    x, y = rows_for(ARCH_B, 9, 0)
    assert close(vl.loss(torch.tensor(x), torch.tensor(y)).item(), O.combined_mean(ARCH_B, [1] * 6, x, y))
    st = VariableLoss(ARCH_B, WEIGHT_B).as_struct()
    assert st.n_var == 6 and st.reserved == 0 and not st.ws and st.ws_bytes == 0
    assert [st.position[i] for i in range(6)] == [v["position"] for v in ARCH_B]
    assert [st.size[i] for i in range(6)] == [v["size"] for v in ARCH_B]
    assert [st.type[i] for i in range(6)] == [hip.VAR_CLASSIFICATION if v["type"] == "classification" else hip.VAR_REGRESSION for v in ARCH_B]
    assert [st.weight[i] for i in range(6)] == [float(np.float32(w)) for w in WEIGHT_B]


def test_predict():
    from codae.tool import VariableLoss
    vl = VariableLoss(ARCH_B, WEIGHT_B)
    _, y = rows_for(ARCH_B, 5, 1)
    out = vl.predict(torch.tensor(y))
    assert len(out) == 6
    for v, o in zip(ARCH_B, out):
        ys = y[:, v["position"]:v["position"] + v["size"]]
        if v["type"] == "regression":
            assert np.array_equal(o.numpy(), ys)
        else:
            idx, prob = o
            assert np.array_equal(idx.numpy(), ys.argmax(axis=1))
            assert np.allclose(prob.numpy(), np.exp(O._log_softmax(ys)), rtol=1e-5, atol=1e-7)
            assert np.allclose(prob.numpy().sum(axis=1), 1.0, atol=1e-6)


def test_constructor_refuses_bad_tables():
    from codae.hip import HipError
    from codae.tool import VariableLoss

    def arch(*triples):
        return [{"position": p, "size": s, "type": t} for p, s, t in triples]
    r, c = "regression", "classification"
    with pytest.raises(HipError, match="overlaps"):
        VariableLoss(arch((0, 3, c), (2, 1, r)))
    with pytest.raises(HipError, match="covered by no variable"):
        VariableLoss(arch((0, 3, c), (4, 1, r)))
    with pytest.raises(HipError, match="covered by no variable"):
        VariableLoss(arch((1, 3, c)))
    with pytest.raises(HipError, match="size"):
        VariableLoss(arch((0, 0, r)))
    with pytest.raises(HipError, match="unknown type"):
        VariableLoss(arch((0, 1, "continuous")))
    with pytest.raises(HipError, match="non-empty"):
        VariableLoss([])
    with pytest.raises(HipError, match="needs position"):
        VariableLoss([{"size": 1, "type": r}])
    for bad in ([1.0, -0.5], [1.0, float("nan")], [1.0, float("inf")]):
        with pytest.raises(HipError, match="finite and >= 0"):
            VariableLoss(arch((0, 3, c), (3, 1, r)), bad)
    with pytest.raises(HipError, match="weights for"):
        VariableLoss(arch((0, 3, c), (3, 1, r)), [1.0])
    with pytest.raises(HipError, match=r"not \[B, 4\]"):
        VariableLoss(arch((0, 3, c), (3, 1, r))).loss(torch.zeros(2, 5), torch.zeros(2, 5))


def test_exactly_reconstructed_regression_variable_is_nan_as_in_torch():
    """sqrt(mse) at 0 has the derivative inf, times the mse's 0: NaN in every column of that variable, finite elsewhere."""
    from codae.tool import VariableLoss
    vl = VariableLoss(ARCH_B, WEIGHT_B)
    x, y = rows_for(ARCH_B, 6, 2)
    y[:, 6:11] = x[:, 6:11]
    ty = torch.tensor(y, requires_grad=True)
    vl.loss(torch.tensor(x), ty).backward()
    got = ty.grad.numpy()
    # the reference expression for that variable alone (metering.py:165-167)
    ry = torch.tensor(y[:, 6:11], requires_grad=True)
    torch.sqrt(torch.nn.MSELoss(reduction="mean")(input=torch.tensor(x[:, 6:11]), target=ry)).backward()
    assert np.isnan(ry.grad.numpy()).all()
    assert np.isnan(got[:, 6:11]).all()
    keep = np.ones(56, dtype=bool); keep[6:11] = False
    assert np.isfinite(got[:, keep]).all()
    assert close(got[:, keep], O.combined_mean_grad_y(ARCH_B, WEIGHT_B, x, np.where(keep, y, y + 1))[:, keep])
