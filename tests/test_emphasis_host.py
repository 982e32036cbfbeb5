"""CPU-only tests of the emphasised denoising loss (include/codae_hip.h, "Emphasised denoising loss"): codae.tool.LossEmphasis
validation and config parsing, LossEmphasis.loss and its autograd gradient against tests/emphasis_ref.py, the plain MSE at
alpha = beta = 1, and the data-parallel property of the weights."""
import numpy as np
import pytest
import torch

import emphasis_ref as ER

MASKING = ("masking", dict(p=0.25), ER.SEED)
ALPHA, BETA, SLOT_W = 3.0, 0.5, (0.5, 1.0, 2.0)


def _case():
    """B = 33, io = 24, S = 3, step 5, MASKING(0.25): (x, y, keep, rows, corrupted)."""
    p = ER.problem(24)
    x = p["data"][p["rows"]]
    keep = p["table"][p["mask_id"]]
    return p, x, p["y"], keep, ER.corrupted(keep, p["rows"], 5, MASKING)


def test_the_fixture_discriminates_b33_io24():
    """The inputs every tolerance below relies on: blank and noise each touch a large share, many elements are replaced but
    not blanked, and the weighted loss is far from both the unweighted one and the one that ignores the noise."""
    p, x, y, keep, corr = _case()
    blank = keep == 0
    rep = ER.replaced(p["rows"], 24, 5, MASKING)
    print("blank %.2f replaced %.2f corrupted %.2f replaced-not-blank %d" % (blank.mean(), rep.mean(), corr.mean(), (rep & ~blank).sum()))
    assert abs(blank.mean() - 1 / 3) < 1e-9 and 0.15 < rep.mean() < 0.35 and (rep & ~blank).sum() > 100
    cw = np.repeat(np.float32(SLOT_W), 8)
    inv_n = 1.0 / x.size
    full = ER.loss_terms(x, y, keep, ER.weights(corr, ALPHA, BETA, cw), inv_n)["loss"]
    plain = ER.loss_terms(x, y, keep, ER.weights(corr, 1, 1), inv_n)["loss"]
    no_noise = ER.loss_terms(x, y, keep, ER.weights(blank, ALPHA, BETA, cw), inv_n)["loss"]
    no_blank = ER.loss_terms(x, y, keep, ER.weights(rep, ALPHA, BETA, cw), inv_n)["loss"]
    print("weighted %.4f unweighted %.4f ignoring the noise %.4f ignoring the blank %.4f" % (full, plain, no_noise, no_blank))
    for other in (plain, no_noise, no_blank):
        assert abs(full - other) > 0.1 * full


def test_validation():
    from codae.hip import HipError
    from codae.tool import LossEmphasis
    e = LossEmphasis()
    assert (e.alpha, e.beta, e.slot_weight, e.column_weight) == (1.0, 1.0, None, None) and e.is_identity
    e = LossEmphasis(alpha=3, beta=0.1, slot_weight=[0.5, 1, 2])
    assert e.alpha == 3.0 and e.beta == float(np.float32(0.1)) and e.slot_weight == (0.5, 1.0, 2.0) and not e.is_identity
    assert not LossEmphasis(column_weight=[1.0] * 4).is_identity
    assert LossEmphasis(alpha=0.0, beta=1.0).alpha == 0.0
    for kw, word in [(dict(alpha=-1.0), "alpha"), (dict(beta=float("nan")), "beta"), (dict(alpha=float("inf")), "alpha"),
                     (dict(alpha=0.0, beta=0.0), "alpha \\+ beta"), (dict(alpha="3"), "alpha"), (dict(beta=True), "beta"),
                     (dict(slot_weight=[1, 2], column_weight=[1, 2]), "not both"), (dict(slot_weight=[1.0, -2.0]), "slot_weight\\[1\\]"),
                     (dict(column_weight=[float("nan")]), "column_weight\\[0\\]"), (dict(slot_weight=[]), "empty"),
                     (dict(slot_weight=2.0), "sequence"), (dict(column_weight="12"), "sequence")]:
        with pytest.raises(HipError, match=word):
            LossEmphasis(**kw)
    # expansion to columns, once the number of slots is known
    np.testing.assert_array_equal(LossEmphasis(slot_weight=[0.5, 1, 2]).column_weights(6, 3), np.float32([0.5, 0.5, 1, 1, 2, 2]))
    np.testing.assert_array_equal(LossEmphasis(column_weight=[1, 2, 3]).column_weights(3), np.float32([1, 2, 3]))
    assert LossEmphasis(alpha=2).column_weights(6, 3) is None
    with pytest.raises(HipError, match="2 slot weights for 3 slots"):
        LossEmphasis(slot_weight=[1, 2]).column_weights(6, 3)
    with pytest.raises(HipError, match="do not divide"):
        LossEmphasis(slot_weight=[1, 2]).column_weights(7)
    with pytest.raises(HipError, match="3 column weights for 4 columns"):
        LossEmphasis(column_weight=[1, 2, 3]).column_weights(4)


def test_config_block():
    from codae.hip import HipError
    from codae.tool.emphasis import loss_emphasis_from_config
    assert loss_emphasis_from_config(None) is None and loss_emphasis_from_config({}) is None
    e = loss_emphasis_from_config({"ALPHA": 3.0, "BETA": 1.0, "SLOT_WEIGHT": [0.5, 1, 2]})
    assert (e.alpha, e.beta, e.slot_weight, e.column_weight) == (3.0, 1.0, (0.5, 1.0, 2.0), None)
    e = loss_emphasis_from_config({"COLUMN_WEIGHT": [1, 2]})
    assert (e.alpha, e.beta, e.column_weight) == (1.0, 1.0, (1.0, 2.0))
    for block, word in [({"ALPHA": 3.0, "GAMMA": 1.0}, "unknown key\\(s\\) GAMMA"), ({"alpha": 3.0}, "unknown key"),
                        ([3.0, 1.0], "must be a mapping"), ({"ALPHA": -3.0}, "alpha"),
                        ({"SLOT_WEIGHT": [1], "COLUMN_WEIGHT": [1]}, "not both")]:
        with pytest.raises(HipError, match=word):
            loss_emphasis_from_config(block)


@pytest.mark.parametrize("form", ["slot", "column", "none"])
def test_loss_and_autograd_gradient_match_the_definition_b33_io24(form):
    """fp32 torch against the float64 reference: every product and the subtraction round once (dy: at most five roundings,
    rtol 1e-6), the loss is a sum of B io non-negative fp32 terms (relative B io 2^-24)."""
    from codae.tool import LossEmphasis
    p, x, y, keep, corr = _case()
    cw = {"slot": np.repeat(np.float32(SLOT_W), 8), "column": np.linspace(0.0, 2.0, 24).astype(np.float32), "none": None}[form]
    e = LossEmphasis(ALPHA, BETA, slot_weight=SLOT_W if form == "slot" else None, column_weight=None if form != "column" else list(cw))
    ref = ER.loss_terms(x, y, keep, ER.weights(corr, ALPHA, BETA, cw), 1.0 / x.size)
    out = torch.tensor(y, requires_grad=True)
    loss = e.loss(torch.tensor(x), out, torch.tensor(keep).float(), corrupted=torch.tensor(corr))
    loss.backward()
    assert abs(float(loss.detach()) - ref["loss"]) <= x.size * 2.0 ** -24 * ref["loss"], (float(loss.detach()), ref["loss"])
    np.testing.assert_allclose(out.grad.numpy().astype(np.float64), ref["dy"], rtol=1e-6, atol=0)
    # corrupted defaults to 1 - fmask: the blank alone
    ref_blank = ER.loss_terms(x, y, keep, ER.weights(keep == 0, ALPHA, BETA, cw), 1.0 / x.size)
    got = float(e.loss(torch.tensor(x), torch.tensor(y), torch.tensor(keep).float()))
    assert abs(got - ref_blank["loss"]) <= x.size * 2.0 ** -24 * ref_blank["loss"]
    assert abs(got - ref["loss"]) > 0.05 * ref["loss"]


def test_alpha_beta_one_without_weights_is_the_mean_squared_error():
    from codae.tool import LossEmphasis
    p, x, y, keep, corr = _case()
    a, b = torch.tensor(x), torch.tensor(y)
    got = LossEmphasis().loss(a, b, torch.tensor(keep).float(), corrupted=torch.tensor(corr))
    want = torch.nn.MSELoss(reduction="mean")(b, a)
    assert abs(float(got) - float(want)) <= 4 * 2.0 ** -24 * float(want)        # (sum / n against mean: the last bits)
    assert float(ER.loss_terms(x, y, keep, ER.weights(corr, 1, 1), 1.0 / x.size)["loss"]) == pytest.approx(float(want), rel=1e-6)


def test_half_batch_gradients_add_up_to_the_full_batch_gradient():
    """w depends on (dataset row, column, step, seed) only and inv_n is the GLOBAL batch's: two data-parallel ranks' gradients
    sum to the one-process gradient (each element's gradient is computed once on either side: bit for bit)."""
    from codae.tool import LossEmphasis
    p, x, y, keep, _ = _case()
    e = LossEmphasis(ALPHA, BETA, slot_weight=SLOT_W)
    rows = p["rows"]

    def grad(sel):
        out = torch.tensor(y[sel], requires_grad=True)
        corr = ER.corrupted(keep[sel], rows[sel], 5, MASKING)              # from the shard's own dataset rows
        e.loss(torch.tensor(x[sel]), out, torch.tensor(keep[sel]).float(), corrupted=torch.tensor(corr), global_rows=len(x)).backward()
        return out.grad.numpy()

    full = grad(np.arange(len(x)))
    halves = np.empty_like(full)
    for r in (0, 1):
        halves[r::2] = grad(np.arange(r, len(x), 2))
    np.testing.assert_array_equal(halves, full)
    ref = ER.loss_terms(x, y, keep, ER.weights(ER.corrupted(keep, rows, 5, MASKING), ALPHA, BETA, np.repeat(np.float32(SLOT_W), 8)), 1.0 / x.size)
    np.testing.assert_allclose(full.astype(np.float64), ref["dy"], rtol=1e-6, atol=0)
