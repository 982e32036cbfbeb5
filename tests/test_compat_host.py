"""Assembled outfits and compatibility without a GPU: the host forms of codae.tool.Compatibility against the per-pair float64 reference
(tests/compat_ref.py), the negatives' contract, the config key, the static contract (header, binding) and a design built by hand whose
AUC is exactly 1 (0 with the weights negated)."""
import os
import re

import numpy as np
import pytest

import compat_ref as R

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(S=3, E=8, N=23, Q=11, seed=0, with_presence=True):
    rng = np.random.default_rng(seed)
    data = rng.standard_normal((N, S * E)).astype(np.float32)
    items = rng.integers(0, N, (Q, S)).astype(np.int32)
    items[1] = 5                                   # one dataset row as it is
    items[2] = [5, -1, 5][:S]                      # ... repeated, with a missing slot
    items[3] = -1
    items[4, 1:] = -7
    presence = None
    if with_presence:
        presence = (rng.random((N, S)) > 0.25).astype(np.uint8)
        data[np.repeat(presence == 0, E, axis=1)] = np.nan      # selection: an absent slot's data is never read
    blank = rng.integers(-1, S, Q).astype(np.int32)
    return data, items, presence, blank


@pytest.mark.parametrize("with_presence", [False, True])
@pytest.mark.parametrize("form", ["none", "blank", "loo"])
def test_assemble_equals_the_reference_exactly(with_presence, form):
    from codae.tool import Compatibility
    data, items, presence, blank = _case(with_presence=with_presence)
    kw = {"blank": blank} if form == "blank" else ({"leave_one_out": True} if form == "loo" else {})
    ref = R.assemble(data, items, 3, presence=presence, **kw)
    tkw = {k: (torch.tensor(v) if k == "blank" else v) for k, v in kw.items()}
    got = Compatibility.assemble(torch.tensor(data), torch.tensor(items), presence=presence, **tkw)
    assert got.dtype == torch.float32 and got.numpy().tobytes() == ref.tobytes()
    assert not np.isnan(ref).any() and np.isnan(data).any() == with_presence      # (no NaN of an absent slot is ever selected)
    # the bf16 image assembles into the image's rows
    img = torch.tensor(data).to(torch.bfloat16)
    got16 = Compatibility.assemble(img, torch.tensor(items), presence=presence, **tkw)
    ref16 = R.assemble(img.view(torch.int16).numpy(), items, 3, presence=presence, **kw)
    assert got16.dtype == torch.bfloat16 and got16.view(torch.int16).numpy().tobytes() == ref16.tobytes()


def test_a_present_nan_is_copied():
    from codae.tool import Compatibility
    data, items, _, _ = _case(with_presence=False)
    data[5, 3] = np.nan
    got = Compatibility.assemble(torch.tensor(data), torch.tensor(items)).numpy()
    assert np.isnan(got[1, 3]) and got.tobytes() == R.assemble(data, items, 3).tobytes()


@pytest.mark.parametrize("with_presence", [False, True])
@pytest.mark.parametrize("E", [8, 24, 64])
def test_slot_scores_within_the_fp32_bound(with_presence, E):
    from codae.tool import Compatibility
    data, items, presence, _ = _case(E=E, with_presence=with_presence, seed=E)
    Q, S = items.shape
    rng = np.random.default_rng(1)
    X = R.assemble(np.nan_to_num(data), items, S, leave_one_out=True, presence=presence)
    Y = (X + 0.3 * rng.standard_normal(X.shape)).astype(np.float32)
    Y[7 * S + 0] = np.nan                          # a NaN reconstruction propagates into the outfit's score
    cos, sq, score, n = R.slot_scores(data, items, Y, S, presence=presence)
    got = Compatibility.slot_scores(torch.tensor(data), torch.tensor(items), torch.tensor(Y), presence=presence)
    bound = (E + 8) * 2.0 ** -23
    assert np.array_equal(got["n_present"].numpy(), n)
    assert np.array_equal(np.isnan(got["cos"].numpy()), np.isnan(cos)) and np.array_equal(np.isnan(got["score"].numpy()), np.isnan(score))
    assert np.nanmax(np.abs(got["cos"].numpy() - cos)) <= bound
    assert np.all(np.abs(got["sq"].numpy() - sq)[~np.isnan(sq)] <= bound * sq[~np.isnan(sq)])
    assert (n < 2).any() and np.isnan(score[n < 2]).all() and (got["cos"].numpy()[3] == 0).all()
    # the score is the fp32 mean of the form's own cosines in ascending slot order
    c32 = got["cos"].numpy()
    for q in range(Q):
        if n[q] >= 2:
            acc = np.float32(0)
            for s in range(S):
                if R.present(items, q, s, len(data), presence):
                    acc = np.float32(acc + c32[q, s])
            want = np.float32(acc / np.float32(n[q]))
            assert got["score"].numpy()[q].tobytes() == want.tobytes() or (np.isnan(want) and np.isnan(got["score"].numpy()[q]))


@pytest.mark.parametrize("P,M", [(37, 53), (300, 500), (1, 1)])
def test_auc_counts_equal_the_reference_exactly(P, M):
    from codae.tool import Compatibility
    S = 4
    pos, neg, neg_slot, neg_parent = R.tricky_scores(P, M, S, seed=P, empty_slot=2)
    pos_on = (np.random.default_rng(2).random(P) > 0.2).astype(np.uint8)
    for on in (None, pos_on):
        ref = R.auc_counts(pos, neg, neg_slot, S, neg_parent, on)
        assert np.array_equal(R.auc_counts_fast(pos, neg, neg_slot, S, neg_parent, on), ref)
        assert np.array_equal(R.auc_counts_fast(pos, neg, neg_slot, S, None, on)[:, :3], R.auc_counts(pos, neg, neg_slot, S, None, on)[:, :3])
        got = Compatibility.auc(torch.tensor(pos), torch.tensor(neg), torch.tensor(neg_slot), S, neg_parent=torch.tensor(neg_parent),
                                pos_on=None if on is None else torch.tensor(on))
        assert got.dtype == torch.int64 and np.array_equal(got.numpy(), ref)
    if P > 1:
        assert np.isnan(pos).any() and np.isnan(neg).any() and np.isinf(pos).any() and ref[:S, R.TIES].sum() > 0
    out = Compatibility.summary(got, skipped=3)
    auc, paired = R.auc_of(ref)
    assert out["pairs"] == ref[:S, R.PAIRS].sum() and out["skipped"] == 3 and out["outfits"] == ref[S, 0]
    assert (np.isnan(auc) and np.isnan(out["auc"])) or out["auc"] == auc
    assert (np.isnan(paired) and np.isnan(out["paired_acc"])) or out["paired_acc"] == paired
    assert out["per_slot"][2]["pairs"] == 0 and np.isnan(out["per_slot"][2]["auc"])      # a slot nothing was swapped in: NaN, no fault


def _dup_dataset(seed=0, N=40, S=3, E=4):
    """duplicated items: slot 0 holds only 5 distinct vectors, slot 2 a single one"""
    rng = np.random.default_rng(seed)
    data = rng.standard_normal((N, S * E)).astype(np.float32)
    data[:, :E] = data[rng.integers(0, 5, N), :E]
    data[:, 2 * E:] = data[0, 2 * E:]
    presence = (rng.random((N, S)) > 0.3).astype(np.uint8)
    presence[:4] = [[1, 0, 0], [0, 0, 0], [1, 1, 1], [0, 1, 0]]
    return data, presence


@pytest.mark.parametrize("distinct", [True, False])
def test_negatives_contract(distinct):
    from codae.tool import Compatibility
    data, presence = _dup_dataset()
    N, S, E = 40, 3, 4
    val = list(range(0, N, 1))[:30]
    ds = R.Dataset(data, S)
    t = Compatibility.negatives(ds, val, negatives=4, seed=7, presence=presence, distinct=distinct)
    t2 = Compatibility.negatives(ds, val, negatives=4, seed=7, presence=presence, distinct=distinct)
    t3 = Compatibility.negatives(ds, val, negatives=4, seed=8, presence=presence, distinct=distinct)
    for k in ("rows", "pos_items", "neg_items", "neg_slot", "neg_parent"):
        assert torch.equal(t[k], t2[k])
    assert t["skipped"] == t2["skipped"] and not torch.equal(t["neg_items"], t3["neg_items"])
    n_r = presence[val].sum(1)
    rows = t["rows"].numpy()
    assert list(rows) == [r for r in val if presence[r].sum() >= 2] and 0 not in rows and 1 not in rows and 3 not in rows
    P, J = t["neg_slot"].shape
    drawn = 0
    for p in range(P):
        r = int(rows[p])
        assert list(t["pos_items"][p].numpy()) == [r if presence[r, s] else -1 for s in range(S)]
        for j in range(J):
            s = int(t["neg_slot"][p, j])
            neg = t["neg_items"][p, j].numpy()
            if s < 0:
                assert (neg == -1).all()
                continue
            drawn += 1
            assert int(t["neg_parent"][p, j]) == p and presence[r, s]
            diff = np.nonzero(neg != t["pos_items"][p].numpy())[0]
            assert list(diff) == [s]                                   # exactly one slot differs
            d = int(neg[s])
            assert d in val and presence[d, s] and d != r
            if distinct:
                assert data[d, s * E:(s + 1) * E].tobytes() != data[r, s * E:(s + 1) * E].tobytes()
    assert drawn > 0
    assert t["skipped"] == int((n_r < 2).sum()) + P * J - drawn
    if distinct:
        assert not (t["neg_slot"] == 2).any()          # a slot with a single distinct item yields no negative
    else:
        assert (t["neg_slot"] == 2).any()


def test_negatives_pick_every_slot_and_many_donors():
    from codae.tool import Compatibility
    rng = np.random.default_rng(0)
    data = rng.standard_normal((50, 12)).astype(np.float32)
    t = Compatibility.negatives(R.Dataset(data, 3), range(50), negatives=8, seed=0)
    assert t["skipped"] == 0 and set(t["neg_slot"].reshape(-1).tolist()) == {0, 1, 2}
    donors = t["neg_items"].reshape(-1, 3).gather(1, t["neg_slot"].reshape(-1, 1).long()).reshape(-1)
    assert len(set(donors.tolist())) > 40


def test_config_block():
    from codae.hip import HipError
    from codae.tool import compatibility_from_config
    assert compatibility_from_config(None) is None
    assert compatibility_from_config({}) == {"negatives": 1, "seed": 0, "distinct": True}
    assert compatibility_from_config({"NEGATIVES": 3, "SEED": 5, "DISTINCT": False}) == {"negatives": 3, "seed": 5, "distinct": False}
    for bad in ({"NEGATIVE": 1}, {"NEGATIVES": 0}, {"NEGATIVES": -2}, {"NEGATIVES": 1.5}, {"NEGATIVES": True}, {"SEED": "a"}, {"SEED": 1.0},
                {"DISTINCT": 1}, {"DISTINCT": "yes"}, [1], "x"):
        with pytest.raises(HipError):
            compatibility_from_config(bad)


def test_header_and_binding():
    from codae import hip
    header = open(os.path.join(ROOT, "include", "codae_hip.h")).read()
    assert re.search(r"#define CODAE_ABI_VERSION 11\b", header) and hip.ABI_VERSION == 11
    assert "Assembled outfits and compatibility" in header
    for name in ("codae_assemble_outfits", "codae_outfit_scores", "codae_auc_blocks", "codae_auc_counts", "codae_score_outfits"):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m, name
        assert name in hip.PROTOTYPES and len(hip.PROTOTYPES[name][1]) == m.group(1).count(",") + 1, name
    for k in ("WINS", "TIES", "PAIRS", "PAIRED", "STRIDE"):
        assert int(re.search(r"#define CODAE_AUC_%s (\d+)" % k, header).group(1)) == getattr(hip, "AUC_" + k) == getattr(R, k)
    assert float(re.search(r"#define CODAE_COS_EPS ([0-9.e-]+)f", header).group(1)) == R.COS_EPS
    makefile = open(os.path.join(ROOT, "mui-deepautoencoder_amd", "csrc", "Makefile")).read()
    assert "compat.hip" in re.search(r"^SRCS := (.*)$", makefile, re.M).group(1).split()


@pytest.mark.parametrize("sign,want", [(1.0, 1.0), (-1.0, 0.0)])
def test_orthogonal_design_has_auc_one(sign, want):
    """The hand-built design, verified in the reference first, then through the host forms and CompatibilityMetrics on the CPU."""
    from codae.tool import Compatibility, CompatibilityMetrics
    d = R.orthogonal_design()
    S, N = d["S"], d["N"]
    data32 = d["data"].astype(np.float32)
    ds = R.Dataset(data32, S)
    val = list(range(N))
    cm = CompatibilityMetrics(ds, val, "cpu", negatives=2, seed=0)
    t = cm.table
    assert t["skipped"] == 0 and len(t["rows"]) == N
    items = np.concatenate([t["pos_items"].numpy(), t["neg_items"].numpy().reshape(-1, S)])
    # the reference's own numbers first
    Y = R.design_forward(d, R.assemble(d["data"], items, S, leave_one_out=True), sign)
    cos, _, score, _ = R.slot_scores(d["data"], items, Y, S)
    assert np.abs(sign * cos[:N] - 1).max() < 1e-12
    neg_ref = score[N:]
    x0 = d["data"][:, :d["E"]]
    for j in (0, 17, 99):
        slot = int(t["neg_slot"].reshape(-1)[j])
        a, b = x0[int(items[N + j][slot])], x0[int(t["rows"][int(t["neg_parent"].reshape(-1)[j])])]
        assert abs(neg_ref[j] - sign * (a @ b) / np.sqrt((a @ a) * (b @ b))) < 1e-12
    assert (sign * neg_ref).max() < 0.99
    c = R.auc_counts(score[:N], neg_ref, t["neg_slot"].reshape(-1).numpy(), S, t["neg_parent"].reshape(-1).numpy())
    assert R.auc_of(c) == (want, want)
    # ... then the host forms in fp32, in two batches
    for rows in (val[:40], val[40:]):
        pl = cm.places(rows)
        it = torch.cat([cm.pos_items[pl], cm.neg_items[pl].reshape(-1, S)])
        X = Compatibility.assemble(torch.tensor(data32), it, leave_one_out=True)
        Yt = torch.tensor(R.design_forward(d, X.numpy(), sign).astype(np.float32))
        sc = Compatibility.slot_scores(torch.tensor(data32), it, Yt)["score"]
        cm.add(sc[:len(rows)], sc[len(rows):].reshape(len(rows), 2), pl)
    out = cm.get()
    assert out["auc"] == want and out["paired_acc"] == want and out["outfits"] == N and out["pairs"] == N * 2 * N
    assert cm.total()["auc"] == want and cm.total()["outfits"] == 0          # (total() reset the stored batch)
