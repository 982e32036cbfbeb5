"""Retrieval metrics without a GPU: RetrievalMetrics.get (the whole-tensor torch form) against the per-pair numpy reference on a
design whose positions are exact, its agreement with RankingLoss where the two definitions coincide, and the static contract
(header, binding, config key)."""
import os
import re

import numpy as np
import pytest

import retrieval_metrics_ref as R

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 5, 10, 50)


def _check_block(got, ref):
    """every integer field ==, the two sums to 1e-12 relative"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape
    for f in [R.PAIRS] + list(range(R.HIT, R.HIT + R.MAX_KS)) + list(range(R.HIST, R.HIST + 32)):
        assert np.array_equal(got[:, f], ref[:, f]), (f, got[:, f], ref[:, f])
    for f in (R.RRE, R.RR):
        assert np.all(np.abs(got[:, f] - ref[:, f]) <= 1e-12 * np.abs(ref[:, f])), (f, got[:, f], ref[:, f])


def _exact_case(distinct, nb_missing, with_presence):
    d = R.exact_design(nb_missing=nb_missing)
    presence = d["presence"] if with_presence else None
    mask_ids = d["mask_to_use"][d["idx"], 0]
    args = (d["inv"], d["val"], presence, distinct, d["table"], mask_ids, d["idx"], d["pred"], KS)
    ref64, pairs64 = R.reference(*args, np.float64)
    ref32, pairs32 = R.reference(*args, np.float32)
    return d, presence, mask_ids, ref64, pairs64, pairs32


@pytest.mark.parametrize("distinct", [True, False])
@pytest.mark.parametrize("nb_missing", [1, 2])
@pytest.mark.parametrize("with_presence", [True, False])
def test_get_equals_the_reference_on_the_exact_design(distinct, nb_missing, with_presence):
    from codae.tool import RetrievalMetrics
    d, presence, mask_ids, ref, pairs64, pairs32 = _exact_case(distinct, nb_missing, with_presence)
    # the design is exact: float64, float32 and float32 over permuted columns give the same positions
    assert pairs64 == pairs32
    order = np.random.default_rng(3).permutation(d["E"])
    shuffle = np.concatenate([c * d["E"] + order for c in range(d["S"])])
    _, pairs_perm = R.reference(d["inv"][:, :, order], d["val"], presence, distinct, d["table"], mask_ids, d["idx"], d["pred"][:, shuffle],
                                KS, np.float32)
    assert pairs_perm == pairs64
    # ... and it has what it is for: ties, a NaN row at the last position, a batch row that is no validation row
    pos = {(b, c): (p, n) for b, c, p, n in pairs64}
    assert len(pairs64) > 15 and all(p == n + 1 for (b, c), (p, n) in pos.items() if b == 5) and any(b == 5 for b, c in pos)
    assert int(d["idx"][-1]) not in d["val"]
    if nb_missing == 2:
        assert max(sum(1 for b2, _ in pos if b2 == b) for b, _ in pos) == 2              # a row with two pairs
    rm = RetrievalMetrics(R.Dataset(d["inv"]), d["val"], "cpu", ks=KS, presence=presence, distinct=distinct)
    fmask = torch.tensor(d["table"][mask_ids]).float()
    got = rm.get(torch.tensor(d["pred"]), fmask, d["idx"].tolist())
    _check_block(got["sums"], ref)
    by_ids = rm.get(torch.tensor(d["pred"]), torch.tensor(mask_ids), torch.tensor(d["idx"]), mask_table=torch.tensor(d["table"]))
    assert np.array_equal(by_ids["sums"], got["sums"])
    # the summary is the block, divided
    n = ref[:, R.PAIRS].sum()
    assert got["pairs"] == int(n) == len(pairs64) and abs(got["mrr"] - ref[:, R.RR].sum() / n) < 1e-12
    assert abs(got["hit@10"] - ref[:, R.HIT + 2].sum() / n) < 1e-12 and abs(got["rre"] - ref[:, R.RRE].sum() / n) < 1e-12
    assert len(got["per_slot"]) == d["S"] and sum(s["pairs"] for s in got["per_slot"]) == got["pairs"]
    half = sorted(p for _, _, p, _ in pairs64)[(len(pairs64) - 1) // 2]
    assert got["median_position_bucket"] == int(np.floor(np.log2(half)))


def test_duplicates_are_one_item_only_when_distinct():
    d = R.exact_design()
    args = (d["inv"], d["val"], None, d["table"], d["mask_to_use"][d["idx"], 0], d["idx"], d["pred"], KS, np.float64)
    n_distinct = {n for b, c, p, n in R.reference(*args[:3], True, *args[3:])[1] if c == 1}
    n_rows = {n for b, c, p, n in R.reference(*args[:3], False, *args[3:])[1] if c == 1}
    assert max(n_distinct) < min(n_rows)                              # slot 1 holds copies: fewer competitors once they are folded


def test_rank_error_sum_is_ranking_loss_where_the_definitions_coincide():
    """duplicate-free, complete, one blanked slot per row, every batch row a validation row: n = V - 1 and sum rre is what
    RankingLoss accumulates"""
    from codae.tool import RankingLoss, RetrievalMetrics
    d = R.gaussian_design(S=3, E=16, N=300, V=90, B=64)
    ds = R.Dataset(d["inv"])
    mask_ids = d["mask_to_use"][d["idx"], 0]
    fmask = torch.tensor(d["table"][mask_ids]).float()
    pred = torch.tensor(d["pred"])
    rl = RankingLoss(ds, d["val"], device="cpu").get(pred, fmask, d["idx"].tolist())
    got = RetrievalMetrics(ds, d["val"], "cpu", ks=KS).get(pred, fmask, d["idx"].tolist())
    assert got["pairs"] == d["B"]
    assert abs(got["sums"][:, R.RRE].sum() - rl) <= 1e-9, (got["sums"][:, R.RRE].sum(), rl)
    ref, _ = R.reference(d["inv"], d["val"], None, True, d["table"], mask_ids, d["idx"], d["pred"], KS, np.float64)
    _check_block(got["sums"], ref)


def test_arguments_are_refused():
    from codae.hip import HipError
    from codae.tool import RetrievalMetrics
    d = R.exact_design()
    ds = R.Dataset(d["inv"])
    for ks in (tuple(range(1, 10)), (5, 1), (1, 1), (0, 3), (1.5,), (True,)):
        with pytest.raises(HipError):
            RetrievalMetrics(ds, d["val"], "cpu", ks=ks)
    with pytest.raises(HipError):
        RetrievalMetrics(ds, d["val"], "cpu", presence=d["presence"][:, :2])
    with pytest.raises(HipError):
        RetrievalMetrics(ds, d["val"], "cpu", presence=d["presence"][:-1])
    assert RetrievalMetrics(ds, d["val"], "cpu", ks=(1, 2, 3, 4, 5, 6, 7, 8)).ks == (1, 2, 3, 4, 5, 6, 7, 8)


def test_header_and_binding_declare_the_entry_and_the_block():
    from codae import hip
    header = open(os.path.join(ROOT, "include", "codae_hip.h")).read()
    assert int(re.search(r"#define CODAE_ABI_VERSION (\d+)", header).group(1)) == 11 == hip.ABI_VERSION      # a new entry only
    m = re.search(r"\nint codae_retrieval_metrics_batched\(([^;]*)\);", header)
    assert m, "the entry is not declared"
    n_args = len([a for a in m.group(1).split(",") if a.strip()])
    res, args = hip.PROTOTYPES["codae_retrieval_metrics_batched"]
    assert len(args) == n_args == 29
    defs = {k: int(v) for k, v in re.findall(r"#define CODAE_RM_(\w+) (\d+)", header)}
    assert defs == {"PAIRS": hip.RM_PAIRS, "RRE": hip.RM_RRE, "RR": hip.RM_RR, "HIT": hip.RM_HIT, "MAX_KS": hip.RM_MAX_KS,
                    "HIST": hip.RM_HIST, "STRIDE": hip.RM_STRIDE}
    assert (R.PAIRS, R.RRE, R.RR, R.HIT, R.MAX_KS, R.HIST, R.STRIDE) == (hip.RM_PAIRS, hip.RM_RRE, hip.RM_RR, hip.RM_HIT, hip.RM_MAX_KS,
                                                                         hip.RM_HIST, hip.RM_STRIDE)
    assert hip.RM_HIT + hip.RM_MAX_KS <= hip.RM_HIST and hip.RM_HIST + 32 <= hip.RM_STRIDE          # the fields do not overlap
    source = open(os.path.join(ROOT, "mui-deepautoencoder_amd", "csrc", "criteria.hip")).read()
    assert "int codae_retrieval_metrics_batched(" in source
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "codae_retrieval_metrics_batched" in table


def test_config_key():
    from codae.hip import HipError
    from codae.tool import retrieval_metrics_from_config
    assert retrieval_metrics_from_config(None) is None
    assert retrieval_metrics_from_config({"K": [1, 10, 50], "DISTINCT": True}) == {"ks": (1, 10, 50), "distinct": True}
    assert retrieval_metrics_from_config({}) == {"ks": (1, 10, 50), "distinct": True}
    assert retrieval_metrics_from_config({"K": [1, 5], "DISTINCT": False}) == {"ks": (1, 5), "distinct": False}
    for bad in ({"KS": [1]}, {"K": [5, 1]}, {"K": list(range(1, 10))}, {"DISTINCT": "yes"}, [1, 10]):
        with pytest.raises(HipError):
            retrieval_metrics_from_config(bad)
