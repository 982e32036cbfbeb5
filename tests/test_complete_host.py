"""Complementarity inference on the host (codae.tool.ComplementRetriever with CPU tensors) against a float64 numpy brute
force: per-row slots, candidate subsets, distinct items, exclusion, short candidate lists, NaN / zero queries, bad
arguments."""
import types

import numpy as np
import pytest
import torch

from complete_ref import check_topk, ref_ranked

S, E, N = 3, 16, 300


def make_dataset(seed=0, dup=True):
    rng = np.random.default_rng(seed)
    blocks = [rng.standard_normal((N, E)).astype(np.float32) for _ in range(S)]
    if dup:
        # planted duplicates: row 40 repeats row 7 in slot 0 and row 12 repeats row 100 (the later row is the copy source);
        # slot 1's rows 50..59 are all one item
        blocks[0][40] = blocks[0][7]
        blocks[0][12] = blocks[0][100]
        blocks[1][50:60] = blocks[1][50]
    ds = types.SimpleNamespace(nb_used_category=S, embedding_size=E,
                               data_per_category={c: torch.from_numpy(blocks[c].copy()) for c in range(S)})
    return ds, blocks


def queries(B, seed=1):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((B, S * E)).astype(np.float32))


def test_per_row_slots_match_float64():
    from codae.tool import ComplementRetriever
    ds, inv = make_dataset()
    pred = queries(40)
    slots = torch.arange(40) % S
    r = ComplementRetriever(ds, "cpu", distinct=False)
    for k in (1, 10, 37):
        idx, sc = r.topk(pred, slots, k)
        assert idx.dtype == torch.long and sc.dtype == torch.float32 and idx.shape == (40, k)
        check_topk(idx, sc, ref_ranked(pred.numpy(), slots.tolist(), inv, E, k, distinct=False), k)


def test_int_slot_and_candidate_subset():
    from codae.tool import ComplementRetriever
    ds, inv = make_dataset()
    pred = queries(16, seed=2)
    cands = [250, 3, 17, 99, 120, 121, 3, 260]
    r = ComplementRetriever(ds, "cpu", candidates=cands, distinct=False)
    idx, sc = r.topk(pred, 2, 5)
    assert set(idx.flatten().tolist()) <= set(cands)
    check_topk(idx, sc, ref_ranked(pred.numpy(), [2] * 16, inv, E, 5, candidates=cands, distinct=False), 5)


def test_distinct_returns_the_lowest_row_once():
    from codae.tool import ComplementRetriever
    ds, inv = make_dataset()
    # queries equal to the duplicated items: the item is the best match and must come back once, as its lowest row
    pred = torch.zeros(3, S * E)
    pred[0, 0:E] = torch.from_numpy(inv[0][7])
    pred[1, 0:E] = torch.from_numpy(inv[0][100])
    pred[2, E:2 * E] = torch.from_numpy(inv[1][55])
    slots = torch.tensor([0, 0, 1])
    idx, sc = ComplementRetriever(ds, "cpu").topk(pred, slots, 12)
    assert idx[0, 0] == 7 and 40 not in idx[0].tolist()
    assert idx[1, 0] == 12 and 100 not in idx[1].tolist()
    assert idx[2, 0] == 50 and not set(range(51, 60)) & set(idx[2].tolist())
    check_topk(idx, sc, ref_ranked(pred.numpy(), slots.tolist(), inv, E, 12), 12)
    # without distinct the copies are separate candidates with equal scores, in ascending row order
    idx2, sc2 = ComplementRetriever(ds, "cpu", distinct=False).topk(pred, slots, 12)
    assert idx2[0, :2].tolist() == [7, 40] and sc2[0, 0] == sc2[0, 1]
    assert idx2[2, :10].tolist() == list(range(50, 60))


def test_exclude_skips_the_row_and_its_item():
    from codae.tool import ComplementRetriever
    ds, inv = make_dataset()
    pred = torch.zeros(2, S * E)
    pred[0, 0:E] = torch.from_numpy(inv[0][40])            # the copy of row 7
    pred[1, 0:E] = torch.from_numpy(inv[0][33])
    ex = torch.tensor([40, 33])
    for distinct in (True, False):
        idx, sc = ComplementRetriever(ds, "cpu", distinct=distinct).topk(pred, 0, 5, exclude=ex)
        assert 33 not in idx[1].tolist() and 40 not in idx[0].tolist()
        assert (7 in idx[0].tolist()) == (not distinct)       # under distinct row 40 collapses into item 7
        check_topk(idx, sc, ref_ranked(pred.numpy(), [0, 0], inv, E, 5, distinct=distinct, exclude=ex.numpy()), 5)


def test_k_beyond_the_candidates_pads_the_tail():
    from codae.tool import ComplementRetriever
    ds, inv = make_dataset()
    pred = queries(4, seed=3)
    cands = [5, 6, 7, 40]                                  # 40 duplicates 7 in slot 0
    idx, sc = ComplementRetriever(ds, "cpu", candidates=cands).topk(pred, 0, 6)
    assert (idx[:, 3:] == -1).all() and torch.isneginf(sc[:, 3:]).all()
    check_topk(idx, sc, ref_ranked(pred.numpy(), [0] * 4, inv, E, 6, candidates=cands), 6)
    idx, sc = ComplementRetriever(ds, "cpu", candidates=cands, distinct=False).topk(pred, 0, 6, exclude=torch.tensor([5, 5, 6, 0]))
    assert (idx[:2, 3:] == -1).all() and (idx[2:3, 3:] == -1).all() and (idx[3, :4] >= 0).all() and (idx[3, 4:] == -1).all()


def test_nan_and_zero_queries():
    from codae.tool import ComplementRetriever
    ds, inv = make_dataset(dup=False)
    pred = queries(3, seed=4)
    pred[0, :E] = float("nan")
    pred[1, :E] = 0.0
    inv0 = inv[0].copy()
    idx, sc = ComplementRetriever(ds, "cpu").topk(pred, 0, 8)
    assert (idx[0] == -1).all() and torch.isneginf(sc[0]).all()          # NaN scores are never returned
    assert idx[1].tolist() == list(range(8)) and (sc[1] == 0).all()       # all ties at 0: ascending row id
    assert not torch.signbit(sc[1]).any()
    check_topk(idx, sc, ref_ranked(pred.numpy(), [0] * 3, {0: inv0}, E, 8), 8)


def test_argument_errors():
    from codae.hip import HipError
    from codae.tool import ComplementRetriever
    ds, _ = make_dataset()
    r = ComplementRetriever(ds, "cpu")
    pred = queries(4)
    for k in (0, 257, 2.0, True):
        with pytest.raises(HipError):
            r.topk(pred, 0, k)
    for slot in (-1, S, 1.5, torch.tensor([0, 1, 2, 3]), torch.tensor([0, 1])):
        with pytest.raises(HipError):
            r.topk(pred, slot, 3)
    with pytest.raises(HipError):
        r.topk(pred[:, :-1], 0, 3)
    with pytest.raises(HipError):
        r.topk(pred, 0, 3, exclude=torch.tensor([1, 2]))
    with pytest.raises(HipError):
        r.topk(pred, 0, 3, chunk=0)
    with pytest.raises(ValueError):
        ComplementRetriever(ds, "cpu", candidates=[0, N])
    assert r.topk(pred, 0, 256)[0].shape == (4, 256)
