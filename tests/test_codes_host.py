"""Outfit codes on the host (no GPU): OutfitCodes.forward_to against the hand-written float64 statement the GPU tests use
(tests/norm_ref.py), the default code layer of the stacks linear_stack builds, similar() on host tensors against a brute-force numpy
cosine ranking, the config block, and the header."""
import os

import numpy as np
import pytest

import norm_ref as NR

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-5


def _tools():
    from codae.hip import HipError
    from codae.tool import Norm, OutfitCodes, Residual, codes_from_config
    return OutfitCodes, Norm, Residual, codes_from_config, HipError


def test_forward_to_is_h_k_of_the_float64_statement_l5_w24():
    OutfitCodes, Norm, Residual, _, HipError = _tools()
    rng = np.random.default_rng(3)
    L, w, B = 5, 24, 17
    params = [(rng.standard_normal((w, w)) * 0.3, rng.standard_normal(w) * 0.05) for _ in range(L)]
    params = [(W.astype(np.float32), b.astype(np.float32)) for W, b in params]
    x = rng.standard_normal((B, w)).astype(np.float32)
    acts = ["relu"] * (L - 1) + [None]
    skips, norms = [0, 1, 1, 1, 0], [1, 1, 1, 1, 0]
    hs = NR.forward(params, acts, skips, norms, "layer", EPS, x)[1]
    Ws = [torch.tensor(W, dtype=torch.float64) for W, _ in params]
    bs = [torch.tensor(b, dtype=torch.float64) for _, b in params]
    flags = [True] * (L - 1) + [False]
    xt = torch.tensor(x, dtype=torch.float64)
    for k in range(1, L):
        got = OutfitCodes.forward_to(xt, Ws, bs, flags, k, residual=Residual("hidden"), norm=Norm("layer", eps=EPS)).numpy()
        assert got.shape == (B, w)
        assert np.allclose(got, hs[k], rtol=1e-9, atol=1e-11), (k, float(np.abs(got - hs[k]).max()))
        plain = OutfitCodes.forward_to(xt, Ws, bs, flags, k).numpy()                 # ... and not the stack without skips and norm
        assert not np.allclose(plain, hs[k], rtol=1e-3, atol=1e-5), k
    # autograd works through it
    xg = xt.clone().requires_grad_(True)
    OutfitCodes.forward_to(xg, Ws, bs, flags, 3, residual=Residual("hidden"), norm=Norm("layer", eps=EPS)).sum().backward()
    assert xg.grad is not None and bool(torch.isfinite(xg.grad).all())
    for bad in (0, L, True, 1.0):
        with pytest.raises(HipError, match="layer"):
            OutfitCodes.forward_to(xt, Ws, bs, flags, bad)


def test_the_default_code_layer_is_the_z_layer_of_a_linear_stack():
    from codae.hip import HipError
    from codae.model.schedule import linear_stack
    from codae.tool.codes import code_layers
    for nb_in, nb_out in ((1, 1), (2, 2), (4, 3), (5, 5)):
        enc, dec = linear_stack(192, 64, nb_in, nb_out, True, True)                  # square: io -> io ... -> z (the mixed form builds it)
        assert code_layers(enc + dec) == nb_in + 1
        assert (enc + dec)[nb_in][1] == 64
    for nb_in, nb_out in ((2, 2), (4, 3), (5, 5)):
        enc, dec = linear_stack(192, 64, nb_in, nb_out, False, False)                # tapered
        assert code_layers(enc + dec) == nb_in + 1
        assert (enc + dec)[nb_in][1] == 64
    # the engine's 4-tuples count as well: kind 0 = none
    assert code_layers([(8, 8, (1, 0, 0, 0)), (8, 4, (0, 0, 0, 0)), (4, 8, (2, 0.1, 0, 0)), (8, 8, (0, 0, 0, 0))]) == 2
    with pytest.raises(HipError, match="no default code layer"):
        code_layers([(24, 24, True)] * 4 + [(24, 24, False)])                        # all-ReLU: only the output layer lacks one


def _brute(bank, query, k, exclude=None, distinct=False, rows=None):
    """float64 cosine ranking from the definition: score descending, ties by ascending row, (-1, -inf) padding; distinct: identical
    bank rows are one entry, the lowest row"""
    M = bank.shape[0]
    rows = np.arange(M) if rows is None else np.asarray(rows)
    b64, q64 = bank.astype(np.float64), query.astype(np.float64)
    cos = (q64 @ b64.T) / (np.maximum(np.linalg.norm(q64, axis=1), 1e-8)[:, None] * np.maximum(np.linalg.norm(b64, axis=1), 1e-8)[None, :])
    cos = cos.astype(np.float32)
    entry = np.arange(M)
    if distinct:
        for i in range(M):
            same = [j for j in range(i) if bank[j].tobytes() == bank[i].tobytes()]
            if same:
                entry[i] = entry[same[0]]
    keep = np.array([entry[i] == i for i in range(M)])
    idx = np.full((query.shape[0], k), -1, dtype=np.int64)
    score = np.full((query.shape[0], k), -np.inf, dtype=np.float32)
    for q in range(query.shape[0]):
        ok = keep.copy()
        if exclude is not None and exclude[q] in set(rows.tolist()):
            ok &= entry != entry[int(np.flatnonzero(rows == exclude[q])[0])]
        ok &= ~np.isnan(cos[q])
        cand = sorted(np.flatnonzero(ok), key=lambda j: (-cos[q, j], rows[j]))[:k]
        idx[q, :len(cand)] = rows[cand]
        score[q, :len(cand)] = cos[q, cand]
    return idx, score


def test_similar_on_host_tensors_is_the_brute_force_cosine_ranking():
    OutfitCodes, _, _, _, HipError = _tools()
    rng = np.random.default_rng(5)
    M, Z, Q = 23, 8, 6
    bank = rng.standard_normal((M, Z)).astype(np.float32)
    bank[7] = bank[2]                      # duplicates: equal scores, ordered by row - or one entry under `distinct`
    bank[19] = bank[2]
    bank[11] = 2.0 * bank[4]               # a tie in cosine that is NOT a duplicate: stays two entries, the lower row first
    bank[15] = 0.0                         # a zero row: the clamped norm, score 0
    query = np.concatenate([bank[[2, 4, 9]], rng.standard_normal((Q - 3, Z)).astype(np.float32)])
    tb, tq = torch.tensor(bank), torch.tensor(query)
    for distinct in (False, True):
        oc = OutfitCodes(tb, distinct=distinct)
        assert len(oc) == M and oc.width == Z
        for k in (1, 5):
            idx, score = oc.similar(tq, k)
            ri, rs = _brute(bank, query, k, distinct=distinct)
            assert idx.dtype == torch.long and score.dtype == torch.float32
            assert np.array_equal(idx.numpy(), ri), (distinct, k)
            assert np.allclose(score.numpy(), rs, rtol=1e-6, atol=1e-7)
        ex = np.array([2, 11, 9, 0, -1, 1000])
        idx, score = oc.similar(tq, 4, exclude=torch.tensor(ex))
        ri, rs = _brute(bank, query, 4, exclude=ex, distinct=distinct)
        assert np.array_equal(idx.numpy(), ri), distinct
        assert np.allclose(score.numpy(), rs, rtol=1e-6, atol=1e-7)
        assert 2 not in idx[0].tolist() and (distinct or 7 in idx[0].tolist())       # the row itself never; its duplicates only folded
        if distinct:
            assert 7 not in idx[0].tolist() and 19 not in idx[0].tolist()
    # ties by ascending row: rows 2, 7, 19 first for their own code, in that order, then whatever follows
    idx, score = OutfitCodes(tb, distinct=False).similar(tq[:1], 3)
    assert idx[0].tolist() == [2, 7, 19] and np.allclose(score[0].numpy(), 1.0, atol=1e-6)
    idx, _ = OutfitCodes(tb, distinct=False).similar(tq[1:2], 2)
    assert idx[0].tolist() == [4, 11]
    # k past the bank: a short list ends in (-1, -inf)
    small = OutfitCodes(tb[:3].clone(), distinct=True)
    idx, score = small.similar(tq, 5)
    assert (idx[:, 3:] == -1).all() and torch.isinf(score[:, 3:]).all() and (score[:, 3:] < 0).all() and (idx[:, :3] >= 0).all()
    # a bank over chosen dataset rows: results and exclude speak dataset rows
    rows = np.arange(100, 100 + M)[::-1].copy()
    oc = OutfitCodes(tb, rows=torch.tensor(rows), distinct=True)
    ex = np.array([rows[2], rows[11], 5, -1, rows[0], 10 ** 6])
    idx, score = oc.similar(tq, 4, exclude=torch.tensor(ex))
    # (the bank is held in ascending dataset row, so ties and the representative of identical entries go by DATASET row)
    order = np.argsort(rows)
    ri, rs = _brute(bank[order], query, 4, exclude=ex, distinct=True, rows=rows[order])
    assert np.array_equal(idx.numpy(), ri)
    assert np.allclose(score.numpy(), rs, rtol=1e-6, atol=1e-7)
    assert not {rows[2], rows[7], rows[19]} & set(idx[0].tolist())
    # a NaN bank row is never returned
    nb = bank.copy()
    nb[3, 1] = np.nan
    idx, score = OutfitCodes(torch.tensor(nb), distinct=False).similar(tq, M)
    assert 3 not in idx.numpy().ravel().tolist() and not torch.isnan(score).any()
    assert (idx[:, -1] == -1).all()
    with pytest.raises(HipError, match="query"):
        oc.similar(torch.zeros((2, Z + 1)), 3)
    with pytest.raises(HipError, match="query"):
        oc.similar(torch.zeros((0, Z)), 3)
    with pytest.raises(HipError, match="exclude"):
        oc.similar(tq, 3, exclude=torch.zeros(Q))
    with pytest.raises(HipError, match="distinct dataset rows"):
        OutfitCodes(tb, rows=[0] * M)


def test_config_block():
    _, _, _, codes_from_config, HipError = _tools()
    assert codes_from_config(None) is None and codes_from_config({}) is None
    assert codes_from_config({"SAVE": True}) == {"save": True, "layer": None, "neighbours": 0, "distinct": True}
    assert codes_from_config({"SAVE": True, "LAYER": 3, "NEIGHBOURS": 5, "DISTINCT": False}) == {
        "save": True, "layer": 3, "neighbours": 5, "distinct": False}
    assert codes_from_config({"SAVE": False, "NEIGHBOURS": 5}) is None
    with pytest.raises(HipError, match=r"CODES: unknown key\(s\) CLUSTERS"):
        codes_from_config({"SAVE": True, "CLUSTERS": 8})
    with pytest.raises(HipError, match="must be a mapping"):
        codes_from_config("yes")
    with pytest.raises(HipError, match="NEIGHBOURS"):
        codes_from_config({"NEIGHBOURS": -1})
    with pytest.raises(HipError, match="LAYER"):
        codes_from_config({"LAYER": 0})


def test_the_header_keeps_its_abi_version_and_documents_the_section():
    text = open(os.path.join(ROOT, "include", "codae_hip.h")).read()
    assert "#define CODAE_ABI_VERSION 11" in text and "CODAE_K_COUNT = 11" in text
    assert "Outfit codes" in text
    for name in ("codae_export_rows", "codae_encode", "codae_decode"):
        assert ("int %s(" % name) in text
    from codae import hip
    for name in ("codae_export_rows", "codae_encode", "codae_decode"):
        assert name in hip.PROTOTYPES
