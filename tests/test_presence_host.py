"""CPU-only tests of per-row slot presence (include/codae_hip.h, "Slot presence"): codae.tool.SlotPresence against plain loops,
ReconstructionLoss.loss(weight=presence weight) and its autograd against tests/presence_ref.py, the properties of assign_masks,
ConcatenatedEmbeddingDataset(keep_incomplete=True), and the header / binding agreement on the new entries."""
import os
import random
import re

import numpy as np
import pytest
import torch

import emphasis_ref as ER
import presence_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, S, E = 120, 4, 6
IO = S * E


def _table():
    return PR.make_table(N, S)


def test_the_fixture_table_n120_s4():
    """About 30 % absent before the repair, every row keeps at least 2 present slots, at least one complete row."""
    t = _table()
    assert t.shape == (N, S) and t.dtype == np.uint8
    assert (t.sum(axis=1) >= 2).all()
    assert t[0].all() and 0.1 < (t == 0).mean() < 0.35
    assert (t.sum(axis=1) == 2).any() and (t.sum(axis=1) == S).any()


def test_apply_weight_and_counts_against_plain_loops_b33_io24():
    from codae.tool import SlotPresence
    t = _table()
    p = ER.problem(IO, S=S)
    rows = p["rows"].copy()
    rows[5] = rows[4]                                              # a repeated row
    sp = SlotPresence(t)
    assert not sp.is_default and sp.n_rows == N and sp.n_slots == S
    assert SlotPresence(None).is_default and SlotPresence(np.ones((5, 3), np.uint8)).is_default
    x = p["data"][rows].copy()
    w = sp.weight(rows, E).numpy()
    want_w = np.zeros((len(rows), IO), np.float32)
    want_x = np.zeros_like(x)
    full = part = 0
    mid = p["mask_id"]
    for b, r in enumerate(rows):
        for s in range(S):
            if t[r, s]:
                want_w[b, s * E:(s + 1) * E] = 1.0
                want_x[b, s * E:(s + 1) * E] = x[b, s * E:(s + 1) * E]
                full += 1
                part += int(p["table"][mid[b], s * E] == 0)
    assert np.array_equal(w, want_w)
    xn = x.copy()
    xn[want_w == 0] = np.nan                                       # a select: what is under an absent slot does not survive
    got = sp.apply(torch.tensor(xn), torch.tensor(rows)).numpy()
    assert np.array_equal(got, want_x) and not np.signbit(got[want_w == 0]).any()
    assert sp.counts(rows, mask_ids=mid, mask_table=p["table"]) == (full, part)
    assert sp.counts(rows) == (full, 0)
    assert 0 < part < full < len(rows) * S
    assert torch.equal(sp.to("cpu"), torch.tensor(t)) and sp.to("cpu") is sp.to("cpu")
    from codae.hip import HipError
    with pytest.raises(HipError):
        sp.weight([N], E)
    with pytest.raises(HipError):
        SlotPresence(np.ones((3, 200), np.uint8))


CASES = [("mse", {}), ("l1", {}), ("smooth_l1", dict(beta=0.5)), ("huber", dict(delta=0.75)), ("slot_cosine", dict(mse_weight=0.25))]


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "emphasis"])
@pytest.mark.parametrize("kind,kw", CASES, ids=[k for k, _ in CASES])
def test_loss_with_the_presence_weight_and_its_autograd_match_the_reference_b33_io24(kind, kw, weighted):
    """float64 torch against float64 numpy: 1e-12 relative on the loss, 1e-12 of the largest gradient on every element, and a
    gradient of exactly 0 under every absent element."""
    from codae.tool import ReconstructionLoss, SlotPresence
    t = _table()
    p = ER.problem(IO, S=S)
    rows, keep = p["rows"], p["table"][p["mask_id"]]
    x, y = p["data"][rows], p["y"]
    w = ER.weights(keep == 0, 3.0, 0.5, np.repeat(np.float32((0.5, 1.0, 2.0, 1.5)), E)) if weighted else None
    inv = np.float32(1.0 / x.size)
    ref = PR.loss_terms(kind, x, y, keep, w, inv, t, rows, param=kw.get("beta", kw.get("delta")), mse_weight=kw.get("mse_weight", 0.0), S=S)
    assert (~ref["pm"]).any() and ref["pm"].any()
    pw = SlotPresence(t).weight(rows, E, dtype=torch.float64)
    weight = pw if w is None else pw * torch.tensor(w)
    out = torch.tensor(y, dtype=torch.float64, requires_grad=True)
    n_rows = 1.0 / (float(inv) * IO)                               # the rows that give exactly the fp32 inv_n the reference rounds to
    loss = ReconstructionLoss(kind, **kw).loss(torch.tensor(x, dtype=torch.float64), out, weight=weight, n_slots=S, global_rows=n_rows)
    loss.backward()
    assert abs(float(loss.detach()) - ref["loss"]) <= 1e-12 * abs(ref["loss"]), (float(loss.detach()), ref["loss"])
    g = out.grad.numpy()
    assert np.abs(g - ref["dy"]).max() <= 1e-12 * np.abs(ref["dy"]).max()
    assert (g[~ref["pm"]] == 0).all() and (ref["dy"][~ref["pm"]] == 0).all()
    # the reference does not look under an absent slot: NaN there, in x and in y, changes nothing
    xn, yn = x.copy(), y.copy()
    xn[~ref["pm"]] = np.nan
    yn[~ref["pm"]] = np.nan
    again = PR.loss_terms(kind, xn, yn, keep, w, inv, t, rows, param=kw.get("beta", kw.get("delta")), mse_weight=kw.get("mse_weight", 0.0), S=S)
    assert again["loss"] == ref["loss"] and np.array_equal(again["dy"], ref["dy"]) and again["sq"] == ref["sq"] and again["sqp"] == ref["sqp"]


def _corrupter(n, k_max=2, seed=11):
    from codae.tool import Corrupter
    random.seed(seed)
    arch = [{"name": str(i), "lambda": 1, "size": E, "type": "regression", "position": i * E} for i in range(S)]
    return Corrupter(n, arch, k_max, "cpu")


def test_assign_masks_is_a_stable_partition_per_row_n120_s4():
    from codae.hip import HipError
    from codae.tool import SlotPresence
    t = _table()
    c = _corrupter(N)
    m2u = c.mask_to_use.numpy()
    before = random.getstate()
    got = SlotPresence(t).assign_masks(c)
    assert random.getstate() == before                              # no random numbers drawn
    assert got.dtype == torch.int32 and tuple(got.shape) == m2u.shape
    got = got.numpy()
    blanks = c.binary_masks.numpy()[:, ::E] == 0
    moved = 0
    for r in range(N):
        usable = [bool((~blanks[m] | (t[r] != 0)).all() and ((t[r] != 0) & ~blanks[m]).any()) for m in range(len(blanks))]
        assert sorted(got[r]) == sorted(m2u[r])                     # a permutation of the row
        want = [m for m in m2u[r] if usable[m]] + [m for m in m2u[r] if not usable[m]]
        assert list(got[r]) == want, r                              # usable first, both halves in their old order
        assert usable[got[r][0]]
        if t[r].all():
            assert list(got[r]) == list(m2u[r])
        moved += list(got[r]) != list(m2u[r])
    assert moved > 0
    # all ones, or no table: mask_to_use itself
    for sp in (SlotPresence(np.ones((N, S), np.uint8)), SlotPresence(None)):
        assert np.array_equal(sp.assign_masks(c).numpy(), m2u)
    # a row with one present slot has nothing to blank and still see
    one = t.copy()
    one[7] = (0, 0, 1, 0)
    with pytest.raises(HipError, match="row 7"):
        SlotPresence(one).assign_masks(c)


def _embeddings():
    rng = np.random.default_rng(5)
    cats = ["top", "bottom", "shoes"]
    emb = {}
    for i in range(12):
        have = cats if i % 3 == 0 else ([c for j, c in enumerate(cats) if j != i % 3] if i % 4 else ["shoes"])
        emb["o%d" % i] = {c: (rng.standard_normal(5) * (10.0 if (c == "shoes" and i == 4) else 1.0)).tolist() for c in have}
    return emb, cats


def test_the_dataset_default_is_the_complete_row_filter():
    from codae.dataset import ConcatenatedEmbeddingDataset
    emb, cats = _embeddings()
    d = ConcatenatedEmbeddingDataset(emb, cats)
    keep = [k for k, v in emb.items() if all(c in v for c in cats)]
    assert d.index == keep and d.nb_observation == len(keep) == 4 and d.presence is None
    raw = np.concatenate([np.asarray([emb[k][c] for k in keep], np.float32) for c in cats], axis=1)
    scale = float(raw.max() - raw.min())
    assert d.scale == scale and np.array_equal(d.data.numpy(), (torch.from_numpy(raw) / scale).numpy())
    for n, c in enumerate(cats):
        assert np.array_equal(d.data_per_category[n].numpy(), np.asarray([emb[k][c] for k in keep], np.float32))
    e = ConcatenatedEmbeddingDataset(emb, cats, None, False, 2)
    assert e.index == d.index and torch.equal(e.data, d.data) and e.scale == d.scale


def test_the_dataset_keeps_incomplete_rows_with_a_table_zeros_and_a_present_only_scale():
    from codae.dataset import ConcatenatedEmbeddingDataset
    emb, cats = _embeddings()
    d = ConcatenatedEmbeddingDataset(emb, cats, keep_incomplete=True)
    keep = [k for k, v in emb.items() if sum(c in v for c in cats) >= 2]
    assert d.index == keep and d.nb_observation == len(keep) == 10               # o4 and o8 have shoes only
    want = np.array([[int(c in emb[k]) for c in cats] for k in keep], np.uint8)
    assert d.presence.dtype == np.uint8 and np.array_equal(d.presence, want) and (want == 0).any()
    vals = np.concatenate([np.asarray(emb[k][c], np.float32) for k in keep for c in cats if c in emb[k]])
    assert d.scale == float(vals.max() - vals.min()) and float(d.min) == float(vals.min()) and float(d.max) == float(vals.max())
    data = d.data.numpy()
    for r, k in enumerate(keep):
        for n, c in enumerate(cats):
            block = data[r, n * 5:(n + 1) * 5]
            if c in emb[k]:
                assert np.array_equal(block, (torch.tensor(emb[k][c], dtype=torch.float32) / d.scale).numpy())
                assert np.array_equal(d.data_per_category[n][r].numpy(), np.asarray(emb[k][c], np.float32))
            else:
                assert (block == 0).all() and (d.data_per_category[n][r].numpy() == 0).all()
    assert d.io_size == 15 and len(d.arch) == 3
    one = ConcatenatedEmbeddingDataset(emb, cats, keep_incomplete=True, min_present=1)
    assert one.nb_observation == 12
    # the 10 x outlier sits in a row that min_present = 2 drops: the scale follows the rows that are kept
    assert one.scale > d.scale
    with pytest.raises(ValueError):
        ConcatenatedEmbeddingDataset(emb, cats, keep_incomplete=True, min_present=4)


def test_header_and_binding_declare_the_new_entries_with_abi_11():
    from codae import hip
    header = open(os.path.join(ROOT, "include", "codae_hip.h")).read()
    assert int(re.search(r"#define CODAE_ABI_VERSION (\d+)", header).group(1)) == 11 == hip.ABI_VERSION      # new entries only
    assert int(re.search(r"#define CODAE_N_STRUCTS (\d+)", header).group(1)) == 7
    names = ("codae_set_slot_presence", "codae_corrupt_batch_present", "codae_mse_loss_present", "codae_emph_loss_present",
             "codae_recon_loss_fwd_bwd_present", "codae_slot_contrast_prepare_present", "codae_slot_contrast_fwd_bwd_present")
    for name in names:
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m, name
        assert name in hip.PROTOTYPES and len(hip.PROTOTYPES[name][1]) == m.group(1).count(",") + 1, name
    assert re.search(r"int codae_set_slot_presence\(codae_handle h, const uint8_t\* present, int64_t n_rows, int32_t n_slots\);", header)
    assert "Slot presence" in header and "may be NaN" in header
    from codae.tool import SlotPresence
    from codae.train import HipEmbeddingTrainer
    import inspect
    assert "presence" in inspect.signature(HipEmbeddingTrainer.__init__).parameters and hasattr(HipEmbeddingTrainer, "set_presence")
    for attr in ("is_default", "to", "apply", "weight", "counts", "assign_masks"):
        assert hasattr(SlotPresence, attr)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "codae_set_slot_presence" in integration
