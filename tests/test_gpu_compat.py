"""Assembled outfits and compatibility on a real MI355X: the assemble kernel bit for bit, its equivalence with the batch gather and
complete_items with complete(), the score kernel against float64 fed the device's own reconstruction, score_outfits' invariance to
batch size and chunking and its leaving the engine's state alone, the AUC counts against numpy, and a hand-built design whose AUC is
exactly 1 (0 with the weights negated, live or averaged)."""
import ctypes as C

import numpy as np
import pytest

import compat_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
S = 3


@pytest.fixture(scope="module")
def hip():
    from codae import hip as H
    H.lib()
    return H


def _data(E, N=50, seed=0, with_presence=False):
    rng = np.random.default_rng(seed + E)
    data = rng.standard_normal((N, S * E)).astype(np.float32)
    presence = None
    if with_presence:
        presence = (rng.random((N, S)) > 0.25).astype(np.uint8)
        presence[:4] = [[1, 1, 1], [1, 0, 1], [0, 0, 1], [0, 0, 0]]
        data[np.repeat(presence == 0, E, axis=1)] = np.nan        # an absent slot's data is never read into a result
    return data, presence


def _items(N, Q=37, seed=0):
    """negatives, one dataset row repeated in several outfits, outfits of three different rows, rows as they are"""
    rng = np.random.default_rng(seed)
    items = rng.integers(0, N, (Q, S)).astype(np.int32)
    items[0] = [0, 1, 2]
    items[1] = 7
    items[2] = [7, -1, 7]
    items[3] = [-1, 7, 9]
    items[4] = -1
    items[5] = [3, 3, 3]
    items[6] = [2, 2, -5]
    return items


def _trainer(E, precision, N=50, max_batch=128, hidden=64, presence=None, data=None, seed=0, **kw):
    from codae.tool import SlotPresence
    from codae.train import HipEmbeddingTrainer
    io = S * E
    if data is None:
        data = _data(E, N, seed)[0]
    tr = HipEmbeddingTrainer([(io, hidden, True), (hidden, io, False)], torch.tensor(data), None, None, 1e-3, 1e-4, 1.0, max_batch=max_batch,
                             precision=precision, device=DEV, n_slots=S, presence=None if presence is None else SlotPresence(presence), **kw)
    tr.init_params(seed=3)
    return tr


# ---- assemble ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_presence", [False, True])
@pytest.mark.parametrize("form", ["blank", "loo"])
@pytest.mark.parametrize("E", [8, 24, 64])
def test_assemble_is_bit_exact(hip, E, form, with_presence):
    from codae.tool import Compatibility
    data, presence = _data(E, with_presence=with_presence)
    N, io = data.shape
    items = _items(N)
    Q = len(items)
    kw = {"leave_one_out": True} if form == "loo" else {"blank": np.random.default_rng(1).integers(-1, S, Q).astype(np.int32)}
    ref = R.assemble(data, items, S, presence=presence, **kw)
    assert not np.isnan(ref).any()
    ref16 = torch.tensor(ref).to(torch.bfloat16).view(torch.int16).numpy()
    tkw = {k: (torch.tensor(v) if k == "blank" else v) for k, v in kw.items()}
    d = torch.tensor(data).to(DEV)
    img = torch.empty(d.shape, dtype=torch.bfloat16, device=DEV)
    hip.check(hip.lib().codae_cast_f32_to_bf16(hip.ptr(d), hip.ptr(img), d.numel(), hip.current_stream()))
    it = torch.tensor(items).to(DEV)
    ld = (io + 63) // 64 * 64                                    # E = 24: 72 columns in rows 128 apart, as the engine's act[0]
    for src, dtype, want in ((d, torch.float32, ref), (d, torch.bfloat16, ref16), (img, torch.bfloat16, ref16)):
        got = Compatibility.assemble(src, it, presence=presence, out_dtype=dtype, **tkw)
        raw = got.view(torch.int16) if dtype == torch.bfloat16 else got
        assert raw.cpu().numpy().tobytes() == want.tobytes(), (src.dtype, dtype)
        out = torch.full((ref.shape[0], ld), 3.0, dtype=dtype, device=DEV)
        got = Compatibility.assemble(src, it, presence=presence, out=out, **tkw)
        raw = out.view(torch.int16) if dtype == torch.bfloat16 else out
        assert raw[:, :io].cpu().numpy().tobytes() == want.tobytes() and bool((out[:, io:] == 3.0).all())      # the pad is not written


def test_assemble_narrow_forms_and_errors(hip):
    from codae.hip import HipError
    from codae.tool import Compatibility
    # E = 6: no group of four columns sits inside a slot (the scalar form); E = 4: the 4-wide form for both output types
    for E, N in ((6, 9), (4, 9)):
        rng = np.random.default_rng(E)
        data = rng.standard_normal((N, S * E)).astype(np.float32)
        items = rng.integers(-1, N, (5, S)).astype(np.int32)
        ref = R.assemble(data, items, S, leave_one_out=True)
        for dtype in (torch.float32, torch.bfloat16):
            got = Compatibility.assemble(torch.tensor(data).to(DEV), torch.tensor(items), leave_one_out=True, out_dtype=dtype)
            assert torch.equal(got.cpu(), torch.tensor(ref).to(dtype))
    L, st = hip.lib(), hip.current_stream()
    d = torch.zeros((4, 24), device=DEV)
    it = torch.zeros((2, 3), dtype=torch.int32, device=DEV)
    out = torch.zeros((6, 24), device=DEV)
    args = lambda io, s, q: (hip.ptr(d), 0, 4, io, s, hip.ptr(it), q, None, 0, None, hip.ptr(out), 0, 0, st)
    for io, s, q, word in ((24, 5, 2, "divide"), (24, 129, 2, "128"), (24, 3, 0, "Q")):
        assert L.codae_assemble_outfits(*args(io, s, q)) == -1 and word in L.codae_last_error().decode()
    with pytest.raises(HipError):
        Compatibility.assemble(d, it, presence=np.ones((5, 3), dtype=np.uint8))      # a presence table of another shape


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_assemble_equals_the_batch_gather_and_complete_items_equals_complete(hip, precision):
    from codae.tool import Compatibility
    E = 24
    data, presence = _data(E, with_presence=True)
    tr = _trainer(E, precision, presence=presence, data=data)
    io = S * E
    rows = torch.tensor([0, 1, 2, 3, 7, 7, 20, 49, 33, 12, 5], dtype=torch.int32, device=DEV)
    table = torch.ones((S, io), dtype=torch.uint8)
    for c in range(S):
        table[c, c * E:(c + 1) * E] = 0
    table = table.to(DEV)
    items = rows[:, None].expand(-1, S).contiguous()
    for c in range(S):
        mid = torch.full((rows.numel(),), c, dtype=torch.int32, device=DEV)
        blank = mid.clone()
        batch = tr.engine.make_batch(tr.data, rows, mid, table)
        for bf in (0, 1):
            dtype = torch.bfloat16 if bf else torch.float32
            want = torch.full((rows.numel(), io), 9.0, dtype=dtype, device=DEV)
            hip.check(hip.lib().codae_corrupt_batch_present(C.byref(batch), None, 0, None, hip.ptr(want), bf, 0, hip.ptr(tr.engine._presence_table),
                                                            S, hip.current_stream()))
            got = Compatibility.assemble(tr.data, items, blank=blank, presence=tr.presence, out_dtype=dtype)
            assert torch.equal(got.view(torch.int16) if bf else got.view(torch.int32), want.view(torch.int16) if bf else want.view(torch.int32))
        # the same query through both routes: the same input bits and the same forward launches -> the same bits out
        for distinct in (True, False):
            i0, s0 = tr.complete(rows, c, 7, distinct=distinct)
            i1, s1 = tr.complete_items(items, c, 7, exclude_items=False, distinct=distinct)
            assert torch.equal(i0, i1) and torch.equal(s0.view(torch.int32), s1.view(torch.int32))
            i0, s0 = tr.complete(rows, c, 7, exclude_self=True, distinct=distinct)
            i1, s1 = tr.complete_items(items, c, 7, distinct=distinct)
            assert torch.equal(i0, i1) and torch.equal(s0.view(torch.int32), s1.view(torch.int32))
            assert not (i1 == rows.long()[:, None]).any() and (i1[:, 0] >= 0).all()


def test_complete_items_mixes_rows_and_ignores_the_blanked_entry(hip):
    tr = _trainer(8, "f32")
    items = torch.tensor([[12, 40, 7], [12, -1, 7], [12, 3, 7]], dtype=torch.int32)
    idx, sc = tr.complete_items(items, 1, 5, exclude_items=False)
    assert torch.equal(idx[0], idx[1]) and torch.equal(idx[0], idx[2]) and torch.equal(sc[0], sc[1])      # whatever items[:, slot] holds
    assert (idx >= 0).all() and bool((sc[:, :-1] >= sc[:, 1:]).all())
    ex, _ = tr.complete_items(items, 1, 5)
    assert 40 not in ex[0].tolist() and 3 not in ex[2].tolist() and torch.equal(ex[1], idx[1])
    # against the definition: assemble by hand, the engine's forward, the host retriever
    from codae.tool import ComplementRetriever
    x = torch.tensor(R.assemble(tr.data.cpu().numpy(), items.numpy(), S, blank=[1, 1, 1])).to(DEV)
    y = tr.engine.forward(x).cpu()
    hi, _ = ComplementRetriever(R.Dataset(tr.data.cpu().numpy(), S), "cpu").topk(y, 1, 5)
    assert torch.equal(hi, idx.cpu())
    before = tr.engine.scalars.clone()
    tr.complete_items(items, 0, 3)
    assert torch.equal(tr.engine.scalars, before)


# ---- slot scores ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_presence", [False, True])
@pytest.mark.parametrize("precision,E", [("f32", 8), ("bf16", 8), ("f32", 24), ("bf16", 24), ("f32", 64), ("bf16", 64), ("f32", 512), ("bf16", 512)])
def test_slot_scores_against_float64_fed_the_devices_own_output(hip, precision, E, with_presence):
    data, presence = _data(E, with_presence=with_presence)
    N = len(data)
    tr = _trainer(E, precision, presence=presence, data=data, max_batch=128)
    items = _items(N)
    Q = len(items)
    got = tr.score_outfits(torch.tensor(items))              # 37 x 3 = 111 rows: one engine call
    # the device's own reconstruction of the leave-one-out rows: the same input bits through the same forward launches (the stand-alone
    # score entry fed this Y gives the engine entry's bits, below)
    from codae.tool import Compatibility
    X = Compatibility.assemble(tr.data, torch.tensor(items), leave_one_out=True, presence=tr.presence)
    Y = tr.engine.forward(X).cpu().numpy()
    cos, sq, score, n = R.slot_scores(data, items, Y, S, presence=presence)
    g = {k: v.cpu().numpy() for k, v in got.items()}
    bound = (E + 8) * 2.0 ** -23
    assert np.array_equal(g["n_present"], n) and (n < 2).any() and (n == 3).any()
    print("E %d %s: max |cos - ref| %.3g (bound %.3g), max rel sq %.3g" % (E, precision, np.abs(g["cos"] - cos).max(), bound,
                                                                        (np.abs(g["sq"] - sq) / np.maximum(sq, 1e-300)).max()))
    assert not np.isnan(g["cos"]).any() and np.abs(g["cos"] - cos).max() <= bound
    assert np.all(np.abs(g["sq"] - sq) <= bound * sq)
    assert np.array_equal(np.isnan(g["score"]), n < 2)
    for q in range(Q):                                       # the fp32 mean of the device's own cosines, ascending slots, exactly
        if n[q] >= 2:
            acc = np.float32(0)
            for s in range(S):
                if R.present(items, q, s, N, presence):
                    acc = np.float32(acc + g["cos"][q, s])
            assert g["score"][q].tobytes() == np.float32(acc / np.float32(n[q])).tobytes()
        else:
            assert (g["cos"][q][[not R.present(items, q, s, N, presence) for s in range(S)]] == 0).all()
    # the stand-alone entry on the same Y: the same bits as the engine entry
    from codae.tool import Compatibility
    alone = Compatibility.slot_scores(tr.data, torch.tensor(items), torch.tensor(Y).to(DEV), presence=presence)
    for k in g:
        assert np.array_equal(alone[k].cpu().numpy().view(np.int32), g[k].view(np.int32)), k


@pytest.mark.parametrize("precision,E", [("f32", 24), ("bf16", 24), ("f32", 64), ("bf16", 64)])
def test_scores_do_not_depend_on_batch_size_position_or_chunking(hip, precision, E):
    data, _ = _data(E)
    items = torch.tensor(_items(len(data)))
    big = _trainer(E, precision, data=data, max_batch=128)
    small = _trainer(E, precision, data=data, max_batch=48)           # 16 outfits per engine call: 37 take three
    whole = big.score_outfits(items)
    chunked = small.score_outfits(items)
    for q in (0, 15, 16, 20, 36):
        one = big.score_outfits(items[q:q + 1])
        for k in whole:
            a, b, c = (t[k].cpu().numpy().view(np.int32) for t in (whole, chunked, one))
            assert np.array_equal(a[q], c[0]) and np.array_equal(a[q], b[q]), (k, q)
    again = big.score_outfits(items)
    assert all(torch.equal(whole[k].view(torch.int32), again[k].view(torch.int32)) for k in whole)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_score_outfits_leaves_the_engine_state_alone(hip, precision):
    from codae.tool import WeightAverage
    tr = _trainer(24, precision, weight_average=WeightAverage("ema", decay=0.9))
    eng = tr.engine
    rows = torch.arange(40, dtype=torch.int32, device=DEV)
    tr.train_batch(rows, run=None)
    tr.eval_batch(rows, run=None)                              # non-zero metric sums
    names = ["scalars", "_params", "grads", "adam_m", "adam_v", "shadow", "shadow_t", "weight_avg", "avg_shadow"]
    eng.sync_average()
    before = {n: getattr(eng, n).clone() for n in names if getattr(eng, n) is not None}
    assert float(before["scalars"][0]) > 0
    items = torch.tensor(_items(50))
    for weights in ("live", "average"):
        out = tr.score_outfits(items, weights=weights)
        assert np.isfinite(out["score"].cpu().numpy()[[0, 1, 5]]).all()
    for n, t in before.items():
        same = torch.equal(getattr(eng, n).view(torch.int16), t.view(torch.int16))
        assert same, n
    assert tr.epoch_sums(reset=False) == (float(before["scalars"][0]), float(before["scalars"][1]))


def test_score_outfits_argument_errors(hip):
    from codae.hip import HipError
    tr = _trainer(8, "f32", max_batch=48)
    eng = tr.engine
    L = hip.lib()
    with pytest.raises(HipError, match="max_batch"):
        eng.score_outfits(tr.data, torch.zeros((17, 3), dtype=torch.int32, device=DEV))
    with pytest.raises(HipError, match="divide"):
        eng.score_outfits(tr.data, torch.zeros((2, 5), dtype=torch.int32, device=DEV))
    with pytest.raises(HipError, match="128"):
        eng.score_outfits(tr.data, torch.zeros((1, 3), dtype=torch.int32, device=DEV), n_slots=129)
    with pytest.raises(HipError, match="Q"):
        eng.score_outfits(tr.data, torch.zeros((0, 3), dtype=torch.int32, device=DEV))
    with pytest.raises(HipError, match="row"):
        tr.score_outfits(torch.tensor([[0, 1, 50]]))           # a host tensor is checked against the dataset's rows
    table = torch.ones((50, 4), dtype=torch.uint8, device=DEV)
    eng._set_presence_table(table, n_rows=50, n_slots=2)       # (2 divides io: the setter takes it; the outfits have 3 slots)
    with pytest.raises(HipError, match="presence"):
        eng.score_outfits(tr.data, torch.zeros((2, 3), dtype=torch.int32, device=DEV))
    eng._set_presence_table(None)
    assert L.codae_auc_counts(None, None, 0, None, None, None, 0, 3, None, None, hip.current_stream()) == -1


# ---- AUC counts -------------------------------------------------------------------------------------------------------------
# the last two: one whole staged chunk of positives plus a ragged one, and 300 negatives past the first trip of the capped grid
AUC_PM = [(37, 53), (3000, 5000), (1, 1), (5, 2048 * 256 + 300), (1030, 2048 * 256 + 300)]


@pytest.mark.parametrize("P,M", AUC_PM)
def test_auc_counts_equal_numpy_exactly(hip, P, M):
    from codae.tool import Compatibility
    n_slots = 4
    pos, neg, neg_slot, neg_parent = R.tricky_scores(P, M, n_slots, seed=P, empty_slot=2)
    if P >= 8:                                                                # (tricky_scores plants them in vectors of 8 and more)
        assert np.isnan(pos).any() and np.isinf(pos).any()
    if P > 1:
        assert np.isnan(neg).any() and np.isinf(neg).any()
    pos_on = (np.random.default_rng(2).random(P) > 0.2).astype(np.uint8)
    neg_slot_bad = neg_slot.copy()
    neg_slot_bad[::11] = -1
    for on, sl, par in ((None, neg_slot, neg_parent), (pos_on, neg_slot_bad, neg_parent), (None, neg_slot, None)):
        ref = R.auc_counts_fast(pos, neg, sl, n_slots, par, on)
        run = lambda: Compatibility.auc(torch.tensor(pos).to(DEV), torch.tensor(neg).to(DEV), torch.tensor(sl).to(DEV), n_slots,
                                        neg_parent=None if par is None else torch.tensor(par).to(DEV),
                                        pos_on=None if on is None else torch.tensor(on).to(DEV))
        a, b = run().cpu().numpy(), run().cpu().numpy()
        assert np.array_equal(a, ref) and np.array_equal(a, b)
        # an unaligned view of the positives takes the scalar loads: the same counts
        if P > 1 and par is not None:
            c = Compatibility.auc(torch.tensor(np.concatenate([[0], pos]).astype(np.float32)).to(DEV)[1:], torch.tensor(neg).to(DEV),
                                  torch.tensor(sl).to(DEV), n_slots, neg_parent=torch.tensor(par).to(DEV),
                                  pos_on=None if on is None else torch.tensor(on).to(DEV))
            assert np.array_equal(c.cpu().numpy(), ref)
    out = Compatibility.summary(torch.tensor(a))
    assert out["per_slot"][2]["pairs"] == 0 and np.isnan(out["per_slot"][2]["auc"])      # pairs 0 -> NaN, not a division fault
    if P > 1:
        assert ref[:n_slots, R.TIES].sum() > 0 and 0 < out["auc"] < 1


# ---- the hand-built design ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_orthogonal_design_on_the_device(hip, precision):
    from codae.tool import WeightAverage
    from codae.train import HipEmbeddingTrainer
    d = R.orthogonal_design()
    N, io = d["N"], 2 * d["E"]
    data = torch.tensor(d["data"].astype(np.float32))
    tr = HipEmbeddingTrainer([(io, io, False), (io, io, False)], data, None, None, 1e-3, 0.0, 1.0, max_batch=64, precision=precision, device=DEV,
                             n_slots=2, weight_average=WeightAverage("ema", decay=0.9))
    zero = np.zeros(io, dtype=np.float32)
    good = [(d["W1"].astype(np.float32), zero), (d["W2"].astype(np.float32), zero)]
    bad = [(-d["W1"].astype(np.float32), zero), (d["W2"].astype(np.float32), zero)]
    cm = tr.compatibility_metrics(list(range(N)), negatives=2, seed=0)
    assert cm.skipped == 0 and cm.P == N

    def sweep(weights="live"):
        for rows in (range(0, 40), range(40, N)):
            cm.add_batch(torch.tensor(list(rows), dtype=torch.int32, device=DEV), weights=weights)
        host = cm.get()
        out = cm.total()
        assert np.array_equal(out["counts"], host["counts"])          # the kernel's counts = the torch form's on the same scores
        assert out["outfits"] == N and out["pairs"] == N * 2 * N and out["skipped"] == 0
        return out["auc"], out["paired_acc"]

    tr.load_params(good)
    sc = tr.score_outfits(cm.pos_items[:N])
    assert float(sc["cos"].min()) > (0.999 if precision == "bf16" else 1 - 1e-5)
    assert sweep() == (1.0, 1.0)
    assert sweep("average") == (1.0, 1.0)                            # (load_params reset the average to the same weights)
    tr.load_average(bad)
    assert sweep("average") == (0.0, 0.0) and sweep("live") == (1.0, 1.0)
    tr.load_params(bad)
    assert sweep() == (0.0, 0.0)
    assert np.isnan(cm.total()["auc"])                               # nothing stored since the last total()
