"""Outfit codes on a real MI355X (include/codae_hip.h, "Outfit codes"): the export kernel on its own, bit for bit; the code of both
engines against tests/norm_ref.py's hs[k]; the bit-exact invariants (decode of encode = the evaluation forward, rows = assembled
items, chunks, two calls); the state a call leaves alone; nearest neighbours in code space against a brute-force float64 cosine
ranking of the oracle's codes; refusals, inference from a checkpoint, and a NaN.

Tolerances.  Export: dst exact; norm against float64 of the same stored values, the project's rtol 1e-3 / atol 1e-5.  fp32 engine:
rtol 1e-3 / atol 1e-5 against the float64 statement.  bf16 engine: 2e-3 relative L2 against the restatement with the engine's
roundings (tests/test_gpu_parity.py's bound at fixture size).  Search: rtol 1e-3 / atol 1e-5 on the scores.
"""
import numpy as np
import pytest

import norm_ref as NR
from golden_util import close, max_err
from test_gpu_norm import (DEV, EPS, POISON, ROWS, SHAPES, SHAPE_IDS, _bits32, _flags, _idx, _norm, _problem, _raw, _rel_l2, _res, _same,
                           _skips, _snapshot, _square, _trainer, _work)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
E, S = 8, 3                         # the fixtures' slots: 3 x 8 = 24 columns


# ---- the export kernel alone ---------------------------------------------------------------------------------------------------------

def _export(src, bf16, ld_src, B, width, dst, ld_dst, norm):
    from codae import hip
    rc = hip.lib().codae_export_rows(hip.ptr(src), int(bf16), ld_src, B, width, hip.ptr(dst), ld_dst, hip.ptr(norm), hip.current_stream())
    torch.cuda.synchronize()
    return rc


def _source(rng, B, width, ld, bf16):
    """standard normal with 15 % exact zeros, one -0.0, (B >= 2) one all-zero row and (B >= 3) one row holding a NaN; pad columns and
    two pad rows poisoned -> (device tensor of the working type, its values widened to fp32, the NaN row or None)"""
    a = np.full((B + 2, ld), POISON, dtype=np.float32)
    a[:B, :width] = rng.standard_normal((B, width)).astype(np.float32)
    a[:B, :width][rng.random((B, width)) < 0.15] = 0.0
    a[0, 0] = -0.0
    nan_row = None
    if B >= 2:
        a[B - 1, :width] = 0.0
    if B >= 3:
        nan_row = B // 2
        a[nan_row, width // 2] = np.nan
    t, w = _work(a, bf16)
    return t, w, nan_row


@pytest.mark.parametrize("bf16,width,ld_src", SHAPES, ids=SHAPE_IDS)
def test_export_kernel_copies_exactly_and_leaves_the_row_norms(bf16, width, ld_src):
    from codae import hip
    rng = np.random.default_rng(width * 7 + int(bf16))
    for B in ROWS:
        for ld_dst in (width, width + 3):
            src, a, nan_row = _source(rng, B, width, ld_src, bf16)
            before = src.clone()
            dst = torch.full((B + 2, ld_dst), POISON, dtype=torch.float32, device=DEV)
            norm = torch.full((B + 1,), POISON, dtype=torch.float32, device=DEV)
            assert _export(src, bf16, ld_src, B, width, dst, ld_dst, norm) == 0, hip.lib().codae_last_error()
            got, gn = dst.cpu().numpy(), norm.cpu().numpy()
            assert np.array_equal(_bits32(got[:B, :width]), _bits32(a[:B, :width])), (B, ld_dst, "dst bits")     # -0.0 and the NaN included
            assert _bits32(got[0, 0]) == 0x80000000
            assert (got[:, width:] == POISON).all() and (got[B:] == POISON).all() and gn[B] == POISON
            assert torch.equal(_raw(src), _raw(before))
            with np.errstate(invalid="ignore"):
                ref = np.sqrt((a[:B, :width].astype(np.float64) ** 2).sum(axis=1))
            ok = np.ones(B, dtype=bool)
            if nan_row is not None:
                ok[nan_row] = False
                assert np.isnan(gn[nan_row]) and np.isfinite(gn[nan_row - 1]) and np.isfinite(gn[nan_row + 1])
            assert np.isfinite(gn[:B][ok]).all()
            assert close(gn[:B][ok], ref[ok]), (B, ld_dst, max_err(gn[:B][ok], ref[ok]))
            if B >= 2:
                assert _bits32(gn[B - 1]) == 0                                                                  # the all-zero row: +0
            # a row alone, at another position and with other leading dimensions (the other access path): the same norm bits
            r = 0 if B < 3 else B // 2 + 1
            ld2 = ld_src + 1
            alone = np.full((3, ld2), POISON, dtype=np.float32)
            alone[:, :width] = 0.5
            alone[2, :width] = a[r, :width]
            src2, _ = _work(alone, bf16)
            dst2 = torch.full((3, width + 1), POISON, dtype=torch.float32, device=DEV)
            norm2 = torch.full((3,), POISON, dtype=torch.float32, device=DEV)
            assert _export(src2, bf16, ld2, 3, width, dst2, width + 1, norm2) == 0
            assert _bits32(norm2.cpu().numpy()[2]) == _bits32(gn[r]), (B, ld_dst, "norm bits of a row alone")
            assert np.array_equal(_bits32(dst2.cpu().numpy()[2, :width]), _bits32(a[r, :width]))
            # without a norm buffer: the same dst bits
            dst3 = torch.full((B + 2, ld_dst), POISON, dtype=torch.float32, device=DEV)
            assert _export(src, bf16, ld_src, B, width, dst3, ld_dst, None) == 0
            assert torch.equal(dst3.view(torch.int32), dst.view(torch.int32))


def test_export_launcher_refuses_bad_arguments():
    from codae import hip
    lib = hip.lib()
    src = torch.ones((4, 8), device=DEV)
    dst = torch.zeros((4, 8), device=DEV)
    n = torch.zeros((4,), device=DEV)

    def refused(rc, word):
        return rc != 0 and word in lib.codae_last_error().decode()
    assert refused(_export(src, 0, 4, 4, 8, dst, 8, n), "ld_src")                 # ld_src < width
    assert refused(_export(src, 0, 8, 4, 8, dst, 4, n), "ld_dst")
    assert refused(_export(src, 0, 8, 0, 8, dst, 8, n), "B 0")
    assert refused(_export(src, 0, 8, 4, 0, dst, 8, n), "width 0")
    assert refused(_export(None, 0, 8, 4, 8, dst, 8, n), "null")
    assert refused(_export(src, 0, 8, 4, 8, None, 8, n), "null")
    assert refused(_export(dst, 0, 8, 4, 8, dst, 8, n), "aliased")
    assert refused(_export(src, 2, 8, 4, 8, dst, 8, n), "bf16")
    assert float(dst.abs().max()) == 0 and float(n.abs().max()) == 0 and float((src - 1).abs().max()) == 0      # a refusal launches nothing


# ---- the code against the oracle ---------------------------------------------------------------------------------------------------

CONFIGS = {"plain": (None, None), "norm": ("layer", None), "skips": (None, "hidden"), "both": ("layer", "hidden")}


def _kw(kind, skip_layers):
    kw = {}
    if kind is not None:
        kw["norm"] = _norm(kind)
    if skip_layers is not None:
        kw["residual"] = _res(skip_layers)
    return kw


def _model(p, kind, skip_layers):
    """(skips, norm flags, kind) of a configuration, as norm_ref.forward takes them"""
    return _skips(p, skip_layers), (_flags(p, "hidden") if kind is not None else [0] * p["L"]), (kind or "layer")


def _hs(p, params, kind, skip_layers, x, bf16=False):
    skips, flags, kd = _model(p, kind, skip_layers)
    return NR.forward(params, p["names"], skips, flags, kd, EPS, x, bf16=bf16)[1]


def _blanked(x, c):
    x = x.copy()
    x[:, c * E:(c + 1) * E] = 0
    return x


@pytest.mark.parametrize("config", list(CONFIGS))
def test_f32_code_is_h_k_of_the_float64_statement_l5_w24_b70(config):
    kind, skip_layers = CONFIGS[config]
    p = _square(5, 24, 70, "relu", seed=101)
    t = _trainer(p, "f32", **_kw(kind, skip_layers))
    rows = p["order"][0]
    x = p["data"][rows]
    first = {"plain": 99, "norm": 1, "skips": 2, "both": 1}[config]           # the lowest k the skips / the norm change h_k at
    for blank, c in ((None, x), (1, _blanked(x, 1))):
        hs, plain = _hs(p, p["params"], kind, skip_layers, c), _hs(p, p["params"], None, None, c)
        for k in range(1, 5):
            code = t.encode(_idx(p, 0), blank=blank, layer=k).cpu().numpy()
            assert code.shape == (70, 24) and t.code_width(k) == 24
            print(config, "blank", blank, "k", k, "worst / tolerance", max_err(code, hs[k]))
            assert close(code, hs[k]), (blank, k, max_err(code, hs[k]))
            if k >= first:                                                    # ... and not the stack without them
                assert not close(code, plain[k]), (blank, k)


def test_f32_default_layer_is_the_activation_free_one_of_a_taper_rms():
    from codae.hip import HipError
    p = _problem([24, 16, 8, 16, 24], ["relu", None, "relu", None], 70, seed=102)
    t = _trainer(p, "f32", norm=_norm("rms"))
    assert t.code_layers == 2 and t.code_width() == 8
    rows = p["order"][0]
    x = p["data"][rows]
    for blank, c in ((None, x), (1, _blanked(x, 1))):
        hs = _hs(p, p["params"], "rms", None, c)
        code = t.encode(_idx(p, 0), blank=blank).cpu().numpy()
        assert code.shape == (70, 8)
        assert close(code, hs[2]), max_err(code, hs[2])
        assert not close(code, _hs(p, p["params"], None, None, c)[2])
    sq = _trainer(_square(5, 24, 70, "relu", seed=101), "f32")
    with pytest.raises(HipError, match="no default code layer"):
        sq.code_layers
    with pytest.raises(HipError, match="no default code layer"):
        sq.encode(_idx(p, 0))


def test_f32_code_on_the_averaged_weights_l5_w24_b70():
    from codae.tool import WeightAverage
    p = _square(5, 24, 70, "relu", seed=103)
    t = _trainer(p, "f32", weight_average=WeightAverage("ema", decay=0.5), **_kw("layer", "hidden"))
    for s in range(2):
        t.train_batch(_idx(p, s), run=0)
    x = p["data"][p["order"][2]]
    avg = [(w.cpu().numpy(), b.cpu().numpy()) for w, b in t.params(average=True)]
    live = [(w.cpu().numpy(), b.cpu().numpy()) for w, b in t.params()]
    for k in range(1, 5):
        ca = t.encode(_idx(p, 2), layer=k, weights="average").cpu().numpy()
        cl = t.encode(_idx(p, 2), layer=k).cpu().numpy()
        assert close(ca, _hs(p, avg, "layer", "hidden", x)[k]), (k, max_err(ca, _hs(p, avg, "layer", "hidden", x)[k]))
        assert close(cl, _hs(p, live, "layer", "hidden", x)[k]), k
        assert not np.array_equal(ca, cl), k


BF16_STACKS = [("square-plain", [24] * 6, ["relu"] * 4 + [None], None, None, (1, 2, 3, 4)),
               ("square-norm", [24] * 6, ["relu"] * 4 + [None], "layer", None, (1, 2, 3, 4)),
               ("square-skips", [24] * 6, ["relu"] * 4 + [None], None, "hidden", (1, 2, 3, 4)),
               ("square-both", [24] * 6, ["relu"] * 4 + [None], "layer", "hidden", (1, 2, 3, 4)),
               ("taper-rms", [24, 16, 8, 16, 24], ["relu", None, "relu", None], "rms", None, (None,))]


@pytest.mark.parametrize("name,widths,acts,kind,skip_layers,ks", BF16_STACKS, ids=[c[0] for c in BF16_STACKS])
def test_bf16_code_matches_the_rounded_restatement_and_is_bf16_valued(name, widths, acts, kind, skip_layers, ks):
    p = _problem(widths, acts, 70, seed=104)
    t = _trainer(p, "bf16", **_kw(kind, skip_layers))
    x = p["data"][p["order"][0]]
    for blank, c in ((None, x), (1, _blanked(x, 1))):
        hs = _hs(p, p["params"], kind, skip_layers, c, bf16=True)
        for k in ks:
            code = t.encode(_idx(p, 0), blank=blank, layer=k)
            kk = t.code_layers if k is None else k
            assert tuple(code.shape) == (70, widths[kk])
            assert int((code.view(torch.int32) & 0xFFFF).abs().max()) == 0          # bf16 numbers widened: the low 16 bits are zero
            err = _rel_l2(code.cpu().numpy(), hs[kk])
            print("MEASURE bf16 code, %s, blank %s, k %d: relative L2 %.3e" % (name, blank, kk, err))
            assert err <= 2e-3, (name, blank, kk, err)


# ---- bit-exact invariants -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("config", ["plain", "both"])
@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_decode_of_encode_is_the_evaluation_forward_and_calls_agree_bit_for_bit(precision, config):
    c = 1
    p = _square(5, 24, 70, "relu", seed=105)
    p["mtu"][:] = c                                                           # every row's mask of run 0 is the one-slot mask {c}
    kw = _kw(*CONFIGS[config])
    t = _trainer(p, precision, **kw)
    rows = _idx(p, 0)
    y = t.eval_batch(rows, run=0, want_y=True)
    for k in range(1, 5):
        z = t.encode(rows, blank=c, layer=k)
        back = t.decode(z, layer=k)
        assert torch.equal(back.view(torch.int32), y.view(torch.int32)), (k, float((back - y).abs().max()))
        assert torch.equal(t.encode(rows, blank=c, layer=k).view(torch.int32), z.view(torch.int32)), k       # two calls: the same bits
    # resident rows = the assembled outfit [r, r, r]
    whole = t.encode(rows, layer=2)
    items = rows[:, None].expand(-1, S).contiguous()
    assert torch.equal(t.encode_items(items, layer=2).view(torch.int32), whole.view(torch.int32))
    both, norms = t.encode(rows, layer=2, want_norm=True)
    assert torch.equal(both.view(torch.int32), whole.view(torch.int32))
    assert close(norms.cpu().numpy(), np.linalg.norm(whole.cpu().numpy().astype(np.float64), axis=1))
    # 70 rows through max_batch 32: the concatenation of its three chunk calls
    small = _trainer(p, precision, max_batch=32, **kw)
    z70 = small.encode(rows, blank=c, layer=3)
    parts = torch.cat([small.encode(rows[o:o + 32], blank=c, layer=3) for o in (0, 32, 64)])
    assert tuple(z70.shape) == (70, 24) and torch.equal(z70.view(torch.int32), parts.view(torch.int32))
    y70 = small.decode(z70, layer=3)
    yparts = torch.cat([small.decode(z70[o:o + 32], layer=3) for o in (0, 32, 64)])
    assert tuple(y70.shape) == (70, 24) and torch.equal(y70.view(torch.int32), yparts.view(torch.int32))


# ---- state is untouched -------------------------------------------------------------------------------------------------------------

def _use_codes(t, p):
    rows = _idx(p, 1)
    z = t.encode(rows, blank=0, layer=2)
    t.decode(z, layer=2)
    index = t.code_index(layer=2)
    index.similar(z, 3, exclude=rows)
    torch.cuda.synchronize()


def test_codes_leave_the_trainers_state_alone_w24_b70():
    p = _square(5, 24, 70, "relu", seed=106)
    t = _trainer(p, "bf16", **_kw("layer", "hidden"))
    t.train_batch(_idx(p, 0), run=0)
    t.eval_batch(_idx(p, 1), run=0)                                           # (the metric sums hold something)
    dig, scal, sums = t.state_digest(), t.engine.scalars.clone(), t.epoch_sums(reset=False)
    _use_codes(t, p)
    assert t.state_digest() == dig
    assert torch.equal(t.engine.scalars.view(torch.int64), scal.view(torch.int64))
    assert t.epoch_sums(reset=False) == sums


@pytest.mark.parametrize("use_graph", [False, True], ids=["plain", "graph"])
def test_a_step_an_encode_and_a_step_are_two_steps_w24_b70(use_graph):
    p = _square(5, 24, 70, "relu", seed=107)
    mk = lambda: _trainer(p, "bf16", use_graph=use_graph, **_kw("layer", "hidden"))
    a, b = mk(), mk()
    a.train_batch(_idx(p, 0), run=0)
    _use_codes(a, p)
    a.train_batch(_idx(p, 1), run=0)
    for s in range(2):
        b.train_batch(_idx(p, s), run=0)
    _same(_snapshot(a), _snapshot(b))
    assert a.state_digest() == b.state_digest()


# ---- search ---------------------------------------------------------------------------------------------------------------------------

def _cosines(codes, queries=None):
    c = np.asarray(codes, dtype=np.float64)
    q = c if queries is None else np.asarray(queries, dtype=np.float64)
    return (q / np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-8)) @ (c / np.maximum(np.linalg.norm(c, axis=1, keepdims=True), 1e-8)).T


def test_similar_is_the_brute_force_cosine_ranking_of_the_oracles_codes_f32():
    k, layer = 4, 2
    p = _square(5, 24, 70, "relu", seed=108)                                  # 120 rows of uniform noise: duplicate-free
    N = p["N"]
    assert N == 120 and len({r.tobytes() for r in p["data"]}) == N
    t = _trainer(p, "f32", **_kw("layer", "hidden"))
    oracle = _hs(p, p["params"], "layer", "hidden", p["data"])[layer]
    index = t.code_index(layer=layer)
    assert len(index) == N and index.width == 24 and index.layer == layer
    assert close(index.bank.cpu().numpy(), oracle)
    assert close(index.norm.cpu().numpy(), np.linalg.norm(oracle, axis=1))
    rows = torch.arange(N, dtype=torch.int32, device=DEV)
    query = t.encode(rows, layer=layer)
    assert torch.equal(query.view(torch.int32), index.bank.view(torch.int32))
    cos = _cosines(oracle)
    idx, score = index.similar(query, k)
    gi, gs = idx.cpu().numpy(), score.cpu().numpy()
    want = -np.sort(-cos, axis=1)[:, :k]
    assert close(gs, want), max_err(gs, want)
    assert close(np.take_along_axis(cos, gi, axis=1), gs)                     # the true cosines at the returned rows (immune to near ties)
    assert (gi[:, 0] == np.arange(N)).all() and (np.abs(gs[:, 0] - 1.0) <= 1e-5).all()
    assert (np.diff(gs, axis=1) <= 0).all()
    # neighbours other than the outfit itself
    idx, score = index.similar(query, k, exclude=rows)
    gi, gs = idx.cpu().numpy(), score.cpu().numpy()
    off = cos.copy()
    np.fill_diagonal(off, -np.inf)
    want = -np.sort(-off, axis=1)[:, :k]
    assert (gi != np.arange(N)[:, None]).all() and (gi >= 0).all()
    assert close(gs, want), max_err(gs, want)
    assert close(np.take_along_axis(cos, gi, axis=1), gs)
    # a partial outfit ("these two items, any top"): valid rows, ordered scores, the oracle's cosines of the blanked input
    part = t.encode(rows[:9], blank=0, layer=layer)
    pc = _cosines(oracle, _hs(p, p["params"], "layer", "hidden", _blanked(p["data"][:9], 0))[layer])
    idx, score = index.similar(part, k)
    gi, gs = idx.cpu().numpy(), score.cpu().numpy()
    assert ((gi >= 0) & (gi < N)).all() and np.isfinite(gs).all() and (np.diff(gs, axis=1) <= 0).all()
    assert close(gs, -np.sort(-pc, axis=1)[:, :k]) and close(np.take_along_axis(pc, gi, axis=1), gs)
    # a bank over chosen rows answers in dataset rows
    sub = t.code_index(rows=[50, 7, 99, 3], layer=layer)
    idx, score = sub.similar(query[[7, 3]], 4, exclude=torch.tensor([7, 3]))
    assert sorted(idx[0].tolist()) == [-1, 3, 50, 99] and sorted(idx[1].tolist()) == [-1, 7, 50, 99]
    assert idx[0, 3] == -1 and score[0, 3] == float("-inf")


def test_duplicated_rows_fold_under_distinct_and_stay_apart_without_f32():
    p = _square(5, 24, 70, "relu", seed=109)
    data = p["data"].copy()
    data[5] = data[3]
    data[77] = data[3]
    t = _trainer(dict(p, data=data), "f32", **_kw("layer", "hidden"))
    q = t.encode(torch.tensor([3]), layer=2)
    idx, score = t.code_index(layer=2, distinct=True).similar(q, 5)
    got = idx[0].tolist()
    assert got[0] == 3 and 5 not in got and 77 not in got and len(set(got)) == 5
    idx, score = t.code_index(layer=2, distinct=False).similar(q, 5)
    assert idx[0, :3].tolist() == [3, 5, 77]                                 # the same bytes, the same score: ascending row
    assert float(score[0, 0]) == float(score[0, 1]) == float(score[0, 2])
    # with `distinct`, excluding a row excludes the entry it belongs to
    idx, _ = t.code_index(layer=2, distinct=True).similar(q, 5, exclude=torch.tensor([77]))
    assert not {3, 5, 77} & set(idx[0].tolist())


def test_absent_slots_encode_as_zeros_f32():
    p = _square(5, 24, 70, "relu", seed=110)
    rng = np.random.default_rng(7)
    table = (rng.random((p["N"], S)) < 0.7).astype(np.uint8)
    table[np.arange(p["N"]), rng.integers(0, S, p["N"])] = 1                   # every row has an item
    from codae.tool import SlotPresence
    t = _trainer(p, "f32", presence=SlotPresence(table), **_kw("layer", "hidden"))
    rows = p["order"][0]
    assert (table[rows] == 0).any()
    x = p["data"][rows] * np.repeat(table[rows], E, axis=1)
    code = t.encode(_idx(p, 0), layer=2).cpu().numpy()
    want = _hs(p, p["params"], "layer", "hidden", x)[2]
    assert close(code, want), max_err(code, want)
    assert not close(code, _hs(p, p["params"], "layer", "hidden", p["data"][rows])[2])
    # assembled: items of three different rows, one of them named absent
    items = np.stack([p["order"][1][:12], p["order"][2][:12], p["order"][3][:12]], axis=1)
    items[4, 1] = -1
    on = np.stack([table[np.maximum(items[:, s], 0), s] for s in range(S)], axis=1) * (items >= 0)
    xq = np.concatenate([p["data"][np.maximum(items[:, s], 0), s * E:(s + 1) * E] * on[:, s:s + 1] for s in range(S)], axis=1)
    code = t.encode_items(torch.tensor(items), blank=torch.tensor([2] + [-1] * 11), layer=2).cpu().numpy()
    xq[0, 2 * E:] = 0
    want = _hs(p, p["params"], "layer", "hidden", xq)[2]
    assert close(code, want), max_err(code, want)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_trainer_unchanged():
    from codae.hip import HipError
    p = _square(5, 24, 70, "relu", seed=111)
    t = _trainer(p, "f32", **_kw("layer", "hidden"))
    t.train_batch(_idx(p, 0), run=0)
    dig = t.state_digest()
    rows = _idx(p, 1)
    for bad in (0, 5, -1, True, 2.0):
        with pytest.raises(HipError, match="layer"):
            t.encode(rows, layer=bad)
        with pytest.raises(HipError, match="layer"):
            t.decode(torch.zeros((4, 24), device=DEV), layer=bad)
    with pytest.raises(HipError, match="Q >= 1"):
        t.encode(rows[:0], layer=2)
    with pytest.raises(HipError, match="Q >= 1"):
        t.decode(torch.zeros((0, 24), device=DEV), layer=2)
    with pytest.raises(HipError, match="no weight average"):
        t.encode(rows, layer=2, weights="average")
    with pytest.raises(HipError, match="no weight average"):
        t.decode(torch.zeros((4, 24), device=DEV), layer=2, weights="average")
    with pytest.raises(HipError, match="blank"):
        t.encode(rows, blank=3, layer=2)
    with pytest.raises(HipError, match=r"\[Q, 24\]"):
        t.decode(torch.zeros((4, 23), device=DEV), layer=2)
    index = t.code_index(layer=2)
    with pytest.raises(HipError, match="query"):
        index.similar(torch.zeros((4, 23), device=DEV), 3)
    # the library's own checks
    from codae import hip
    import ctypes as C
    eng = t.engine
    x = torch.zeros((4, 24), device=DEV)
    out = torch.zeros((4, 24), device=DEV)
    lib = hip.lib()
    for args in ((4, 0), (4, 5), (0, 2), (71, 2)):
        assert lib.codae_encode(eng._h, C.byref(eng.bufs), hip.ptr(x), args[0], args[1], hip.ptr(out), None, hip.current_stream()) != 0
        assert lib.codae_decode(eng._h, C.byref(eng.bufs), hip.ptr(x), args[0], args[1], hip.ptr(out), hip.current_stream()) != 0
    assert lib.codae_encode(eng._h, C.byref(eng.bufs), None, 4, 2, hip.ptr(out), None, hip.current_stream()) != 0
    assert lib.codae_decode(eng._h, C.byref(eng.bufs), hip.ptr(x), 4, 2, None, hip.current_stream()) != 0
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0
    with pytest.raises(HipError, match="are on: a forward over the layer range"):      # the partial drop-in forward stays refused
        eng.forward(torch.tensor(p["data"][:70], device=DEV), 0, 2)
    assert t.state_digest() == dig


# ---- inference --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_load_for_inference_gives_the_writers_codes(tmp_path, precision):
    from codae.train import HipEmbeddingTrainer
    p = _square(5, 24, 70, "relu", seed=112)
    t = _trainer(p, precision, **_kw("rms", "hidden"))
    for s in range(2):
        t.train_batch(_idx(p, s), run=0)
    path = str(tmp_path / "ck.codae")
    t.save(path)
    inf = HipEmbeddingTrainer.load_for_inference(path, torch.tensor(p["data"]), torch.tensor(p["bm"]).to(torch.uint8), torch.tensor(p["mtu"]),
                                                 n_slots=p["S"], max_batch=70, device=DEV)
    for blank in (None, 2):
        a, b = t.encode(_idx(p, 3), blank=blank, layer=3), inf.encode(_idx(p, 3), blank=blank, layer=3)
        assert float(a.abs().max()) > 0 and torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(t.decode(a, layer=3).view(torch.int32), inf.decode(b, layer=3).view(torch.int32))


# ---- non-finite -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_a_nan_row_has_a_nan_code_and_no_other_row_has_w24(precision):
    p = _square(5, 24, 70, "relu", seed=113)
    data = p["data"].copy()
    bad = 17
    data[bad, 9] = np.nan
    t = _trainer(dict(p, data=data), precision, **_kw("layer", "hidden"))
    rows = torch.arange(p["N"], dtype=torch.int32, device=DEV)
    code, norm = t.encode(rows, layer=2, want_norm=True)
    c, n = code.cpu().numpy(), norm.cpu().numpy()
    assert np.isnan(c[bad]).all() and np.isfinite(np.delete(c, bad, axis=0)).all()
    assert np.isnan(n[bad]) and np.isfinite(np.delete(n, bad)).all()
    index = t.code_index(layer=2)
    idx, score = index.similar(code, 4)
    gi, gs = idx.cpu().numpy(), score.cpu().numpy()
    assert not np.isnan(gs).any()
    assert (gi[bad] == -1).all() and np.isneginf(gs[bad]).all()              # a NaN query has no neighbour
    assert not (np.delete(gi, bad, axis=0) == bad).any()                      # and the NaN row is nobody's
