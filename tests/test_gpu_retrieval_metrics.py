"""Retrieval metrics on a real MI355X (codae_retrieval_metrics_batched: prepare, fp32 GEMM + compare-and-count per chunk, finish)
against the per-pair numpy reference: exactly on a design whose positions do not depend on the summation order, within a fixed
number of flipped near-ties on a gaussian one; accumulation and determinism; what a position MEANS (membership in
ComplementRetriever.topk); the bf16-plane GEMM route; the embedding script's HIP: RETRIEVAL_METRICS key."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import retrieval_metrics_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "mui-deepautoencoder_amd", "script")
KS = (1, 5, 10, 50)
INT_FIELDS = [R.PAIRS] + list(range(R.HIT, R.HIT + R.MAX_KS)) + list(range(R.HIST, R.HIST + 32))


@pytest.fixture(scope="module")
def hip():
    from codae import hip as H
    H.lib()
    return H


@pytest.fixture
def f32_gemm_mode(hip, monkeypatch):
    """CODAE_F32_GEMM for one test (native = fp32 MFMA, x3 = three bf16 planes per operand), restored afterwards"""
    def set_mode(mode):
        monkeypatch.setenv("CODAE_F32_GEMM", mode)
        hip.check(hip.lib().codae_reload_env())
    yield set_mode
    monkeypatch.delenv("CODAE_F32_GEMM", raising=False)
    hip.check(hip.lib().codae_reload_env())


class Corr:
    """the two device tables of a Corrupter that add() reads"""

    def __init__(self, d):
        self.mask_table_u8 = torch.tensor(d["table"]).to(torch.uint8).contiguous().to(DEV)
        self.mask_to_use_i32 = torch.tensor(d["mask_to_use"]).to(torch.int32).contiguous().to(DEV)


def _dev(a, dtype=None):
    return torch.tensor(a, dtype=dtype).to(DEV)


_GAUSS = {}


def gaussian():
    """the gaussian design, its float64 reference and the device objects: computed once, shared, never written to"""
    if not _GAUSS:
        d = R.gaussian_design()
        mask_ids = d["mask_to_use"][d["idx"], 1]
        args = (d["inv"], d["val"], None, True, d["table"], mask_ids, d["idx"], d["pred"], KS)
        _GAUSS.update(d=d, ref64=R.reference(*args, np.float64), ref32=R.reference(*args, np.float32), ds=R.Dataset(d["inv"]),
                      corr=Corr(d), pred=_dev(d["pred"]), idx=_dev(d["idx"], torch.int32))
    return _GAUSS


@pytest.mark.parametrize("distinct", [True, False])
@pytest.mark.parametrize("nb_missing", [1, 2])
@pytest.mark.parametrize("with_presence", [True, False])
def test_exact_design_equals_the_reference(hip, distinct, nb_missing, with_presence):
    """chunk 16 over at most 53 items: four chunks, the last one ragged (n % 4 != 0: the scalar tail); B = 37 is no multiple of the
    waves per workgroup nor of the prepare pass's rows per workgroup; all three slots have pairs"""
    from codae.tool import RetrievalMetrics
    d = R.exact_design(nb_missing=nb_missing)
    presence = d["presence"] if with_presence else None
    mask_ids = d["mask_to_use"][d["idx"], 0]
    ref, pairs = R.reference(d["inv"], d["val"], presence, distinct, d["table"], mask_ids, d["idx"], d["pred"], KS, np.float64)
    assert all(ref[c, R.PAIRS] > 0 for c in range(d["S"]))
    rm = RetrievalMetrics(R.Dataset(d["inv"]), d["val"], DEV, ks=KS, presence=presence, distinct=distinct)
    counts = rm._host_tables()[1]
    assert any(n % 4 for n in counts) and min(counts) > 32                            # ragged tails, three chunks or more per slot
    if not with_presence and not distinct:
        assert counts == [53, 53, 53]                                                 # 16 + 16 + 16 + 5
    rm.add(_dev(d["pred"]), _dev(d["idx"], torch.int32), Corr(d), run=0, chunk=16)
    pos = rm.last_positions().numpy()
    want = np.zeros_like(pos)
    for b, c, p, n in pairs:
        want[c, b] = p
    assert np.array_equal(pos, want), np.argwhere(pos != want)[:10]
    got = rm.total()["sums"]
    for f in INT_FIELDS:
        assert np.array_equal(got[:, f], ref[:, f]), (f, got[:, f], ref[:, f])
    for f in (R.RRE, R.RR):
        assert np.all(np.abs(got[:, f] - ref[:, f]) <= 1e-12 * np.abs(ref[:, f])), (f, got[:, f], ref[:, f])


def test_gaussian_several_chunks_all_slots(hip):
    """S = 3, E = 64, N = 3000, V = 700, B = 500, chunk 256.  The reference's fp32 and fp64 evaluations agree on every pair (asserted
    first), so what follows measures the kernel alone: a different fp32 summation order may flip a near-tie, at most 4 of them."""
    from codae.tool import RetrievalMetrics
    g = gaussian()
    d, (ref, pairs64), (_, pairs32) = g["d"], g["ref64"], g["ref32"]
    assert pairs64 == pairs32
    assert all(ref[c, R.PAIRS] > 100 for c in range(d["S"])) and ref[:, R.PAIRS].sum() == d["B"]
    rm = RetrievalMetrics(g["ds"], d["val"], DEV, ks=KS)
    rm.add(g["pred"], g["idx"], g["corr"], run=1, chunk=256)
    got = rm.total()["sums"]
    print("gaussian: kernel", got.sum(axis=0)[:R.HIT + 4], "reference", ref.sum(axis=0)[:R.HIT + 4])
    assert np.array_equal(got[:, R.PAIRS], ref[:, R.PAIRS])
    for f in INT_FIELDS[1:]:
        assert abs(got[:, f].sum() - ref[:, f].sum()) <= 4, (f, got[:, f], ref[:, f])
    assert abs(got[:, R.RRE].sum() - ref[:, R.RRE].sum()) <= 4.0 / (d["V"] - 1)


@pytest.mark.parametrize("chunk", [4096, 1024])
def test_wide_chunks_take_whole_sweeps_and_several_segments(hip, chunk):
    """The count pass takes 2048 columns per wave in whole sweeps of 1024 with all loads in flight, and the rest of a segment one
    16-byte group at a time: V = 2603 items in one chunk is two segments (two whole sweeps; 552 columns in groups and a ragged tail of
    3), in chunks of 1024 two whole sweeps and a 555-column rest.  B = 70 is five prepare workgroups, the last one ragged.  Same cap
    on flipped near-ties as the gaussian test, on positions and sums."""
    from codae.tool import RetrievalMetrics
    d = R.gaussian_design(S=2, E=32, N=2603, V=2603, B=70, seed=11)
    mask_ids = d["mask_to_use"][d["idx"], 0]
    args = (d["inv"], d["val"], None, True, d["table"], mask_ids, d["idx"], d["pred"], KS)
    (ref, pairs64), (_, pairs32) = R.reference(*args, np.float64), R.reference(*args, np.float32)
    assert pairs64 == pairs32 and len(pairs64) == d["B"]
    rm = RetrievalMetrics(R.Dataset(d["inv"]), d["val"], DEV, ks=KS)
    assert rm._host_tables()[1] == [2603, 2603]
    rm.add(_dev(d["pred"]), _dev(d["idx"], torch.int32), Corr(d), run=0, chunk=chunk)
    pos = rm.last_positions().numpy()
    want = np.zeros_like(pos)
    for b, c, p, n in pairs64:
        want[c, b] = p
    assert np.array_equal(pos != 0, want != 0)
    assert int(np.abs(pos - want).sum()) <= 4, np.argwhere(pos != want)[:10]
    got = rm.total()["sums"]
    assert np.array_equal(got[:, R.PAIRS], ref[:, R.PAIRS])
    for f in INT_FIELDS[1:]:
        assert abs(got[:, f].sum() - ref[:, f].sum()) <= 4, (f, got[:, f], ref[:, f])
    assert abs(got[:, R.RRE].sum() - ref[:, R.RRE].sum()) <= 4.0 / (d["V"] - 1)


def test_accumulation_reset_and_determinism(hip):
    from codae.tool import RetrievalMetrics
    g = gaussian()
    d = g["d"]
    rm = RetrievalMetrics(g["ds"], d["val"], DEV, ks=KS)
    half = d["B"] // 2 + 3
    parts = []
    for lo, hi in ((0, half), (half, d["B"])):
        rm.add(g["pred"][lo:hi].contiguous(), g["idx"][lo:hi].contiguous(), g["corr"], run=1, chunk=256)
        parts.append(rm.total()["sums"])
    assert rm.total()["pairs"] == 0                                                  # total() resets
    sweeps = []
    for _ in range(2):
        for lo, hi in ((0, half), (half, d["B"])):
            rm.add(g["pred"][lo:hi].contiguous(), g["idx"][lo:hi].contiguous(), g["corr"], run=1, chunk=256)
        sweeps.append(rm.total(reset=False)["sums"])
        assert np.array_equal(rm.total()["sums"], sweeps[-1])                        # reset=False had left them
    assert sweeps[0].tobytes() == sweeps[1].tobytes()                                # the same bits every run
    both = parts[0] + parts[1]
    for f in INT_FIELDS:
        assert np.array_equal(sweeps[0][:, f], both[:, f])
    assert np.allclose(sweeps[0][:, [R.RRE, R.RR]], both[:, [R.RRE, R.RR]], rtol=1e-14, atol=0)


def test_a_position_means_membership_in_topk(hip):
    """no ties on the gaussian input: p <= k for a pair iff the pair's own item is among the k items ComplementRetriever returns"""
    from codae.tool import ComplementRetriever, RetrievalMetrics
    g = gaussian()
    d = g["d"]
    rm = RetrievalMetrics(g["ds"], d["val"], DEV, ks=KS)
    rm.add(g["pred"], g["idx"], g["corr"], run=1, chunk=256)
    pos = rm.last_positions().numpy()                                                 # [S, B]
    ret = ComplementRetriever(g["ds"], DEV, candidates=d["val"], distinct=True)
    n_in = 0
    for c in range(d["S"]):
        rows = np.nonzero(pos[c])[0]
        assert len(rows) > 100
        top = ret.topk(g["pred"][torch.as_tensor(rows, device=DEV)], c, 50)[0].cpu().numpy()
        own = d["idx"][rows][:, None]
        for k in (1, 10, 50):
            inside = (top[:, :k] == own).any(axis=1)
            assert np.array_equal(inside, pos[c][rows] <= k), (c, k, np.nonzero(inside != (pos[c][rows] <= k))[0][:10])
            n_in += int(inside.sum())
    assert n_in > 100                                                                 # (both sides of the iff are exercised)


def test_headline_width_runs_on_the_bf16_plane_gemm(hip, f32_gemm_mode):
    """E = 512: gemm_f32 hands every k-contiguous product with K in whole 32-deep tiles and 16-byte aligned rows to the bf16-plane
    kernel (gemm_f32x3_takes: no size threshold), device-side row count included - so one tile of pairs per slot is enough.  Against
    the same call on the fp32-MFMA kernel: a few near-ties may flip."""
    from codae.tool import RetrievalMetrics
    d = R.gaussian_design(S=3, E=512, N=600, V=300, B=192, seed=5)
    rm = RetrievalMetrics(R.Dataset(d["inv"]), d["val"], DEV, ks=KS)
    corr, pred, idx = Corr(d), _dev(d["pred"]), _dev(d["idx"], torch.int32)
    rm.add(pred, idx, corr, run=0, chunk=128)
    plane = rm.total()["sums"]
    f32_gemm_mode("native")
    rm.add(pred, idx, corr, run=0, chunk=128)
    native = rm.total()["sums"]
    assert np.array_equal(plane[:, R.PAIRS], native[:, R.PAIRS]) and plane[:, R.PAIRS].sum() == d["B"]
    for i in range(len(KS)):
        assert abs(plane[:, R.HIT + i].sum() - native[:, R.HIT + i].sum()) <= 20
    assert 0 < plane[:, R.HIT].sum() < d["B"]


def _run(cmd, cwd):
    r = subprocess.run([sys.executable] + cmd, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout + r.stderr


def test_embedding_script_logs_and_books_the_metrics(tmp_path):
    """the tiny incomplete-observations run of test_gpu_presence_script.py with HIP: RETRIEVAL_METRICS, and without it"""
    import yaml
    from codae.tool import load_dataset_of_embeddings
    rng = np.random.default_rng(1)
    cats = ["top", "bottom", "shoe", "bag"]
    S, E = len(cats), 16
    centers = rng.standard_normal((5, S * E)).astype(np.float32)
    emb = {}
    for i in range(360):
        v = centers[i % 5] + 0.1 * rng.standard_normal(S * E).astype(np.float32)
        missing = [] if i % 3 == 0 else ([cats[i % S]] if i % 3 == 1 else [c for c in cats if c != cats[i % S]])
        emb["o%04d" % i] = {c: v[s * E:(s + 1) * E].tolist() for s, c in enumerate(cats) if c not in missing}
    (tmp_path / "emb.json").write_text(json.dumps(emb))
    cfg = {"MODEL": {"Z_SIZE": 48, "BATCH_SIZE": 64, "NB_INPUT_LAYER": 2, "NB_OUTPUT_LAYER": 2, "STEEP_LAYER_SIZE": False,
                     "EPOCH": 2, "LEARNING_RATE": 1e-3, "WEIGHT_DECAY": 1e-4, "NB_CORRUPTED": 1, "TRUNK_GRAD": True},
           "DATASET": {"NAME": "EMBEDDING", "USED_CATEGORY": cats, "EMBEDDING_SIZE": E, "SHUFFLE": True, "SPLIT": [0.7, 0.3]},
           "HIP": {"KEEP_INCOMPLETE": True, "MIN_PRESENT": 2, "RETRIEVAL_METRICS": {"K": [1, 5]}},
           "SEED": 27493045}
    # the complete validation rows, by the script's own split
    ds = load_dataset_of_embeddings(str(tmp_path / "emb.json"), cfg, keep_incomplete=True, min_present=2)
    order = list(range(ds.nb_observation))
    np.random.seed(cfg["SEED"])
    np.random.shuffle(order)
    validation = order[int(np.floor(ds.nb_observation * 0.7)):]
    n_complete = int(ds.presence[validation].all(axis=1).sum())
    assert 0 < n_complete < len(validation)
    os.makedirs(tmp_path / "log")
    books = {}
    for name, with_key in (("with", True), ("without", False)):
        if not with_key:
            del cfg["HIP"]["RETRIEVAL_METRICS"]
        (tmp_path / ("%s.yaml" % name)).write_text(yaml.safe_dump(cfg))
        out = _run([os.path.join(SCRIPTS, "train_dae_on_embedding.py"), "--embedding_path", "emb.json", "--output_path", name,
                    "--config", "%s.yaml" % name, "--precision", "f32"], cwd=str(tmp_path))
        assert "TRAINING HAS ENDED." in out and "VALIDATION RANKING ERROR" in out
        assert ("VALIDATION MRR" in out) == ("VALIDATION HIT@5" in out) == ("VALIDATION RANKED PAIRS" in out) == with_key
        books[name] = json.load(open(tmp_path / name / os.listdir(tmp_path / name)[0] / "book.json"))
    assert set(books["without"]) == {"ftl", "ptl", "fvl", "pvl", "rl"}
    book = books["with"]
    assert set(book) == {"ftl", "ptl", "fvl", "pvl", "rl", "mrr", "hit@1", "hit@5", "ranked_pairs"}
    assert all(len(book[k]) == 2 and np.isfinite(book[k]).all() for k in book)
    for e in range(2):
        assert 0 <= book["hit@1"][e] <= book["hit@5"][e] <= 1 and 0 < book["mrr"][e] <= 1
        assert n_complete < book["ranked_pairs"][e] <= len(validation)
