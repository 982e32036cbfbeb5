"""End-to-end runs of the embedding training script with and without HIP: CODE_CLUSTERS on a real MI355X, on the small synthetic file
of tests/test_gpu_codes_script.py (200 observations around 5 centres, 3 x 64, 2 epochs, bf16): with the key the run ends, logs one
line and writes clusters.npz; with CODES as well both files are written from one encoded bank and the labels are those of a fit done
by hand on the written codes; without the key the run logs and books what a config that never heard of it logs and books."""
import json
import os

import numpy as np
import pytest

from test_gpu_codes_script import _run_dir
from test_gpu_norm_script import _run, _shape

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
KEYS = {"centroids", "cluster", "score", "counts", "objective", "changed", "rows", "layer"}


def _check_file(z, k, iters):
    assert set(z.files) == KEYS
    assert z["centroids"].shape == (k, 64) and z["centroids"].dtype == np.float32
    assert z["cluster"].shape == (200,) and z["cluster"].dtype == np.int64 and ((z["cluster"] >= 0) & (z["cluster"] < k)).all()
    assert z["score"].shape == (200,) and np.isfinite(z["score"]).all()
    assert np.array_equal(z["counts"], np.bincount(z["cluster"], minlength=k))
    assert z["objective"].shape == (iters + 1,) and z["changed"].shape == (iters,) and z["changed"][0] == 200
    assert np.array_equal(z["rows"], np.arange(200)) and int(z["layer"]) == 3


def test_embedding_script_writes_the_clusters_and_is_unchanged_without_the_key(tmp_path):
    rng = np.random.default_rng(1)
    cats = ["top", "bottom", "shoe"]
    S, E, n_obs = len(cats), 64, 200
    centers = rng.standard_normal((5, S * E)).astype(np.float32)
    emb = {}
    for i in range(n_obs):
        v = centers[i % 5] + 0.1 * rng.standard_normal(S * E).astype(np.float32)
        emb["o%04d" % i] = {c: v[s * E:(s + 1) * E].tolist() for s, c in enumerate(cats)}
    (tmp_path / "emb.json").write_text(json.dumps(emb))
    os.makedirs(tmp_path / "log")
    model = {"NORM": {"KIND": "layer", "LAYERS": "hidden", "EPS": 1e-5}, "RESIDUAL": {"LAYERS": "hidden"}}
    # the key alone
    rc, out, book = _run(tmp_path, "clusters", dict(model, CODE_CLUSTERS={"K": 4, "ITERS": 5}))
    assert rc == 0, out[-3000:]
    assert "TRAINING HAS ENDED." in out and "OUTFIT CODES" not in out
    lines = [ln for ln in out.splitlines() if "OUTFIT CLUSTERS:" in ln]
    assert len(lines) == 1 and "OUTFIT CLUSTERS: K 4, 5 iterations, converged_at " in lines[0] and "bank encoded" in lines[0], lines
    assert " empty, bank " in lines[0] and lines[0].rstrip().endswith("clusters.npz")
    run = _run_dir(tmp_path, "clusters")
    assert not os.path.exists(run / "codes.npz")
    _check_file(np.load(run / "clusters.npz"), 4, 5)
    # with CODES as well: both files, one encoded bank, and the labels of a fit done by hand on the written codes
    rc, out2, book2 = _run(tmp_path, "both", dict(model, CODES={"SAVE": True}, CODE_CLUSTERS={"K": 4, "ITERS": 5}))
    assert rc == 0, out2[-3000:]
    lines = [ln for ln in out2.splitlines() if "OUTFIT CLUSTERS:" in ln]
    assert len(lines) == 1 and "bank reused" in lines[0] and len([ln for ln in out2.splitlines() if "OUTFIT CODES" in ln]) == 1
    run = _run_dir(tmp_path, "both")
    codes, z = np.load(run / "codes.npz"), np.load(run / "clusters.npz")
    _check_file(z, 4, 5)
    from codae.tool import CodeClusters
    hand = CodeClusters.fit(torch.tensor(codes["codes"], device="cuda:0"), 4, iters=5, seed=0, precision="bf16")
    assert np.array_equal(hand.assign.cpu().numpy(), z["cluster"])
    assert np.array_equal(hand.changed.cpu().numpy(), z["changed"])
    assert np.allclose(hand.centroids.cpu().numpy(), z["centroids"], rtol=1e-3, atol=1e-5)
    # without the key: no line, no file, the log and the book of a config that never heard of it
    rc, out0, book0 = _run(tmp_path, "plain", dict(model))
    assert rc == 0, out0[-3000:]
    assert "OUTFIT CLUSTERS" not in out0 and not os.path.exists(_run_dir(tmp_path, "plain") / "clusters.npz")
    assert _shape(out) == _shape(out0) and len(_shape(out0)) > 10            # (the clusters line comes behind the end of training)
    assert {k: len(v) for k, v in book0.items()} == {k: len(v) for k, v in book.items()}
    assert all(np.isfinite(book0[k]).all() and np.isfinite(book[k]).all() for k in book0)
