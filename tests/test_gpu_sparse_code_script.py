"""End-to-end runs of the embedding training script with and without HIP: SPARSE_CODE on a real MI355X, on a small synthetic file of
the reference's input schema (tests/test_gpu_norm_script.py's harness: 200 observations, 3 x 64, 2 epochs, bf16): with the key the
run trains through the sparse code, logs one line and writes codes.npz whose rows are keep-sparse; without it two runs log and book
what a config that never heard of the key logs and books."""
import json
import os

import numpy as np
import pytest

from test_gpu_codes_script import _run_dir
from test_gpu_norm_script import _run, _shape

pytestmark = pytest.mark.gpu


def test_embedding_script_trains_through_the_sparse_code_and_is_unchanged_without_the_key(tmp_path):
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
    rc, out, book = _run(tmp_path, "sparse", {"SPARSE_CODE": {"KEEP": 8, "LAYER": None}, "CODES": {"SAVE": True}})
    assert rc == 0, out[-3000:]
    assert "TRAINING HAS ENDED." in out
    lines = [ln for ln in out.splitlines() if "SPARSE CODE:" in ln]
    assert len(lines) == 1 and lines[0].rstrip().endswith("SPARSE CODE: keep 8 of 64 at layer 3"), lines
    z = np.load(_run_dir(tmp_path, "sparse") / "codes.npz")
    assert z["codes"].shape == (200, 64) and int(z["layer"]) == 3 and np.isfinite(z["codes"]).all()
    nnz = (z["codes"] != 0).sum(axis=1)
    assert nnz.max() <= 8 and nnz.min() >= 1, (nnz.min(), nnz.max())
    assert len(book["ftl"]) == 2 and all(np.isfinite(book[k]).all() for k in book)
    # an unknown key is refused before training starts
    rc, bad, _ = _run(tmp_path, "bad", {"SPARSE_CODE": {"KEEP": 8, "PENALTY": 0.1}})
    assert rc != 0 and "SPARSE_CODE: unknown key(s) PENALTY" in bad
    # without the key: no line, and two runs log and book alike (the script draws unseeded weights: digits masked)
    rc, out0, book0 = _run(tmp_path, "plain", None)
    assert rc == 0, out0[-3000:]
    rc, out1, book1 = _run(tmp_path, "again", None)
    assert rc == 0, out1[-3000:]
    assert "SPARSE CODE" not in out0 and "SPARSE CODE" not in out1
    assert _shape(out0) == _shape(out1) and len(_shape(out0)) > 10
    assert [ln for ln in _shape(out) if not ln.startswith("SPARSE CODE:")] == _shape(out0)   # the line is all the key adds to the training log
    assert {k: len(v) for k, v in book0.items()} == {k: len(v) for k, v in book1.items()} == {k: len(v) for k, v in book.items()}
    assert all(np.isfinite(book0[k]).all() and np.isfinite(book1[k]).all() for k in book0)
