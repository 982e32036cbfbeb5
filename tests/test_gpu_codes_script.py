"""End-to-end runs of the embedding training script with and without HIP: CODES on a real MI355X, on a small synthetic file of the
reference's input schema (tests/test_gpu_norm_script.py's harness: 200 observations, 3 x 64, 2 epochs, bf16): with the key the run
ends, logs one line and writes codes.npz with every row's code and its nearest other rows; without it the run logs and books what a
config that never heard of the key logs and books, and writes no codes."""
import json
import os

import numpy as np
import pytest

from test_gpu_norm_script import _run, _shape

pytestmark = pytest.mark.gpu


def _run_dir(tmp_path, name):
    runs = os.listdir(tmp_path / ("out_" + name))
    assert len(runs) == 1
    return tmp_path / ("out_" + name) / runs[0]


def test_embedding_script_writes_the_codes_and_is_unchanged_without_the_key(tmp_path):
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
    rc, out, book = _run(tmp_path, "codes", dict(model, CODES={"SAVE": True, "NEIGHBOURS": 3}))
    assert rc == 0, out[-3000:]
    assert "TRAINING HAS ENDED." in out
    lines = [ln for ln in out.splitlines() if "OUTFIT CODES" in ln]
    assert len(lines) == 1 and "OUTFIT CODES: [200, 64] layer 3 -> " in lines[0] and lines[0].rstrip().endswith("codes.npz"), lines
    z = np.load(_run_dir(tmp_path, "codes") / "codes.npz")
    assert z["codes"].shape == (200, 64) and z["codes"].dtype == np.float32 and np.isfinite(z["codes"]).all()
    assert np.array_equal(z["rows"], np.arange(200)) and int(z["layer"]) == 3
    ni, ns = z["neighbour_idx"], z["neighbour_score"]
    assert ni.shape == (200, 3) and ns.shape == (200, 3)
    assert ((ni >= 0) & (ni < 200)).all() and (ni != np.arange(200)[:, None]).all()
    assert np.isfinite(ns).all() and (np.diff(ns, axis=1) <= 0).all()
    # the stored scores are the cosines of the stored codes
    c = z["codes"].astype(np.float64)
    u = c / np.maximum(np.linalg.norm(c, axis=1, keepdims=True), 1e-8)
    assert np.allclose((u[:, None, :] * u[ni]).sum(axis=2), ns, rtol=1e-3, atol=1e-5)
    # without the key: no line, no file, the log and the book of a config that never heard of it
    rc, out0, book0 = _run(tmp_path, "plain", dict(model))
    assert rc == 0, out0[-3000:]
    assert "OUTFIT CODES" not in out0 and not os.path.exists(_run_dir(tmp_path, "plain") / "codes.npz")
    assert _shape(out) == _shape(out0) and len(_shape(out0)) > 10            # (the codes line comes behind the end of training)
    assert {k: len(v) for k, v in book0.items()} == {k: len(v) for k, v in book.items()}
    assert all(np.isfinite(book0[k]).all() and np.isfinite(book[k]).all() for k in book0)
