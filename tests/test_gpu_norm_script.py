"""End-to-end runs of the embedding training script with and without HIP: NORM on a real MI355X, on a small synthetic file of the
reference's input schema: the key trains through the norm and logs one line; without it, or with no layer chosen, the run logs and
books what a config that never heard of the key logs and books."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "mui-deepautoencoder_amd", "script")
SEED = 27493045


def _run(tmp_path, name, hip_block):
    import yaml
    cats = ["top", "bottom", "shoe"]
    cfg = {"MODEL": {"Z_SIZE": 64, "BATCH_SIZE": 64, "NB_INPUT_LAYER": 2, "NB_OUTPUT_LAYER": 2, "STEEP_LAYER_SIZE": False,
                     "EPOCH": 2, "LEARNING_RATE": 1e-3, "WEIGHT_DECAY": 1e-4, "NB_CORRUPTED": 1, "TRUNK_GRAD": True},
           "DATASET": {"NAME": "EMBEDDING", "USED_CATEGORY": cats, "EMBEDDING_SIZE": 64, "SHUFFLE": True, "SPLIT": [0.7, 0.3]},
           "SEED": SEED}
    if hip_block is not None:
        cfg["HIP"] = hip_block
    (tmp_path / (name + ".yaml")).write_text(yaml.safe_dump(cfg))
    r = subprocess.run([sys.executable, os.path.join(SCRIPTS, "train_dae_on_embedding.py"), "--embedding_path", "emb.json", "--output_path",
                        "out_" + name, "--config", name + ".yaml", "--precision", "bf16"], cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=600)
    out = r.stdout + r.stderr
    runs = os.listdir(tmp_path / ("out_" + name)) if r.returncode == 0 else []
    book = json.load(open(tmp_path / ("out_" + name) / runs[0] / "book.json")) if runs else None
    return r.returncode, out, book


def _shape(out):
    """the log's INFO lines from the description of the stack to the end of training, without their time stamps, every run of digits and the run's output directory masked"""
    import re
    lines = [re.sub(r"[0-9]+", "#", re.sub(r"out_[a-z]+", "out", ln.split(" - INFO - ", 1)[1])) for ln in out.splitlines() if " - INFO - " in ln]
    start = [i for i, ln in enumerate(lines) if ln.startswith("Linear stack:")]
    end = [i for i, ln in enumerate(lines) if ln.startswith("TRAINING HAS ENDED.")]
    assert len(start) == 1 and len(end) == 1
    # (in front of it the script prints the config it was given; behind it the plotting library may log that it built its font cache)
    return lines[start[0]:end[0] + 1]


def test_embedding_script_trains_through_the_norm_and_is_unchanged_without_the_key(tmp_path):
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
    rc, out, book = _run(tmp_path, "norm", {"NORM": {"KIND": "layer", "LAYERS": "hidden", "EPS": 1e-5}})
    assert rc == 0, out[-3000:]
    assert "TRAINING HAS ENDED." in out
    lines = [ln for ln in out.splitlines() if "NORM: Norm('layer', layers='hidden', eps=1e-05)" in ln]
    assert len(lines) == 1 and "layers [0, 1, 2, 3, 4]" in lines[0], lines            # one log line: every layer of the six but the last
    assert len(book["ftl"]) == 2 and all(np.isfinite(book[k]).all() for k in book)
    assert all(v > 0 for k in ("ftl", "ptl", "fvl", "pvl") for v in book[k])
    # without the key, and with the key but no layer: no norm line, and the same log and book as each other
    rc, out0, book0 = _run(tmp_path, "plain", None)
    assert rc == 0, out0[-3000:]
    rc, out1, book1 = _run(tmp_path, "empty", {"NORM": {"KIND": "rms", "LAYERS": []}})
    assert rc == 0, out1[-3000:]
    assert "NORM:" not in out0 and "NORM:" not in out1
    # (the script draws its initial weights from an unseeded generator, so no two runs share their numbers; what can be compared is
    #  the log line by line with the digits masked and the shape of the book - the bits are test_gpu_norm.py::test_off_is_off_192_b40's)
    assert _shape(out0) == _shape(out1) and len(_shape(out0)) > 10
    assert [ln for ln in _shape(out) if not ln.startswith("NORM:")] == _shape(out0)   # the norm line is all the key adds to the log
    assert {k: len(v) for k, v in book0.items()} == {k: len(v) for k, v in book1.items()} == {k: len(v) for k, v in book.items()}
    assert all(np.isfinite(book0[k]).all() and np.isfinite(book1[k]).all() for k in book0)
