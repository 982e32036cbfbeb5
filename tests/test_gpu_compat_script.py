"""End-to-end run of the embedding training script with and without HIP: COMPATIBILITY on a real MI355X, on the synthetic file the other
script tests use: with the key three more log lines and three more book.json keys, one value per epoch; without it exactly the lines
and keys the script always had."""
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "mui-deepautoencoder_amd", "script")
LINES = ("VALIDATION COMPATIBILITY AUC", "VALIDATION PAIRED ACCURACY", "VALIDATION SCORED OUTFITS")
KEYS = ("auc", "paired_acc", "scored_outfits")


def _run(cmd, cwd):
    r = subprocess.run([sys.executable] + cmd, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _labels(out):
    """the metric lines of the log, in order: 'TRAINING FULL ERROR', 'VALIDATION RANKING ERROR', ..."""
    return re.findall(r"((?:TRAINING|VALIDATION) [A-Z@0-9 ]+?)\s*=", out)


def test_embedding_script_logs_compatibility_only_with_the_key(tmp_path):
    import yaml
    rng = np.random.default_rng(1)
    cats, E, epochs = ["top", "bottom", "shoe"], 64, 2
    centers = rng.standard_normal((5, 3 * E)).astype(np.float32)
    emb = {}
    for i in range(360):
        v = centers[i % 5] + 0.1 * rng.standard_normal(3 * E).astype(np.float32)
        emb["o%04d" % i] = {c: v[s * E:(s + 1) * E].tolist() for s, c in enumerate(cats)}
    (tmp_path / "emb.json").write_text(json.dumps(emb))
    os.makedirs(tmp_path / "log")
    books, logs = {}, {}
    for name, hip_block in (("plain", None), ("compat", {"COMPATIBILITY": {"NEGATIVES": 2, "SEED": 3, "DISTINCT": True}})):
        cfg = {"MODEL": {"Z_SIZE": 64, "BATCH_SIZE": 64, "NB_INPUT_LAYER": 2, "NB_OUTPUT_LAYER": 2, "STEEP_LAYER_SIZE": False,
                         "EPOCH": epochs, "LEARNING_RATE": 1e-3, "WEIGHT_DECAY": 1e-4, "NB_CORRUPTED": 1, "TRUNK_GRAD": True},
               "DATASET": {"NAME": "EMBEDDING", "USED_CATEGORY": cats, "EMBEDDING_SIZE": E, "SHUFFLE": True, "SPLIT": [0.7, 0.3]},
               "SEED": 27493045}
        if hip_block is not None:
            cfg["HIP"] = hip_block
        (tmp_path / (name + ".yaml")).write_text(yaml.safe_dump(cfg))
        logs[name] = _run([os.path.join(SCRIPTS, "train_dae_on_embedding.py"), "--embedding_path", "emb.json", "--output_path", "out_" + name,
                           "--config", name + ".yaml", "--precision", "bf16"], cwd=str(tmp_path))
        runs = os.listdir(tmp_path / ("out_" + name))
        books[name] = json.load(open(tmp_path / ("out_" + name) / runs[0] / "book.json"))
    # without the key: the parent's log lines and book keys, nothing else
    per_epoch = ["TRAINING FULL ERROR", "TRAINING PARTIAL ERROR", "VALIDATION FULL ERROR", "VALIDATION PARTIAL ERROR", "VALIDATION RANKING ERROR"]
    assert _labels(logs["plain"]) == per_epoch * epochs
    assert sorted(books["plain"]) == sorted(["ftl", "ptl", "fvl", "pvl", "rl"])
    assert not any(l in logs["plain"] for l in LINES)
    # with it: the three lines behind the validation lines of every epoch, the three keys with one value per epoch
    assert _labels(logs["compat"]) == (per_epoch + list(LINES)) * epochs
    assert sorted(books["compat"]) == sorted(["ftl", "ptl", "fvl", "pvl", "rl"] + list(KEYS))
    b = books["compat"]
    assert all(len(b[k]) == epochs for k in KEYS)
    nb_validation = 360 - math.floor(360 * 0.7)                            # the script's split; every row is complete
    assert b["scored_outfits"] == [float(nb_validation)] * epochs
    assert all(0.0 <= v <= 1.0 for k in ("auc", "paired_acc") for v in b[k])
