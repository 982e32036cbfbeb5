"""End-to-end run of the embedding training script on incomplete observations (HIP: KEEP_INCOMPLETE) on a real MI355X, with a
small synthetic file of the reference's input schema in which a third of the observations lack a category."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "mui-deepautoencoder_amd", "script")


def _run(cmd, cwd):
    r = subprocess.run([sys.executable] + cmd, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout + r.stderr


@pytest.mark.parametrize("precision,E,z", [("f32", 16, 48), ("bf16", 64, 64)])
def test_embedding_script_trains_on_incomplete_observations(tmp_path, precision, E, z):
    import yaml
    rng = np.random.default_rng(1)
    cats = ["top", "bottom", "shoe", "bag"]
    S = len(cats)
    centers = rng.standard_normal((5, S * E)).astype(np.float32)
    emb, kept, absent = {}, 0, 0
    for i in range(360):
        v = centers[i % 5] + 0.1 * rng.standard_normal(S * E).astype(np.float32)
        missing = [] if i % 3 == 0 else ([cats[i % S]] if i % 3 == 1 else [c for c in cats if c != cats[i % S]])     # 4, 3 or 1 of 4
        emb["o%04d" % i] = {c: v[s * E:(s + 1) * E].tolist() for s, c in enumerate(cats) if c not in missing}
        if S - len(missing) >= 2:
            kept += 1
            absent += len(missing)
    (tmp_path / "emb.json").write_text(json.dumps(emb))
    cfg = {"MODEL": {"Z_SIZE": z, "BATCH_SIZE": 64, "NB_INPUT_LAYER": 2, "NB_OUTPUT_LAYER": 2, "STEEP_LAYER_SIZE": False,
                     "EPOCH": 2, "LEARNING_RATE": 1e-3, "WEIGHT_DECAY": 1e-4, "NB_CORRUPTED": 1, "TRUNK_GRAD": True},
           "DATASET": {"NAME": "EMBEDDING", "USED_CATEGORY": cats, "EMBEDDING_SIZE": E, "SHUFFLE": True, "SPLIT": [0.7, 0.3]},
           "HIP": {"KEEP_INCOMPLETE": True, "MIN_PRESENT": 2},
           "SEED": 27493045}
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    os.makedirs(tmp_path / "log")
    out = _run([os.path.join(SCRIPTS, "train_dae_on_embedding.py"), "--embedding_path", "emb.json", "--output_path", "out",
                "--config", "cfg.yaml", "--precision", precision], cwd=str(tmp_path))
    assert "TRAINING HAS ENDED." in out and "VALIDATION RANKING ERROR" in out
    assert "Keeping incomplete observations: %d of %d slots are absent" % (absent, kept * S) in out and kept == 240 and absent == 120
    runs = os.listdir(tmp_path / "out")
    book = json.load(open(tmp_path / "out" / runs[0] / "book.json"))
    assert len(book["ftl"]) == 2 and all(np.isfinite(book[k]).all() for k in book)
    assert all(v > 0 for k in ("ftl", "ptl", "fvl", "pvl") for v in book[k])
    assert book["ftl"][-1] < book["ftl"][0], book["ftl"]            # it learns
    assert 0 <= book["rl"][-1] <= 1
