"""End-to-end run of the embedding training script with swap noise (HIP: INPUT_NOISE: {KIND: swap}) on a real MI355X, on a small
synthetic file of the reference's input schema."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "mui-deepautoencoder_amd", "script")
SEED = 27493045


def test_embedding_script_trains_with_swap_noise_from_the_training_rows(tmp_path):
    import yaml
    from codae.tool.noise import input_noise_from_config
    rng = np.random.default_rng(1)
    cats = ["top", "bottom", "shoe"]
    S, E, n_obs = len(cats), 64, 360
    centers = rng.standard_normal((5, S * E)).astype(np.float32)
    emb = {}
    for i in range(n_obs):
        v = centers[i % 5] + 0.1 * rng.standard_normal(S * E).astype(np.float32)
        emb["o%04d" % i] = {c: v[s * E:(s + 1) * E].tolist() for s, c in enumerate(cats)}
    (tmp_path / "emb.json").write_text(json.dumps(emb))
    block = {"KIND": "swap", "P": 0.15, "SEED": 7, "POOL": "train"}
    cfg = {"MODEL": {"Z_SIZE": 64, "BATCH_SIZE": 64, "NB_INPUT_LAYER": 2, "NB_OUTPUT_LAYER": 2, "STEEP_LAYER_SIZE": False,
                     "EPOCH": 2, "LEARNING_RATE": 1e-3, "WEIGHT_DECAY": 1e-4, "NB_CORRUPTED": 1, "TRUNK_GRAD": True},
           "DATASET": {"NAME": "EMBEDDING", "USED_CATEGORY": cats, "EMBEDDING_SIZE": E, "SHUFFLE": True, "SPLIT": [0.7, 0.3]},
           "HIP": {"INPUT_NOISE": block},
           "SEED": SEED}
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    os.makedirs(tmp_path / "log")
    r = subprocess.run([sys.executable, os.path.join(SCRIPTS, "train_dae_on_embedding.py"), "--embedding_path", "emb.json", "--output_path",
                        "out", "--config", "cfg.yaml", "--precision", "bf16"], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    n_train = math.floor(n_obs * 0.7)
    assert "TRAINING HAS ENDED." in out
    assert "INPUT NOISE: swap, p = 0.15, pool of %d rows" % n_train in out
    runs = os.listdir(tmp_path / "out")
    book = json.load(open(tmp_path / "out" / runs[0] / "book.json"))
    assert len(book["ftl"]) == 2 and all(np.isfinite(book[k]).all() for k in book)          # the loss stays finite
    assert all(v > 0 for k in ("ftl", "ptl", "fvl", "pvl") for v in book[k])
    # the script's own split: with POOL: train no validation row is ever a source, at any step of the run
    indices = list(range(n_obs))
    np.random.seed(SEED)
    np.random.shuffle(indices)
    train, validation = indices[:n_train], set(indices[n_train:])
    noise = input_noise_from_config(block, train_rows=train)
    everywhere = input_noise_from_config(dict(block, POOL="all"), train_rows=train)
    swaps = leaks = 0
    for step in range(1, 2 * math.ceil(n_train / 64) + 1):
        acc, src = noise.swapped(train, step, S, n_rows=n_obs)
        assert not (set(src[acc].tolist()) & validation) and not (set(src.reshape(-1).tolist()) & validation)
        swaps += int(acc.sum())
        acc, src = everywhere.swapped(train, step, S, n_rows=n_obs)
        leaks += len(set(src[acc].tolist()) & validation)
    assert swaps > 0 and leaks > 0          # swaps happen, and without the pool validation rows would have been sources
