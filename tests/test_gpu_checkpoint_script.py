"""The embedding training script with HIP: CHECKPOINT and --resume on a real MI355X: a three-epoch run and its twin resumed from the
first epoch's file end in the same state digests and the same book.json; without the key nothing is written."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "mui-deepautoencoder_amd", "script")
BOOK_KEYS = {"ftl", "ptl", "fvl", "pvl", "rl"}


def _setup(tmp_path, checkpoint):
    import yaml
    rng = np.random.default_rng(1)
    cats = ["top", "bottom", "shoe"]
    S, E, n_obs = len(cats), 64, 360
    centers = rng.standard_normal((5, S * E)).astype(np.float32)
    emb = {}
    for i in range(n_obs):
        v = centers[i % 5] + 0.1 * rng.standard_normal(S * E).astype(np.float32)
        emb["o%04d" % i] = {c: v[s * E:(s + 1) * E].tolist() for s, c in enumerate(cats)}
    (tmp_path / "emb.json").write_text(json.dumps(emb))
    hip = {"INPUT_NOISE": {"KIND": "gaussian", "SIGMA": 0.05, "SEED": 3},
           "OPTIMIZER": {"KIND": "adamw", "SCHEDULE": {"KIND": "cosine", "WARMUP": 2, "MIN_FACTOR": 0.1}},
           "WEIGHT_AVERAGE": {"KIND": "ema", "DECAY": 0.9}}
    if checkpoint:
        hip["CHECKPOINT"] = {"EVERY": 1, "KEEP": 3}
    cfg = {"MODEL": {"Z_SIZE": 64, "BATCH_SIZE": 64, "NB_INPUT_LAYER": 2, "NB_OUTPUT_LAYER": 2, "STEEP_LAYER_SIZE": False,
                     "EPOCH": 3, "LEARNING_RATE": 1e-3, "WEIGHT_DECAY": 1e-4, "NB_CORRUPTED": 1, "TRUNK_GRAD": True},
           "DATASET": {"NAME": "EMBEDDING", "USED_CATEGORY": cats, "EMBEDDING_SIZE": E, "SHUFFLE": True, "SPLIT": [0.7, 0.3]},
           "HIP": hip, "SEED": 27493045}
    name = "cfg_ck.yaml" if checkpoint else "cfg_plain.yaml"
    (tmp_path / name).write_text(yaml.safe_dump(cfg))
    os.makedirs(tmp_path / "log", exist_ok=True)
    return name


def _run(tmp_path, cfg, out, *more):
    r = subprocess.run([sys.executable, os.path.join(SCRIPTS, "train_dae_on_embedding.py"), "--embedding_path", "emb.json", "--output_path",
                        out, "--config", cfg, "--precision", "bf16"] + list(more), cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    text = r.stdout + r.stderr
    assert r.returncode == 0, text[-3000:]
    assert "TRAINING HAS ENDED." in text
    (run,) = os.listdir(tmp_path / out)
    return tmp_path / out / run, text


def test_resumed_script_run_ends_in_the_digests_and_the_book_of_the_straight_run(tmp_path):
    from codae.tool.checkpoint import read_checkpoint
    cfg = _setup(tmp_path, True)
    a_dir, a_log = _run(tmp_path, cfg, "out_a")
    assert sorted(f for f in os.listdir(a_dir) if f.endswith(".npz")) == ["checkpoint_epoch%d.npz" % k for k in (1, 2, 3)]
    assert a_log.count("CHECKPOINT ") == 3 and not any(f.endswith(".tmp") for f in os.listdir(a_dir))
    b_dir, b_log = _run(tmp_path, cfg, "out_b", "--resume", str(a_dir / "checkpoint_epoch1.npz"))
    assert "RESUMED" in b_log and b_log.count("= EPOCH = ") == 2
    assert sorted(f for f in os.listdir(b_dir) if f.endswith(".npz")) == ["checkpoint_epoch2.npz", "checkpoint_epoch3.npz"]
    (ta, ma), (tb, mb) = read_checkpoint(str(a_dir / "checkpoint_epoch3.npz")), read_checkpoint(str(b_dir / "checkpoint_epoch3.npz"))
    assert ma["digests"] == mb["digests"] and ma["all"] == mb["all"] and ma["step_count"] == mb["step_count"] == 3 * 4
    assert set(ma["digests"]) == {"params", "adam_m", "adam_v", "weight_avg", "scalars"}
    assert all(np.array_equal(ta[n].view(np.uint8), tb[n].view(np.uint8)) for n in ta)
    assert ma["extra"]["epoch"] == 3 and ma["extra"]["rng"] == mb["extra"]["rng"] and ma["extra"]["mask_to_use"] == mb["extra"]["mask_to_use"]
    book_a, book_b = json.load(open(a_dir / "book.json")), json.load(open(b_dir / "book.json"))
    assert set(book_a) == set(book_b) == BOOK_KEYS
    for k in book_a:
        assert len(book_a[k]) == 3 and book_a[k] == book_b[k], k
    assert ma["extra"]["book"] == book_a

    # another dataset is refused, with both digests named
    emb = json.load(open(tmp_path / "emb.json"))
    emb["o0000"]["top"][0] += 1.0
    (tmp_path / "emb.json").write_text(json.dumps(emb))
    r = subprocess.run([sys.executable, os.path.join(SCRIPTS, "train_dae_on_embedding.py"), "--embedding_path", "emb.json", "--output_path",
                        "out_c", "--config", cfg, "--precision", "bf16", "--resume", str(a_dir / "checkpoint_epoch1.npz")],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and ma["extra"]["dataset_digest"] in r.stderr and "this run's dataset has" in r.stderr


def test_without_the_key_nothing_is_written_and_the_book_is_todays(tmp_path):
    cfg = _setup(tmp_path, False)
    d, log = _run(tmp_path, cfg, "out")
    assert not [f for f in os.listdir(d) if f.endswith(".npz")] and "CHECKPOINT" not in log and "RESUMED" not in log
    assert sorted(os.listdir(d)) == ["book.json", "full_RMSE.png", "partial_RMSE.png"]
    assert set(json.load(open(d / "book.json"))) == BOOK_KEYS
