#!/usr/bin/env python3
"""Cost of the layer-wise trust ratios at the headline shape (10 x Linear(1536, 1536) = 3 slots x 512, batch 8192, bf16): the whole
fused training step under adam (the default instantiation: the anchor every other log of this box can be laid beside), adamw, lamb
and lars, alternating inside every round in one process, and the update's own launches from the engine's profile (class "adam":
the tiled update alone under adamw; the norms pass, the finish and the tiled update under lamb / lars).

  python tools/bench_trust.py [--steps K] [--warmup W] [--rounds N]      JSON lines, then one summary line per case

Bytes per parameter, counted from what each pass must move once: the Adam update reads p, g, m, v and writes p, m, v and the two
bf16 shadows: 32 B; the norms pass reads p, g, m, v (lamb: 16 B) or p, g (lars: 8 B); the lars update moves no v: 24 B.  The spread
across rounds (min - max) is the noise floor of every comparison.  DESIGN.md section 6 holds the numbers."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mui-deepautoencoder_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from codae.model.schedule import linear_stack  # noqa: E402
from codae.tool import Optimizer  # noqa: E402
from codae.train import HipEmbeddingTrainer  # noqa: E402

DEV = "cuda:0"
RESULTS = {}


def record(case, value, line):
    RESULTS.setdefault(case, []).append(value)
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--io", type=int, default=1536)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    B, io = args.batch, args.io
    rng = np.random.default_rng(1234)
    data = torch.from_numpy(rng.random((4 * B, io), dtype=np.float32)).to(DEV)
    S = 3
    table = torch.ones((S, io), dtype=torch.uint8, device=DEV)
    for c in range(S):
        table[c, c * (io // S):(c + 1) * (io // S)] = 0
    mtu = torch.from_numpy(rng.integers(0, S, (4 * B, 1)).astype(np.int32)).to(DEV)
    idx = [torch.tensor(rng.permutation(4 * B)[:B], dtype=torch.int32, device=DEV) for _ in range(8)]
    enc, dec = linear_stack(io, io, 4, 4, False, False)
    settings = [("adam", None), ("adamw", Optimizer("adamw")), ("lamb", Optimizer("lamb")), ("lars", Optimizer("lars", momentum=0.9))]
    trainers = {}
    for name, opt in settings:
        tr = HipEmbeddingTrainer(enc + dec, data, table, mtu, 1e-5, 1e-4, 1.0, max_batch=B, precision="bf16", device=DEV, optimizer=opt)
        tr.init_params(seed=0)
        for s in range(args.warmup):
            tr.train_batch(idx[s % 8], run=0)
        trainers[name] = tr
    torch.cuda.synchronize()
    n_param = trainers["adam"].engine.n_param
    for rnd in range(args.rounds):
        for name, _ in settings:
            tr = trainers[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(args.steps):
                tr.train_batch(idx[s % 8], run=0)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            record("fused_step " + name, ms,
                   {"what": "fused_step", "round": rnd, "optimizer": name, "batch": B, "io": io, "layers": len(enc + dec), "n_param": n_param,
                    "ms_per_step": round(ms, 4), "loss": tr.engine.read_scalars()[3], "path": tr.engine.step_path(B),
                    "ratios_min_max": [float(x) for x in torch.aminmax(tr.trust_ratios())] if name in ("lamb", "lars") else None})
    # the update's launches per step from the engine's own profile, in a pass of its own (an event pair costs 2-4 us of stream time)
    n = 5
    for name, _ in settings:
        tr = trainers[name]
        for rnd in range(args.rounds):
            tr.engine.profile_begin(classes=("adam",), max_records=64 * n)
            for s in range(n):
                tr.train_batch(idx[s % 8], run=0)
            us = [1e3 * v for v in tr.engine.profile_end().get("adam", [])]
            per_step = sum(us) / n
            record("update_launches " + name, per_step,
                   {"what": "update_launches", "round": rnd, "optimizer": name, "scopes_per_step": len(us) // n, "us_per_step": round(per_step, 2),
                    "TB_per_s_at_32B_per_param": round(32.0 * n_param / per_step * 1e-6, 3)})
    for case, vals in RESULTS.items():
        print("SUMMARY %-28s median %9.3f   min - max %9.3f - %9.3f   (%s, %d rounds)" % (
            case, float(np.median(vals)), min(vals), max(vals), "ms per step" if case.startswith("fused_step") else "us per step", len(vals)))


if __name__ == "__main__":
    main()
