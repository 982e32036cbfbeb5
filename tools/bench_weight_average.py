#!/usr/bin/env python3
"""Cost of the weight average (include/codae_hip.h, "Weight average") on the fused training step: trainers of the same build that
differ in the setting only, alternating inside every round of one process, at BASELINE's C3 shape (10 x Linear(1536, 1536), 3 slots
of 512, batch 8192, bf16).

  python tools/bench_weight_average.py [--steps K] [--warmup W] [--rounds N]      JSON lines

Settings: off; ema (an EMA sampled every step, inside the update's launch); ema8 (every = 8); alone (averaging off in the engine,
codae_weight_average_update behind every step instead: the stand-alone kernel the fused form has to beat).  Per round and setting:
ms per fused step; then, in a pass of its own, the engine's event pairs around the update class; then one sync_average() (the bf16
image of the average, paid once per evaluation, not per step).  DESIGN.md section 6 holds the numbers."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mui-deepautoencoder_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from codae.tool import WeightAverage  # noqa: E402
from codae.train import HipEmbeddingTrainer  # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    io, L, B, S = 1536, 10, 8192, 3
    rng = np.random.default_rng(1234)
    n_rows = 2 * B
    data = torch.from_numpy(rng.random((n_rows, io), dtype=np.float32)).to(DEV)
    table = torch.ones((S, io), dtype=torch.uint8, device=DEV)
    for c in range(S):
        table[c, c * (io // S):(c + 1) * (io // S)] = 0
    mtu = torch.from_numpy(rng.integers(0, S, (n_rows, 1)).astype(np.int32)).to(DEV)
    idx = [torch.tensor(rng.permutation(n_rows)[:B], dtype=torch.int32, device=DEV) for _ in range(8)]
    sched = [(io, io, l + 1 < L and l != L // 2 - 1) for l in range(L)]
    settings = {"off": None, "ema": WeightAverage("ema", decay=0.999), "ema8": WeightAverage("ema", decay=0.999, every=8), "alone": None}
    alone_tool = WeightAverage("ema", decay=0.999)
    trainers = {}
    for name, tool in settings.items():
        tr = HipEmbeddingTrainer(sched, data, table, mtu, 1e-5, 1e-4, 1.0, max_batch=B, precision="bf16", device=DEV, n_slots=S,
                                 weight_average=tool)
        tr.init_params(seed=0)
        trainers[name] = tr
    alone_avg = trainers["alone"].engine.params.clone()

    def step(name, tr, s):
        tr.train_batch(idx[s % 8], run=0)
        if name == "alone":
            alone_tool.update(alone_avg, tr.engine._params, tr.engine.step_count)

    for name, tr in trainers.items():
        for s in range(args.warmup):
            step(name, tr, s)
    torch.cuda.synchronize()
    for rnd in range(args.rounds):
        for name, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(args.steps):
                step(name, tr, s)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            print(json.dumps({"what": "fused_step", "round": rnd, "setting": name, "batch": B, "io": io, "layers": L,
                              "ms_per_step": round(ms, 4), "loss": tr.engine.read_scalars()[3], "path": tr.engine.step_path(B)}), flush=True)
    for rnd in range(args.rounds):
        for name, tr in trainers.items():
            if name == "alone":
                continue
            tr.engine.profile_begin(classes=("adam",), max_records=4 * args.steps)
            for s in range(args.steps):
                step(name, tr, s)
            us = [1e3 * v for v in tr.engine.profile_end().get("adam", [])]
            print(json.dumps({"what": "update_launch", "round": rnd, "setting": name, "adam_us_per_step": round(float(np.sum(us)) / args.steps, 2),
                              "records_per_step": len(us) / args.steps}), flush=True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        alone_tool.update(alone_avg, trainers["alone"].engine._params, 5)
    e0.record()
    for _ in range(args.steps):
        alone_tool.update(alone_avg, trainers["alone"].engine._params, 5)
    e1.record()
    torch.cuda.synchronize()
    print(json.dumps({"what": "kernel", "kernel": "weight_average_update", "elements": int(alone_avg.numel()),
                      "us": round(1e3 * e0.elapsed_time(e1) / args.steps, 2)}), flush=True)
    eng = trainers["ema"].engine
    for rnd in range(args.rounds):
        eng._avg_stale = True
        e0.record()
        eng.sync_average()
        e1.record()
        torch.cuda.synchronize()
        print(json.dumps({"what": "sync_average", "round": rnd, "us": round(1e3 * e0.elapsed_time(e1), 2)}), flush=True)


if __name__ == "__main__":
    main()
