#!/usr/bin/env python3
"""Cost of tied weights (include/codae_hip.h, "Tied weights") on the fused training step: a tied and an untied trainer of the same
build, alternating inside every round of one process, at BASELINE's C3 shape (10 x Linear(1536, 1536), 3 slots of 512, batch 8192,
bf16) or its C2 shape (10 x Linear(384, 384), 3 slots of 128, batch 1024: the persistent chain kernel).

  python tools/bench_tied.py --shape c3|c2 [--steps K] [--warmup W] [--rounds N]      JSON lines

Per round and setting: ms per fused step; then, in passes of their own, the engine's event pairs around the norm class (untied:
nothing or the flat pass; tied: the fold and the flat pass) and the update class (tied: the update of the free parameters and the
mirror), and the fold and the mirror kernels alone on the tied engine's buffers.  Run one shape per process, each under a time
limit of its own.  DESIGN.md section 6 holds the numbers."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mui-deepautoencoder_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from codae.hip.engine import tie_fold, tie_mirror  # noqa: E402
from codae.train import HipEmbeddingTrainer  # noqa: E402

DEV = "cuda:0"
SHAPES = {"c3": (1536, 10, 8192), "c2": (384, 10, 1024)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="c3")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    io, L, B = SHAPES[args.shape]
    S = 3
    rng = np.random.default_rng(1234)
    n_rows = 2 * B
    data = torch.from_numpy(rng.random((n_rows, io), dtype=np.float32)).to(DEV)
    table = torch.ones((S, io), dtype=torch.uint8, device=DEV)
    for c in range(S):
        table[c, c * (io // S):(c + 1) * (io // S)] = 0
    mtu = torch.from_numpy(rng.integers(0, S, (n_rows, 1)).astype(np.int32)).to(DEV)
    idx = [torch.tensor(rng.permutation(n_rows)[:B], dtype=torch.int32, device=DEV) for _ in range(8)]
    sched = [(io, io, l + 1 < L and l != L // 2 - 1) for l in range(L)]
    trainers = {}
    for name, tied in (("untied", False), ("tied", True)):
        tr = HipEmbeddingTrainer(sched, data, table, mtu, 1e-5, 1e-4, 1.0, max_batch=B, precision="bf16", device=DEV, n_slots=S,
                                 tied_weights=tied)
        tr.init_params(seed=0)
        for s in range(args.warmup):
            tr.train_batch(idx[s % 8], run=0)
        trainers[name] = tr
    torch.cuda.synchronize()
    for rnd in range(args.rounds):
        for name, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(args.steps):
                tr.train_batch(idx[s % 8], run=0)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            print(json.dumps({"what": "fused_step", "shape": args.shape, "round": rnd, "setting": name, "batch": B, "io": io, "layers": L,
                              "ms_per_step": round(ms, 4), "loss": tr.engine.read_scalars()[3], "path": tr.engine.step_path(B)}), flush=True)
    for rnd in range(args.rounds):
        for name, tr in trainers.items():
            tr.engine.profile_begin(classes=("sumsq", "adam"), max_records=8 * args.steps)
            for s in range(args.steps):
                tr.train_batch(idx[s % 8], run=0)
            rec = tr.engine.profile_end()
            out = {"what": "launches", "shape": args.shape, "round": rnd, "setting": name}
            for k in ("sumsq", "adam"):
                us = [1e3 * v for v in rec.get(k, [])]
                out[k + "_us_per_step"] = round(float(np.sum(us)) / args.steps, 2) if us else 0.0
                out[k + "_records_per_step"] = len(us) / args.steps
            print(json.dumps(out), flush=True)
    eng = trainers["tied"].engine
    pairs = eng.tie_pairs()
    for what, fn in (("fold", lambda: tie_fold(eng.grads, pairs)), ("mirror", lambda: tie_mirror(eng._params, pairs, eng.shadow, eng.shadow_t)),
                     ("mirror_fp32_only", lambda: tie_mirror(eng._params, pairs))):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        n = sum(r * c for _, _, r, c in pairs)
        print(json.dumps({"what": "kernel", "shape": args.shape, "kernel": what, "pairs": len(pairs), "elements": n,
                          "us": round(1e3 * e0.elapsed_time(e1) / args.steps, 2)}), flush=True)


if __name__ == "__main__":
    main()
