#!/usr/bin/env python3
"""Cost of the input noise at the headline shape (batch 8192, io 1536, bf16): the gather + corruption launch alone
(codae_corrupt_batch: noise off, MASKING, SALT_PEPPER, GAUSSIAN) and the whole fused training step per kind.

  python tools/bench_noise.py [--reps R] [--steps K] [--warmup W] [--rounds N]      JSON lines
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_noise.py --launch-only    per-kernel times, a run of its own

The kinds alternate inside every round (off, masking, salt_pepper, gaussian, off, ...), so that a drift of the machine lands
on all of them; every round prints its own line and the spread across rounds is the noise floor of the comparison.
CODAE_HIP_LIB / another checkout give the same `off` launch of another build.  DESIGN.md section 6 holds the numbers."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mui-deepautoencoder_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from codae import hip  # noqa: E402
from codae.model.schedule import linear_stack  # noqa: E402
from codae.tool import InputNoise  # noqa: E402
from codae.train import HipEmbeddingTrainer  # noqa: E402

DEV = "cuda:0"


def kinds():
    return [("off", None), ("masking", InputNoise("masking", p=0.25, seed=1)),
            ("salt_pepper", InputNoise("salt_pepper", p=0.1, lo=0.0, hi=1.0, seed=1)),
            ("gaussian", InputNoise("gaussian", sigma=0.1, seed=1))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--io", type=int, default=1536)
    ap.add_argument("--reps", type=int, default=200, help="launches per timed window")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launch-only", action="store_true")
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
    out = torch.zeros((B, io), dtype=torch.bfloat16, device=DEV)
    lib = hip.lib()
    stream = hip.current_stream()
    batches = [hip.Batch(hip.ptr(data), hip.ptr(i), None, hip.ptr(table), B, io, hip.ptr(mtu), 1, 0) for i in idx]
    moved = 4 * B * io + 2 * B * io                  # fp32 rows read, bf16 rows written (mask table and ids: < 1 %)

    def launch(noise_struct, r):
        hip.check(lib.codae_corrupt_batch(C.byref(batches[r % 8]), None if noise_struct is None else C.byref(noise_struct), 1 + r,
                                          None, hip.ptr(out), 1, io, stream))

    for rnd in range(args.rounds):
        for name, noise in kinds():
            st = None if noise is None else noise.as_struct()
            for r in range(20):
                launch(st, r)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for r in range(args.reps):
                launch(st, r)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / args.reps
            print(json.dumps({"what": "gather_launch", "round": rnd, "noise": name, "batch": B, "io": io, "us_per_launch": round(us, 3),
                              "TB_per_s": round(moved / us * 1e-6, 3)}), flush=True)
    if args.launch_only:
        return
    enc, dec = linear_stack(io, io, 4, 4, False, False)
    trainers = {}
    for name, noise in kinds():
        tr = HipEmbeddingTrainer(enc + dec, data, table, mtu, 1e-5, 1e-4, 1.0, max_batch=B, precision="bf16", device=DEV,
                                 input_noise=noise)
        tr.init_params(seed=0)
        for s in range(args.warmup):
            tr.train_batch(idx[s % 8], run=0)
        trainers[name] = tr
    torch.cuda.synchronize()
    for rnd in range(args.rounds):
        for name, _ in kinds():
            tr = trainers[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(args.steps):
                tr.train_batch(idx[s % 8], run=0)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            print(json.dumps({"what": "fused_step", "round": rnd, "noise": name, "batch": B, "io": io, "ms_per_step": round(ms, 4),
                              "loss": tr.engine.read_scalars()[3], "path": tr.engine.step_path(B)}), flush=True)


if __name__ == "__main__":
    main()
