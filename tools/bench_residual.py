#!/usr/bin/env python3
"""Cost of residual connections at the headline shape (10 x Linear(1536, 1536), batch 8192, bf16): the whole fused training step
with skips off and with Residual("hidden") (layers 1 .. 8), alternating inside every round in one process, and the two new kernels
on their own beside the dropout kernels on the same [8192][1536] bf16 matrix (device events around `reps` back-to-back launches
of the stand-alone launchers).

  python tools/bench_residual.py [--steps K] [--warmup W] [--rounds N]      JSON lines

Bytes per launch are counted from the shapes (what the algorithm must move, not what the caches saved):
  residual_fwd   read act[l + 1] and act[l], write act[l + 1], write the bits                   3 B W e + B W / 8
  residual_bwd   read U, write D (working precision), read + write G (fp32), read the bits      2 B W e + 8 B W + B W / 8
  dropout_fwd / dropout_bwd   read + write one matrix                                           2 B W e
The spread across rounds is the noise floor of every comparison.  DESIGN.md section 6 holds the numbers."""
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
from codae.tool import Residual  # noqa: E402
from codae.train import HipEmbeddingTrainer  # noqa: E402

DEV = "cuda:0"


def time_launches(fn, reps):
    """us per launch of `reps` back-to-back launches between two device events (after two unrecorded ones)"""
    fn(); fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def kernels(B, W, reps, rounds):
    lib = hip.lib()
    s = hip.current_stream()
    y = torch.randn((B, W), device=DEV).to(torch.bfloat16)
    x = torch.randn((B, W), device=DEV).to(torch.bfloat16)
    g = torch.randn((B, W), device=DEV)
    bits = torch.zeros((B, W // 8), dtype=torch.uint8, device=DEV)
    parts = torch.zeros((lib.codae_residual_blocks(B), W), device=DEV)
    p = (C.c_float * 3)(0.0, 0.0, 0.0)
    e = 2
    cases = {
        "residual_fwd": (lambda: hip.check(lib.codae_residual_fwd(hip.ptr(y), hip.ptr(x), 1, W, W, B, W, hip.ptr(bits), W // 8, s)),
                         3 * B * W * e + B * W // 8),
        "residual_fwd_eval": (lambda: hip.check(lib.codae_residual_fwd(hip.ptr(y), hip.ptr(x), 1, W, W, B, W, None, 0, s)), 3 * B * W * e),
        "residual_bwd": (lambda: hip.check(lib.codae_residual_bwd(hip.ptr(y), 1, W, B, W, hip.ptr(g), hip.ptr(g), W, hip.ptr(bits), W // 8, None, 0,
                                                                  1, p, hip.ptr(parts), s)), 2 * B * W * e + 8 * B * W + B * W // 8),
        "dropout_fwd": (lambda: hip.check(lib.codae_dropout_fwd(hip.ptr(y), 1, W, B, W, None, 1, 1, 0.5, 7, s)), 2 * B * W * e),
        "dropout_bwd": (lambda: hip.check(lib.codae_dropout_bwd(hip.ptr(y), 1, W, B, W, None, 1, 1, 0.5, 7, hip.ptr(parts), s)), 2 * B * W * e),
    }
    for rnd in range(rounds):
        for name, (fn, nbytes) in cases.items():
            y.normal_(); g.normal_()                                # (the in-place kernels would otherwise drive the values to inf / 0)
            us = time_launches(fn, reps)
            print(json.dumps({"what": "kernel", "round": rnd, "kernel": name, "rows": B, "width": W, "reps": reps, "us": round(us, 2),
                              "bytes": nbytes, "GB_per_s": round(nbytes / us * 1e-3, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--io", type=int, default=1536)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
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
    settings = [("off", None), ("hidden", Residual("hidden"))]
    trainers = {}
    for name, res in settings:
        tr = HipEmbeddingTrainer(enc + dec, data, table, mtu, 1e-5, 1e-4, 1.0, max_batch=B, precision="bf16", device=DEV, residual=res)
        tr.init_params(seed=0)
        for s in range(args.warmup):
            tr.train_batch(idx[s % 8], run=0)
        trainers[name] = tr
    torch.cuda.synchronize()
    for rnd in range(args.rounds):
        for name, _ in settings:
            tr = trainers[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(args.steps):
                tr.train_batch(idx[s % 8], run=0)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            print(json.dumps({"what": "fused_step", "round": rnd, "setting": name, "batch": B, "io": io, "layers": len(enc + dec),
                              "skipped": tr.engine.residual_layers, "ms_per_step": round(ms, 4), "loss": tr.engine.read_scalars()[3],
                              "path": tr.engine.step_path(B)}), flush=True)
    # the streaming class of the step with skips on, in a pass of its own (an event pair costs 2-4 us of stream time): per step 8
    # forward launches, then 9 backward ones (behind the data gradients of layers 9 .. 1)
    tr = trainers["hidden"]
    n = 5
    tr.engine.profile_begin(classes=("dropout",), max_records=64 * n)
    for s in range(n):
        tr.train_batch(idx[s % 8], run=0)
    us = [1e3 * v for v in tr.engine.profile_end().get("dropout", [])]
    per = len(us) // n
    fwd = [v for i, v in enumerate(us) if i % per < len(tr.engine.residual_layers)]
    bwd = [v for i, v in enumerate(us) if i % per >= len(tr.engine.residual_layers)]
    print(json.dumps({"what": "in_step_launches", "per_step": per, "fwd_us_median": round(float(np.median(fwd)), 2),
                      "bwd_us_median": round(float(np.median(bwd)), 2)}), flush=True)
    kernels(B, io, args.reps, args.rounds)


if __name__ == "__main__":
    main()
