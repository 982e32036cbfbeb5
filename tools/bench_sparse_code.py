#!/usr/bin/env python3
"""Cost of the sparse code at the headline shape (10 x Linear(1536, 1536) = 3 slots x 512, batch 8192, bf16): the whole fused
training step with the sparse code off and on (keep 64 of 1536 at the code layer), alternating inside every round in one process,
and the two new kernels on their own on an [8192][1536] matrix of both types beside the yardsticks of a streaming pass - the norm
forward and the dropout backward kernel on the same matrix - and beside torch.topk + scatter for the forward (device events
around `reps` back-to-back launches).

  python tools/bench_sparse_code.py [--steps K] [--warmup W] [--rounds N] [--reps R]      JSON lines, then one summary line per case

Bytes per launch are counted from the shapes (what the algorithm must move once, not what the caches served on the later passes):
  sparse_fwd        read and write act[m + 1], write the bits        2 B W e + B W / 8        (evaluation: no bits)
  sparse_bwd        read and write dA_m, read the bits               2 B W e + B W / 8
  norm_fwd          read and write act[l + 1], write r and the bits  2 B W e + 4 B + B W / 8
  dropout_bwd       read and write dA_l                              2 B W e
  topk + scatter    what the selection must move at least: 2 B W e
The forward kernel works in place, and a matrix it has sparsified is another input (W - keep equal keys per row): every timed
launch gets a fresh copy of the dense matrix; "sparse_fwd_again" times it on its own output.  The spread across rounds (min - max)
is the noise floor of every comparison.  DESIGN.md section 6 holds the numbers."""
import argparse
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
from codae.tool import SparseCode  # noqa: E402
from codae.train import HipEmbeddingTrainer  # noqa: E402

DEV = "cuda:0"
RESULTS = {}


def record(case, value, line):
    RESULTS.setdefault(case, []).append(value)
    print(json.dumps(line), flush=True)


def time_launches(fn, reps):
    """us per launch of `reps` back-to-back launches fn(i) between two device events (after two unrecorded ones, fn(reps), fn(reps + 1))"""
    fn(reps); fn(reps + 1)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(reps):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def kernels(B, W, keep, reps, rounds, bf16):
    lib = hip.lib()
    s = hip.current_stream()
    dt = torch.bfloat16 if bf16 else torch.float32
    e = 2 if bf16 else 4
    tag = "bf16" if bf16 else "f32"
    dense = torch.randn((B, W), device=DEV).to(dt)
    ys = [dense.clone() for _ in range(reps + 2)]              # the in-place forward kernels: a fresh dense matrix per launch
    d = torch.randn((B, W), device=DEV).to(dt)
    r = torch.ones((B,), device=DEV)
    bits = torch.zeros((B, W // 8), dtype=torch.uint8, device=DEV)
    parts = torch.zeros((lib.codae_sparse_code_blocks(B), W), device=DEV)
    again = dense.clone()
    hip.check(lib.codae_sparse_code_fwd(hip.ptr(again), int(bf16), W, B, W, keep, hip.ptr(bits), W // 8, s))

    def topk_scatter(i):
        idx = torch.topk(dense.abs(), keep, dim=1).indices
        return torch.zeros_like(dense).scatter_(1, idx, dense.gather(1, idx))

    cases = {
        "sparse_fwd": (lambda i: hip.check(lib.codae_sparse_code_fwd(hip.ptr(ys[i]), int(bf16), W, B, W, keep, hip.ptr(bits), W // 8, s)),
                       2 * B * W * e + B * W // 8),
        "sparse_fwd_eval": (lambda i: hip.check(lib.codae_sparse_code_fwd(hip.ptr(ys[i]), int(bf16), W, B, W, keep, None, 0, s)), 2 * B * W * e),
        "sparse_fwd_again": (lambda i: hip.check(lib.codae_sparse_code_fwd(hip.ptr(again), int(bf16), W, B, W, keep, None, 0, s)), 2 * B * W * e),
        "sparse_bwd": (lambda i: hip.check(lib.codae_sparse_code_bwd(hip.ptr(d), int(bf16), W, B, W, hip.ptr(bits), W // 8, hip.ptr(parts), s)),
                       2 * B * W * e + B * W // 8),
        "norm_fwd_layer": (lambda i: hip.check(lib.codae_norm_fwd(hip.ptr(ys[i]), int(bf16), W, B, W, 1, 1e-5, hip.ptr(r), hip.ptr(bits), W // 8, s)),
                           2 * B * W * e + 4 * B + B * W // 8),
        "dropout_bwd": (lambda i: hip.check(lib.codae_dropout_bwd(hip.ptr(d), int(bf16), W, B, W, None, 1, 1, 0.5, 7, hip.ptr(parts), s)),
                        2 * B * W * e),
        "torch_topk_scatter": (topk_scatter, 2 * B * W * e),
    }
    for rnd in range(rounds):
        for name, (fn, nbytes) in cases.items():
            for y in ys:
                y.copy_(dense)
            d.normal_()
            if name == "sparse_bwd":                            # (the mask of a forward over the dense matrix)
                hip.check(lib.codae_sparse_code_fwd(hip.ptr(ys[0]), int(bf16), W, B, W, keep, hip.ptr(bits), W // 8, s))
            us = time_launches(fn, reps)
            record("kernel %s %s" % (tag, name), us,
                   {"what": "kernel", "round": rnd, "type": tag, "kernel": name, "rows": B, "width": W, "keep": keep, "reps": reps,
                    "us": round(us, 2), "bytes": nbytes, "TB_per_s": round(nbytes / us * 1e-6, 3)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--io", type=int, default=1536)
    ap.add_argument("--keep", type=int, default=64)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
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
    settings = [("off", None), ("on", SparseCode(args.keep))]
    trainers = {}
    for name, sparse in settings:
        tr = HipEmbeddingTrainer(enc + dec, data, table, mtu, 1e-5, 1e-4, 1.0, max_batch=B, precision="bf16", device=DEV, sparse_code=sparse)
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
            res = tr.engine.sparse_resolved
            record("fused_step " + name, ms,
                   {"what": "fused_step", "round": rnd, "setting": name, "batch": B, "io": io, "layers": len(enc + dec),
                    "sparse": None if res is None else {"keep": args.keep, "of": res[1], "layer": res[0] + 1}, "ms_per_step": round(ms, 4),
                    "loss": tr.engine.read_scalars()[3], "path": tr.engine.step_path(B)})
    # the two launches per step from the engine's own profile, in a pass of its own (an event pair costs 2-4 us of stream time)
    n = 5
    tr = trainers["on"]
    tr.engine.profile_begin(classes=("dropout",), max_records=64 * n)
    for s in range(n):
        tr.train_batch(idx[s % 8], run=0)
    us = [1e3 * v for v in tr.engine.profile_end().get("dropout", [])]
    per = max(len(us) // n, 1)
    print(json.dumps({"what": "in_step_launches", "setting": "on", "per_step": len(us) // n,
                      "fwd_us_median": round(float(np.median(us[0::per])), 2) if us else None,
                      "bwd_us_median": round(float(np.median(us[1::per])), 2) if len(us) > 1 else None}), flush=True)
    del trainers
    for bf16 in (True, False):
        kernels(B, io, args.keep, args.reps, args.rounds, bf16)
    for case, vals in RESULTS.items():
        print("SUMMARY %-36s median %9.3f   min - max %9.3f - %9.3f   (%s, %d rounds)" % (
            case, float(np.median(vals)), min(vals), max(vals), "ms per step" if case.startswith("fused_step") else "us per launch", len(vals)))


if __name__ == "__main__":
    main()
