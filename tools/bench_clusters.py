#!/usr/bin/env python3
"""Cost of code clusters at the headline bank (65 536 codes x 1536, bf16-valued as the bf16 engine exports them) with K = 256 and
K = 4096: the fused nearest-centroid kernel in both forms against the torch route on the same device in the same precision -
(x @ c.T).argmax(1), bf16 operands for the bf16 form, which writes and re-reads the [M][K] scores the kernel never forms -, the
centroid update against index_add_ + normalise, and a whole CodeClusters.fit(iters=10).  Kernel and torch route alternate inside
every round in one process; min and max over the rounds are printed with every mean.

  python tools/bench_clusters.py [--rows N] [--width Z] [--ks 256,4096] [--rounds 5] [--reps N]      JSON lines

Shares of peak are counted from the shapes: the assignment's 2 M K Z flops over the time against 2.5 PF (bf16 MFMA, dense) or
157.3 TF (f32-input MFMA); the update's bytes - the bank once (4 M Z), norms and assignments, the centroids out - against 8 TB/s.
DESIGN.md section 6 "Code clusters" holds the numbers."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mui-deepautoencoder_amd")]

import torch  # noqa: E402

from codae import hip  # noqa: E402
from codae.tool import CodeClusters  # noqa: E402

DEV = "cuda:0"
PEAK_BF16, PEAK_F32, PEAK_HBM = 2.5e15, 157.3e12, 8.0e12


def time_launches(fn, reps):
    """us per call of `reps` back-to-back calls between two device events (after two unrecorded ones)"""
    fn(); fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def spread(v):
    return {"mean": round(sum(v) / len(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--width", type=int, default=1536)
    ap.add_argument("--ks", default="256,4096")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--fit-iters", type=int, default=10)
    args = ap.parse_args()
    M, Z = args.rows, args.width
    lib, s = hip.lib(), hip.current_stream()
    torch.manual_seed(1234)
    x = torch.randn((M, Z), device=DEV).bfloat16().float()                    # a bank as the bf16 engine exports it
    norm = torch.linalg.vector_norm(x, dim=1)
    x16 = x.bfloat16()
    assign = torch.empty(M, dtype=torch.long, device=DEV)
    best = torch.empty(M, device=DEV)
    for K in [int(k) for k in args.ks.split(",")]:
        c = torch.nn.functional.normalize(torch.randn((K, Z), device=DEV), dim=1)
        c16 = c.bfloat16()
        flops = 2.0 * M * K * Z
        ws = {b: torch.empty(int(lib.codae_nearest_centroid_ws_bytes(Z, K, b)), dtype=torch.uint8, device=DEV) for b in (0, 1)}

        def kernel(b):
            hip.check(lib.codae_nearest_centroid(hip.ptr(x), Z, M, Z, hip.ptr(c), Z, K, b, hip.ptr(norm), hip.ptr(assign), hip.ptr(best),
                                                 hip.ptr(ws[b]), s))
        routes = {"kernel_bf16": lambda: kernel(1), "torch_bf16": lambda: (x16 @ c16.t()).argmax(1),
                  "kernel_f32": lambda: kernel(0), "torch_f32": lambda: (x @ c.t()).argmax(1)}
        # the two routes agree wherever the scores are not a near-tie (reported, not asserted: different accumulation orders)
        kernel(0)
        agree = float((assign == (x @ c.t()).argmax(1)).float().mean())
        times = {name: [] for name in routes}
        for rnd in range(args.rounds):
            for name, fn in routes.items():
                times[name].append(time_launches(fn, args.reps if K <= 1024 or "bf16" in name else max(2, args.reps // 5)))
        for name, v in times.items():
            peak = PEAK_BF16 if "bf16" in name else PEAK_F32
            sp = spread(v)
            print(json.dumps({"what": "assign", "route": name, "M": M, "Z": Z, "K": K, "rounds": args.rounds, "us": sp,
                              "TFLOPs": round(flops / sp["mean"] * 1e-6, 1), "share_of_mfma_peak": round(flops / (sp["mean"] * 1e-6) / peak, 4),
                              "agree_with_torch_f32": round(agree, 6) if name == "kernel_f32" else None}), flush=True)
        # the update: members added in ascending row order against index_add_ (float atomics) + normalise
        kernel(0)
        a = assign.clone()
        out = torch.empty_like(c)
        counts = torch.empty(K, dtype=torch.long, device=DEV)
        wsu = torch.empty(int(lib.codae_centroid_update_ws_bytes(M, Z, K)), dtype=torch.uint8, device=DEV)

        def upd_kernel():
            hip.check(lib.codae_centroid_update(hip.ptr(x), Z, M, Z, hip.ptr(norm), hip.ptr(a), hip.ptr(c), hip.ptr(out), Z, K, hip.ptr(counts),
                                                hip.ptr(wsu), s))

        def upd_torch():
            sums = torch.zeros_like(c).index_add_(0, a, x / norm.clamp_min(1e-8)[:, None])
            return torch.nn.functional.normalize(sums, dim=1, eps=1e-8)
        nbytes = 4.0 * M * Z + 12.0 * M + 8.0 * K * Z
        times = {"kernel": [], "torch": []}
        for rnd in range(args.rounds):
            times["kernel"].append(time_launches(upd_kernel, args.reps))
            times["torch"].append(time_launches(upd_torch, args.reps))
        for name, v in times.items():
            sp = spread(v)
            print(json.dumps({"what": "update", "route": name, "M": M, "Z": Z, "K": K, "rounds": args.rounds, "us": sp, "bytes": nbytes,
                              "TB_per_s": round(nbytes / sp["mean"] * 1e-6, 3), "share_of_hbm_peak": round(nbytes / (sp["mean"] * 1e-6) / PEAK_HBM, 4)}),
                  flush=True)
        # a whole fit
        for precision in ("bf16", "f32"):
            if precision == "f32" and K > 1024:
                continue                                                      # (minutes of f32 MFMA: the assignment above is the figure)
            fit = lambda: CodeClusters.fit(x, K, norm=norm, iters=args.fit_iters, seed=0, precision=precision)      # noqa: E731
            v = [time_launches(fit, 1) * 1e-3 for _ in range(args.rounds)]
            print(json.dumps({"what": "fit", "precision": precision, "M": M, "Z": Z, "K": K, "iters": args.fit_iters, "rounds": args.rounds,
                              "ms": spread(v)}), flush=True)


if __name__ == "__main__":
    main()
