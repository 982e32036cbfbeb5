#!/usr/bin/env python3
"""Cost of outfit codes at the headline shape (10 x Linear(1536, 1536) = 3 slots x 512, 65 536 resident rows, max_batch 8192, bf16,
Norm("layer") and Residual("hidden") on): the export kernel on its own beside the norm forward kernel on the same [8192][1536]
matrix, code_index() over every row against one evaluation sweep (eval_batch) of the same rows, alternating inside every round in
one process, similar() for 8192 queries with k = 10, and what the training script adds after its last epoch (code_index, the copy
to the host, codes.npz).

  python tools/bench_codes.py [--rows N] [--rounds N] [--reps N]      JSON lines

Bytes per launch are counted from the shapes: export reads B W e and writes 4 B W + 4 B; norm_fwd (evaluation form) as
tools/bench_norm.py counts it.  code_index runs code_layers = 5 of the 10 Linears, one assemble and one export per chunk; the sweep
runs 10 Linears, one gather and one loss kernel per chunk.  The spread across rounds is the noise floor of every comparison.
DESIGN.md section 6 holds the numbers."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mui-deepautoencoder_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from codae import hip  # noqa: E402
from codae.model.schedule import linear_stack  # noqa: E402
from codae.tool import Norm, Residual  # noqa: E402
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


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def kernels(B, W, reps, rounds):
    lib = hip.lib()
    s = hip.current_stream()
    src32 = torch.randn((B, W), device=DEV)
    src16 = src32.to(torch.bfloat16)
    dst = torch.empty((B, W), device=DEV)
    norm = torch.empty((B,), device=DEV)
    y = torch.randn((B, W), device=DEV).to(torch.bfloat16)
    r = torch.ones((B,), device=DEV)
    cases = {
        "export_bf16": (lambda: hip.check(lib.codae_export_rows(hip.ptr(src16), 1, W, B, W, hip.ptr(dst), W, hip.ptr(norm), s)), B * W * 2 + 4 * B * W + 4 * B),
        "export_f32": (lambda: hip.check(lib.codae_export_rows(hip.ptr(src32), 0, W, B, W, hip.ptr(dst), W, hip.ptr(norm), s)), B * W * 4 + 4 * B * W + 4 * B),
        "norm_fwd_eval_layer_bf16": (lambda: hip.check(lib.codae_norm_fwd(hip.ptr(y), 1, W, B, W, 1, 1e-5, hip.ptr(r), None, 0, s)), 2 * B * W * 2 + 4 * B),
    }
    for rnd in range(rounds):
        for name, (fn, nbytes) in cases.items():
            y.normal_()
            us = time_launches(fn, reps)
            print(json.dumps({"what": "kernel", "round": rnd, "kernel": name, "rows": B, "width": W, "reps": reps, "us": round(us, 2),
                              "bytes": nbytes, "TB_per_s": round(nbytes / us * 1e-6, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--io", type=int, default=1536)
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--k", type=int, default=10)
    args = ap.parse_args()
    B, io, N = args.batch, args.io, args.rows
    kernels(B, io, args.reps, args.rounds)
    rng = np.random.default_rng(1234)
    data = torch.from_numpy(rng.random((N, io), dtype=np.float32)).to(DEV)
    S = 3
    table = torch.ones((S, io), dtype=torch.uint8, device=DEV)
    for c in range(S):
        table[c, c * (io // S):(c + 1) * (io // S)] = 0
    mtu = torch.from_numpy(rng.integers(0, S, (N, 1)).astype(np.int32)).to(DEV)
    enc, dec = linear_stack(io, io, 4, 4, False, False)
    tr = HipEmbeddingTrainer(enc + dec, data, table, mtu, 1e-5, 1e-4, 1.0, max_batch=B, precision="bf16", device=DEV,
                             residual=Residual("hidden"), norm=Norm("layer"))
    tr.init_params(seed=0)
    chunks = [torch.arange(o, min(o + B, N), dtype=torch.int32, device=DEV) for o in range(0, N, B)]

    def sweep():
        for idx in chunks:
            tr.eval_batch(idx, run=0)

    sweep(); tr.code_index()                     # warm both
    index = None
    for rnd in range(args.rounds):
        ms_sweep, _ = wall_ms(sweep)
        ms_index, index = wall_ms(tr.code_index)
        print(json.dumps({"what": "code_index_vs_sweep", "round": rnd, "rows": N, "io": io, "max_batch": B, "layers": len(enc + dec),
                          "code_layers": tr.code_layers, "eval_sweep_ms": round(ms_sweep, 3), "code_index_ms": round(ms_index, 3),
                          "ratio": round(ms_index / ms_sweep, 3)}), flush=True)
    query = tr.encode(chunks[0][:args.queries], blank=0)
    ms_first, _ = wall_ms(lambda: index.similar(query, args.k, exclude=chunks[0][:args.queries]))
    print(json.dumps({"what": "similar_first_call", "note": "builds the retriever's tables (distinct folding on the host)", "bank": N,
                      "queries": int(query.shape[0]), "k": args.k, "ms": round(ms_first, 1)}), flush=True)
    for rnd in range(args.rounds):
        ms, _ = wall_ms(lambda: index.similar(query, args.k, exclude=chunks[0][:args.queries]))
        print(json.dumps({"what": "similar", "round": rnd, "bank": N, "width": index.width, "queries": int(query.shape[0]), "k": args.k,
                          "ms": round(ms, 3)}), flush=True)
    with tempfile.TemporaryDirectory() as d:
        for rnd in range(min(args.rounds, 3)):
            def script_extra():
                ix = tr.code_index()
                np.savez(os.path.join(d, "codes.npz"), codes=ix.bank.cpu().numpy(), rows=np.arange(N, dtype=np.int64), layer=np.int64(ix.layer))
            ms, _ = wall_ms(script_extra)
            print(json.dumps({"what": "script_extra", "round": rnd, "rows": N, "width": index.width, "ms": round(ms, 1),
                              "file_MB": round(os.path.getsize(os.path.join(d, "codes.npz")) / 1e6, 1)}), flush=True)


if __name__ == "__main__":
    main()
