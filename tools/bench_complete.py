#!/usr/bin/env python3
"""Complementarity-inference throughput on one MI355X: ComplementRetriever.topk (codae_complete_topk = one fp32 GEMM per
candidate chunk + the HIP top-k selection pass) against the same retrieval in torch on the same GPU (normalize -> matmul
-> topk per chunk, running top-k merged with torch.topk), chunked the same way.

    python tools/bench_complete.py [--B 8192 --N 65536 --E 512 --k 10 100 --chunk 8192]      one JSON line per k
    python tools/bench_complete.py --iters 2 --no-torch                                      (the run to put under rocprofv3)
    python tools/bench_complete.py --summarize-stats results.db|kernel_stats.csv             GEMM / selection split, bytes/s

Queries all fill one slot, so the GEMM is B x N x E; the selection pass reads the B x chunk score block of every chunk
once (4 B N bytes per call); HBM_TBS is the measured copy rate it is compared with."""
import argparse
import csv
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mui-deepautoencoder_amd"))

HBM_TBS = 6.3


def torch_topk(q, inv_n, k, chunk):
    import torch
    qn = torch.nn.functional.normalize(q, dim=1, eps=1e-8)
    best_v = best_i = None
    for c0 in range(0, inv_n.shape[0], chunk):
        s = qn @ inv_n[c0:c0 + chunk].t()
        v, i = torch.topk(s, min(k, s.shape[1]), dim=1)
        i = i + c0
        if best_v is not None:
            v, j = torch.topk(torch.cat([best_v, v], 1), k, dim=1)
            i = torch.cat([best_i, i], 1).gather(1, j)
        best_v, best_i = v, i
    return best_i, best_v


def timed(fn, iters):
    import torch
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def summarize(path, B, N, chunk):
    """rocprofv3 --kernel-trace --stats output (kernel_stats.csv, or the SQLite results.db newer rocprofv3 writes by
    default) -> per kernel: launches, total / mean us, and for the selection kernels the score-block read rate"""
    per = {}
    if path.endswith(".db"):
        import sqlite3
        for name, n, tot in sqlite3.connect(path).execute("select name, count(*), sum(end - start) from kernels group by name"):
            per[name] = (int(n), float(tot))
    else:
        for r in csv.DictReader(open(path)):
            per[r["Name"]] = (int(r["Calls"]), float(r["TotalDurationNs"]))
    w = csv.writer(sys.stdout)
    w.writerow(["kernel", "calls", "total_us", "mean_us", "score_block_TBps", "frac_of_hbm"])
    block = 4.0 * B * min(chunk, N)                       # bytes of one chunk's score block
    for name, (n, tot) in sorted(per.items(), key=lambda kv: -kv[1][1]):
        mean = tot / n
        rate = frac = ""
        if "topk_merge_kernel" in name:
            rate = "%.2f" % (block / mean / 1e3)
            frac = "%.2f" % (block / mean / 1e3 / HBM_TBS)
        short = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:70]
        w.writerow([short, n, "%.1f" % (tot / 1e3), "%.1f" % (mean / 1e3), rate, frac])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--N", type=int, default=65536)
    ap.add_argument("--E", type=int, default=512)
    ap.add_argument("--k", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--chunk", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--summarize-stats")
    a = ap.parse_args()
    if a.summarize_stats:
        summarize(a.summarize_stats, a.B, a.N, a.chunk)
        return
    import torch
    from codae.tool import ComplementRetriever
    dev = "cuda:0"
    g = torch.Generator(device="cpu").manual_seed(0)
    inv = torch.randn(a.N, a.E, generator=g)
    ds = types.SimpleNamespace(nb_used_category=1, embedding_size=a.E, data_per_category={0: inv})
    q = (inv[torch.randint(0, a.N, (a.B,), generator=g)] + 0.3 * torch.randn(a.B, a.E, generator=g)).to(dev)
    t0 = time.perf_counter()
    r = ComplementRetriever(ds, dev, distinct=False)
    r._device_tables(torch.device(dev))
    build_s = time.perf_counter() - t0
    inv_n = torch.nn.functional.normalize(inv.to(dev), dim=1, eps=1e-8)
    for k in a.k:
        res = {"B": a.B, "N": a.N, "E": a.E, "k": k, "chunk": a.chunk, "table_build_s": round(build_s, 2)}
        ms = timed(lambda: r.topk(q, 0, k, chunk=a.chunk), a.iters)
        res["hip_ms"] = round(ms, 3)
        res["hip_queries_per_s"] = round(a.B / ms * 1e3)
        res["gemm_tflops_if_all_gemm"] = round(2.0 * a.B * a.N * a.E / ms / 1e9, 1)
        if not a.no_torch:
            tms = timed(lambda: torch_topk(q, inv_n, k, a.chunk), a.iters)
            res["torch_ms"] = round(tms, 3)
            res["torch_queries_per_s"] = round(a.B / tms * 1e3)
            hi, hs = r.topk(q, 0, k, chunk=a.chunk)
            ti, ts = torch_topk(q, inv_n, k, a.chunk)
            res["max_score_diff_vs_torch"] = float((hs - ts).abs().max())
            res["top1_agree"] = float((hi[:, 0] == ti[:, 0]).float().mean())
            res["faster"] = "hip" if ms < tms else "torch"
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
