#!/usr/bin/env python3
"""Cost of the validation retrieval metrics on one MI355X, against the rank metric they sit beside: RetrievalMetrics.add
(codae_retrieval_metrics_batched) and RankingLoss.add (codae_ranking_loss_batched) on the same batch, tables and chunking, in ONE
process, alternating (rank metric, retrieval metrics, rank metric) in every round, warmed up and synchronised - the two rank-metric
figures of a round show the spread the comparison has to be read against.

    python tools/bench_retrieval_metrics.py [--B 8192 --V 65536 --E 512 --S 3 --chunk 8192 --rounds 5 --iters 3]
    python tools/bench_retrieval_metrics.py --rounds 1 --iters 1                                 (the run to put under rocprofv3)
    python tools/bench_retrieval_metrics.py --summarize-stats results.db|kernel_stats.csv        per kernel: us, score-block read rate

Both read every B/S x chunk score block once (4 B V bytes per call over the S slots); HBM_TBS is the measured copy rate the count
passes are compared with."""
import argparse
import csv
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mui-deepautoencoder_amd"))

HBM_TBS = 6.3


def timed(fn, iters):
    import torch
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def summarize(path, B, V, S, chunk):
    """rocprofv3 --kernel-trace --stats output (kernel_stats.csv or results.db) -> per kernel: launches, total / mean us, and
    for the two count passes the rate at which they read their score block (B / S rows of one chunk)"""
    per = {}
    if path.endswith(".db"):
        import sqlite3
        db = sqlite3.connect(path)
        tables = [r[0] for r in db.execute("select name from sqlite_master where type in ('table', 'view')")]
        view = "kernels" if "kernels" in tables else [t for t in tables if t.startswith("kernels")][0]
        for name, n, tot in db.execute("select name, count(*), sum(end - start) from %s group by name" % view):
            per[name] = (int(n), float(tot))
    else:
        for r in csv.DictReader(open(path)):
            per[r["Name"]] = (int(r["Calls"]), float(r["TotalDurationNs"]))
    w = csv.writer(sys.stdout)
    w.writerow(["kernel", "calls", "total_us", "mean_us", "score_block_TBps", "frac_of_hbm"])
    block = 4.0 * (B / S) * min(chunk, V)
    for name, (n, tot) in sorted(per.items(), key=lambda kv: -kv[1][1]):
        mean = tot / n
        rate = frac = ""
        if "metrics_count_kernel" in name or "rank_count_kernel" in name:
            rate = "%.2f" % (block / mean / 1e3)
            frac = "%.2f" % (block / mean / 1e3 / HBM_TBS)
        short = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:70]
        w.writerow([short, n, "%.1f" % (tot / 1e3), "%.1f" % (mean / 1e3), rate, frac])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--V", type=int, default=65536)
    ap.add_argument("--E", type=int, default=512)
    ap.add_argument("--S", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--distinct", action="store_true", help="fold duplicate rows into items (a host pass over the inventory; none here)")
    ap.add_argument("--summarize-stats")
    a = ap.parse_args()
    if a.summarize_stats:
        summarize(a.summarize_stats, a.B, a.V, a.S, a.chunk)
        return
    import torch
    from codae.tool import RankingLoss, RetrievalMetrics
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    S, E, V, B = a.S, a.E, a.V, a.B
    ds = types.SimpleNamespace(nb_used_category=S, embedding_size=E, nb_predictor=S * E,
                               data_per_category={c: torch.randn(V, E, generator=g) for c in range(S)})
    table = torch.ones(S, S * E, dtype=torch.uint8)
    for c in range(S):
        table[c, c * E:(c + 1) * E] = 0
    corr = types.SimpleNamespace(mask_table_u8=table.to(dev), mask_to_use_i32=torch.randint(0, S, (V, 1), generator=g, dtype=torch.int32).to(dev))
    val = list(range(V))
    idx = torch.randperm(V, generator=g)[:B].to(torch.int32)
    pred = (torch.cat([ds.data_per_category[c][idx.long()] for c in range(S)], dim=1) * 0.3 + torch.randn(B, S * E, generator=g)).to(dev)
    idx = idx.to(dev)
    rl = RankingLoss(ds, val, device=dev)
    rm = RetrievalMetrics(ds, val, dev, ks=(1, 10, 50), distinct=a.distinct)
    run_rl = lambda: rl.add(pred, idx, corr, run=0, chunk=a.chunk)            # noqa: E731
    run_rm = lambda: rm.add(pred, idx, corr, run=0, chunk=a.chunk)            # noqa: E731
    for fn in (run_rl, run_rm, run_rl, run_rm):                                # warm-up: tables, workspaces, code objects
        fn()
    torch.cuda.synchronize()
    rows = []
    for r in range(a.rounds):
        t = {"round": r, "ranking_loss_ms": round(timed(run_rl, a.iters), 3), "retrieval_metrics_ms": round(timed(run_rm, a.iters), 3),
             "ranking_loss_again_ms": round(timed(run_rl, a.iters), 3)}
        rows.append(t)
        print(json.dumps(t), flush=True)
    n_calls = 2 + (2 * a.rounds) * a.iters
    rl_total, m = rl.total(), rm.total()
    med = lambda k: statistics.median(t[k] for t in rows)                      # noqa: E731
    print(json.dumps({"B": B, "V": V, "E": E, "S": S, "chunk": a.chunk, "rounds": a.rounds, "iters": a.iters,
                      "ranking_loss_ms": med("ranking_loss_ms"), "ranking_loss_again_ms": med("ranking_loss_again_ms"),
                      "retrieval_metrics_ms": med("retrieval_metrics_ms"),
                      "ranking_loss_spread_ms": round(max(abs(t["ranking_loss_ms"] - t["ranking_loss_again_ms"]) for t in rows), 3),
                      "rre_ranking_loss": rl_total / (n_calls * B), "rre_retrieval_metrics": m["rre"], "mrr": m["mrr"],
                      "hit@10": m["hit@10"], "pairs_per_call": m["pairs"] / (2 + a.rounds * a.iters)}), flush=True)


if __name__ == "__main__":
    main()
