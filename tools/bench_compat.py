#!/usr/bin/env python3
"""Cost of the validation compatibility metric on one MI355X, against the validation sweep it rides on: (a) the plain eval_batch
sweep over V validation rows, (b) the same sweep plus CompatibilityMetrics.add_batch for every batch and one total(), in ONE process,
alternating (a, b, a) in every round, timed with device events after a warm-up - the two (a) figures of a round show the spread the
ratio has to be read against.

    python tools/bench_compat.py [--S 3 --E 512 --batch 8192 --V 65536 --negatives 1 --precision bf16 --rounds 3]
    python tools/bench_compat.py --rounds 1                                  (the run to put under rocprofv3 --kernel-trace --stats)
    python tools/bench_compat.py --summarize-stats results.db|kernel_stats.csv    per kernel: launches, total and mean us

By counts (b) adds (1 + negatives) S forward rows per validation row - each outfit and each negative once per left-out slot -, the
assemble and score passes (2 Q S io elements moved) and one P x M count; the printed `forward_rows_ratio` is 1 + (1 + negatives) S,
the figure `ratio` is to be read beside."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mui-deepautoencoder_amd"))


def timed(fn):
    import torch
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def summarize(path):
    """rocprofv3 --kernel-trace --stats output (kernel_stats.csv or results.db) -> per kernel: launches, total / mean us"""
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
    w.writerow(["kernel", "calls", "total_us", "mean_us"])
    for name, (n, tot) in sorted(per.items(), key=lambda kv: -kv[1][1]):
        short = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:90]
        w.writerow([short, n, "%.1f" % (tot / 1e3), "%.1f" % (tot / n / 1e3)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, default=3)
    ap.add_argument("--E", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--V", type=int, default=65536)
    ap.add_argument("--negatives", type=int, default=1)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--layers", type=int, default=10, help="square Linears of width S E (the flagship stack has 10)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-distinct", action="store_true", help="a donor is another row, not another item (no host pass over the bytes)")
    ap.add_argument("--summarize-stats")
    a = ap.parse_args()
    if a.summarize_stats:
        summarize(a.summarize_stats)
        return
    import torch
    from codae.train import HipEmbeddingTrainer
    dev = torch.device("cuda:0")
    S, E, V, B = a.S, a.E, a.V, a.batch
    io = S * E
    g = torch.Generator(device="cpu").manual_seed(0)
    data = torch.randn(V, io, generator=g)
    relu = [True] * (a.layers // 2 - 1) + [False] + [True] * (a.layers - a.layers // 2 - 1) + [False]
    table = torch.ones(S, io, dtype=torch.uint8)
    for c in range(S):
        table[c, c * E:(c + 1) * E] = 0
    m2u = torch.randint(0, S, (V, 1), generator=g, dtype=torch.int32)
    tr = HipEmbeddingTrainer([(io, io, r) for r in relu], data, table, m2u, 1e-5, 1e-4, 1.0, max_batch=B, precision=a.precision, device=dev)
    tr.init_params(seed=0)
    t0 = time.time()
    cm = tr.compatibility_metrics(list(range(V)), negatives=a.negatives, seed=0, distinct=not a.no_distinct)
    table_s = time.time() - t0
    order = torch.randperm(V, generator=g).to(torch.int32).to(dev)
    batches = [order[o:o + B].contiguous() for o in range(0, V, B)]

    def sweep_plain():
        for idx in batches:
            tr.eval_batch(idx, run=0)

    last = {}

    def sweep_compat():
        for idx in batches:
            tr.eval_batch(idx, run=0)
            cm.add_batch(idx)
        last.update(cm.total())

    for fn in (sweep_plain, sweep_compat):                                    # warm-up: code objects, workspaces, allocator
        fn()
    rows = []
    for r in range(a.rounds):
        t = {"round": r, "plain_ms": round(timed(sweep_plain), 3), "with_compat_ms": round(timed(sweep_compat), 3),
             "plain_again_ms": round(timed(sweep_plain), 3)}
        rows.append(t)
        print(json.dumps(t), flush=True)
    med = lambda k: statistics.median(t[k] for t in rows)                     # noqa: E731
    plain = 0.5 * (med("plain_ms") + med("plain_again_ms"))
    print(json.dumps({"S": S, "E": E, "batch": B, "V": V, "negatives": a.negatives, "precision": a.precision, "layers": a.layers,
                      "distinct": not a.no_distinct, "rounds": a.rounds, "plain_ms": med("plain_ms"), "plain_again_ms": med("plain_again_ms"),
                      "with_compat_ms": med("with_compat_ms"), "ratio": round(med("with_compat_ms") / plain, 3),
                      "forward_rows_ratio": 1 + (1 + a.negatives) * S,
                      "plain_spread_ms": round(max(abs(t["plain_ms"] - t["plain_again_ms"]) for t in rows), 3),
                      "negatives_table_host_s": round(table_s, 2), "auc": last.get("auc"), "paired_acc": last.get("paired_acc"),
                      "outfits": last.get("outfits"), "pairs": last.get("pairs")}), flush=True)


if __name__ == "__main__":
    main()
