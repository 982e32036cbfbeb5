#!/usr/bin/env python3
"""Cost of hidden dropout at the headline shape (10 x Linear(1536, 1536), batch 8192, bf16): the whole fused training step
with dropout off, on the code layer only (p = 0.5 on one hidden output) and on all nine hidden outputs (p = 0.5), and the
launches of class `dropout` on their own (the engine's event pairs) with the bytes each moves - 2 * B * ld * esize: the
matrix is read and written once - beside what the gather achieves in the same run (it reads B * io * 4 and writes
B * ld * esize).

  python tools/bench_dropout.py [--steps K] [--warmup W] [--rounds N]      JSON lines

The settings alternate inside every round, so that a drift of the machine lands on all of them; every round prints its own
line and the spread across rounds is the noise floor of the comparison.  DESIGN.md section 6 holds the numbers."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mui-deepautoencoder_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from codae.model.schedule import linear_stack  # noqa: E402
from codae.tool import HiddenDropout  # noqa: E402
from codae.train import HipEmbeddingTrainer  # noqa: E402

DEV = "cuda:0"


def settings(sched):
    n_hidden = len(sched) - 1
    code = [0.0] * n_hidden
    linear = [l for l in range(n_hidden) if not sched[l][2]]       # the encoder's last Linear has no activation: the code layer
    code[linear[0] if linear else (n_hidden - 1) // 2] = 0.5
    return [("off", None), ("code", HiddenDropout(code, seed=1)), ("all", HiddenDropout(0.5, seed=1))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--io", type=int, default=1536)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
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
    sched = enc + dec
    sets = settings(sched)
    trainers = {}
    for name, drop in sets:
        tr = HipEmbeddingTrainer(sched, data, table, mtu, 1e-5, 1e-4, 1.0, max_batch=B, precision="bf16", device=DEV, hidden_dropout=drop)
        tr.init_params(seed=0)
        for s in range(args.warmup):
            tr.train_batch(idx[s % 8], run=0)
        trainers[name] = tr
    torch.cuda.synchronize()
    for rnd in range(args.rounds):
        for name, _ in sets:
            tr = trainers[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(args.steps):
                tr.train_batch(idx[s % 8], run=0)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            print(json.dumps({"what": "fused_step", "round": rnd, "setting": name, "batch": B, "io": io, "layers": len(sched),
                              "ms_per_step": round(ms, 4), "loss": tr.engine.read_scalars()[3], "path": tr.engine.step_path(B)}), flush=True)
    # the dropout launches (and the gather) of each setting, in a pass of its own (an event pair costs 2-4 us of stream time).  A step
    # records its forward launches first (layers ascending), then its backward launches (descending): n of each.
    ld = (io + 63) // 64 * 64
    drop_bytes = 2 * B * ld * 2
    gather_bytes = B * io * 4 + B * ld * 2
    for rnd in range(args.rounds):
        for name, drop in sets:
            tr = trainers[name]
            n = 0 if drop is None else sum(1 for v in drop.per_layer(len(sched)) if v > 0)
            tr.engine.profile_begin(classes=("dropout", "gather"), max_records=args.steps * (2 * n + 1))
            for s in range(args.steps):
                tr.train_batch(idx[s % 8], run=0)
            rec = tr.engine.profile_end()
            us = [1e3 * v for v in rec.get("dropout", [])]
            gus = [1e3 * v for v in rec.get("gather", [])]
            line = {"what": "launches", "round": rnd, "setting": name, "gather_us_median": round(float(np.median(gus)), 2),
                    "gather_TBps": round(gather_bytes / (float(np.median(gus)) * 1e-6) / 1e12, 3)}
            for kind, sel in (("fwd", [u for i, u in enumerate(us) if n and i % (2 * n) < n]),
                              ("bwd", [u for i, u in enumerate(us) if n and i % (2 * n) >= n])):
                if sel:
                    med = float(np.median(sel))
                    line.update({kind + "_launches": len(sel), kind + "_us_median": round(med, 2), kind + "_us_min": round(min(sel), 2),
                                 kind + "_bytes": drop_bytes, kind + "_TBps": round(drop_bytes / (med * 1e-6) / 1e12, 3)})
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
