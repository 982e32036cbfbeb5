#!/usr/bin/env python3
"""Cost of a slot-presence table on the path it shares (headline shape: 10 x Linear(1536, 1536), S = 3 slots of 512, batch 8192,
bf16; --io 512 --layers 3 --slots 4 is the small shape DESIGN.md also quotes): the whole fused training
step with no table (the loss in the last forward GEMM's epilogue), with the stand-alone loss under unit weights (LossEmphasis with
a column-weight vector of ones: the kernel a table routes the plain MSE to, without the predicate) and with a table that has about
30 % of the slots absent, and the gather and loss launches of each setting on their own (the engine's event pairs).

  python tools/bench_presence.py [--steps K] [--warmup W] [--rounds N]      JSON lines

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

from codae.tool import LossEmphasis, SlotPresence  # noqa: E402
from codae.train import HipEmbeddingTrainer  # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--io", type=int, default=1536)
    ap.add_argument("--layers", type=int, default=10)
    ap.add_argument("--slots", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    B, io, S = args.batch, args.io, args.slots
    rng = np.random.default_rng(1234)
    n_rows = 4 * B
    data = torch.from_numpy(rng.random((n_rows, io), dtype=np.float32)).to(DEV)
    table = torch.ones((S, io), dtype=torch.uint8, device=DEV)
    for c in range(S):
        table[c, c * (io // S):(c + 1) * (io // S)] = 0
    mtu = torch.from_numpy(rng.integers(0, S, (n_rows, 1)).astype(np.int32)).to(DEV)
    present = (rng.random((n_rows, S)) >= 0.3).astype(np.uint8)
    for r in np.flatnonzero(present.sum(axis=1) < 2):
        present[r, rng.permutation(S)[:2]] = 1
    idx = [torch.tensor(rng.permutation(n_rows)[:B], dtype=torch.int32, device=DEV) for _ in range(8)]
    sched = [(io, io, l + 1 < args.layers) for l in range(args.layers)]
    settings = [("off", {}), ("standalone_unit", dict(loss_emphasis=LossEmphasis(column_weight=[1.0] * io))),
                ("presence", dict(presence=SlotPresence(present)))]
    trainers = {}
    for name, kw in settings:
        tr = HipEmbeddingTrainer(sched, data, table, mtu, 1e-5, 1e-4, 1.0, max_batch=B, precision="bf16", device=DEV, n_slots=S, **kw)
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
            print(json.dumps({"what": "fused_step", "round": rnd, "setting": name, "batch": B, "io": io, "layers": args.layers,
                              "absent": round(float((present == 0).mean()), 3) if name == "presence" else 0.0,
                              "ms_per_step": round(ms, 4), "loss": tr.engine.read_scalars()[3], "path": tr.engine.step_path(B)}), flush=True)
    # the gather and loss launches of each setting, in a pass of their own (an event pair costs 2-4 us of stream time)
    for rnd in range(args.rounds):
        for name, _ in settings:
            tr = trainers[name]
            tr.engine.profile_begin(classes=("loss", "gather"), max_records=2 * args.steps)
            for s in range(args.steps):
                tr.train_batch(idx[s % 8], run=0)
            rec = tr.engine.profile_end()
            out = {"what": "launches", "round": rnd, "setting": name}
            for k in ("gather", "loss"):
                us = [1e3 * v for v in rec.get(k, [])]
                out[k + "_us_median"] = round(float(np.median(us)), 2) if us else None
                out[k + "_launches"] = len(us)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
