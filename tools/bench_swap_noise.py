#!/usr/bin/env python3
"""Cost of swap noise at the headline shape (10 x Linear(1536, 1536), batch 8192, bf16): the whole fused training step and the
gather launch on its own (the engine's event pairs around its gather class) for four legs:

  none       no input noise: the gather reads the bf16 image of the dataset
  masking    element masking noise: the fp32-row gather every element noise takes (for scale)
  swap       swap noise, p = 0.15, a pool of half the rows: the swapped rows come from the bf16 image
  swap_f32   the same without a dataset image: the fp32-row swap gather

  python tools/bench_swap_noise.py [--steps K] [--warmup W] [--rounds N]                          this build, JSON lines
  python tools/bench_swap_noise.py --baseline-tree DIR [--alternations A] ...                     two builds, alternating

--baseline-tree DIR: a checkout of another commit, built in place (its library inside its own package).  The two builds then
alternate as fresh child processes of this tool on one machine, A times, so that a drift of the machine lands on both; every line
carries "build": "baseline" or "this".  A build that does not know a leg (the parent of swap noise has no swap) reports it as
unsupported.  Inside a process the legs alternate in every round; the spread across rounds and alternations is the noise floor of
the comparison.  DESIGN.md section 6 holds the numbers."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("none", "masking", "swap", "swap_f32")
DEV = "cuda:0"


def run_legs(args, tree, build):
    sys.path[:0] = [tree, os.path.join(tree, "mui-deepautoencoder_amd")]
    import numpy as np
    import torch
    from codae.hip import HipError
    from codae.model.schedule import linear_stack
    from codae.tool import InputNoise
    from codae.train import HipEmbeddingTrainer
    B, io = args.batch, args.io
    rng = np.random.default_rng(1234)
    n_rows = 4 * B
    data = torch.from_numpy(rng.random((n_rows, io), dtype=np.float32)).to(DEV)
    S = 3
    table = torch.ones((S, io), dtype=torch.uint8, device=DEV)
    for c in range(S):
        table[c, c * (io // S):(c + 1) * (io // S)] = 0
    mtu = torch.from_numpy(rng.integers(0, S, (n_rows, 1)).astype(np.int32)).to(DEV)
    idx = [torch.tensor(rng.permutation(n_rows)[:B], dtype=torch.int32, device=DEV) for _ in range(8)]
    pool = np.sort(rng.permutation(n_rows)[:n_rows // 2])
    enc, dec = linear_stack(io, io, 4, 4, False, False)
    trainers = {}
    for leg in LEGS:
        try:
            noise = {"none": lambda: None, "masking": lambda: InputNoise("masking", p=0.25, seed=1),
                     "swap": lambda: InputNoise("swap", p=0.15, seed=1, pool=pool),
                     "swap_f32": lambda: InputNoise("swap", p=0.15, seed=1, pool=pool)}[leg]()
        except (HipError, TypeError) as e:
            print(json.dumps({"what": "unsupported", "build": build, "leg": leg, "why": str(e)[:80]}), flush=True)
            continue
        tr = HipEmbeddingTrainer(enc + dec, data, table, mtu, 1e-5, 1e-4, 1.0, max_batch=B, precision="bf16", device=DEV,
                                 input_noise=noise, dataset_image=leg != "swap_f32")
        tr.init_params(seed=0)
        for s in range(args.warmup):
            tr.train_batch(idx[s % 8], run=0)
        trainers[leg] = tr
    torch.cuda.synchronize()
    for rnd in range(args.rounds):
        for leg, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(args.steps):
                tr.train_batch(idx[s % 8], run=0)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            print(json.dumps({"what": "fused_step", "build": build, "round": rnd, "leg": leg, "batch": B, "io": io, "layers": len(enc + dec),
                              "ms_per_step": round(ms, 4), "loss": tr.engine.read_scalars()[3]}), flush=True)
    # the gather launch of each leg, in a pass of its own (an event pair costs 2-4 us of stream time)
    for rnd in range(args.rounds):
        for leg, tr in trainers.items():
            tr.engine.profile_begin(classes=("gather",), max_records=args.steps)
            for s in range(args.steps):
                tr.train_batch(idx[s % 8], run=0)
            us = [1e3 * v for v in tr.engine.profile_end().get("gather", [])]
            print(json.dumps({"what": "gather_launch", "build": build, "round": rnd, "leg": leg, "launches": len(us),
                              "us_median": round(float(np.median(us)), 2), "us_min": round(min(us), 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--io", type=int, default=1536)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--baseline-tree", default=None)
    ap.add_argument("--alternations", type=int, default=2)
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)       # child mode: the tree whose package is imported
    ap.add_argument("--build", default="this", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.baseline_tree is None:
        run_legs(args, args.tree or HERE, args.build)
        return
    common = [sys.executable, os.path.abspath(__file__), "--batch", str(args.batch), "--io", str(args.io), "--steps", str(args.steps),
              "--warmup", str(args.warmup), "--rounds", str(args.rounds)]
    for alt in range(args.alternations):
        for build, tree in (("baseline", os.path.abspath(args.baseline_tree)), ("this", HERE)):
            print(json.dumps({"what": "process", "alternation": alt, "build": build}), flush=True)
            r = subprocess.run(common + ["--tree", tree, "--build", build], timeout=600)
            if r.returncode != 0:           # a build that failed: stop, start nothing more on the GPU
                sys.exit(r.returncode)


if __name__ == "__main__":
    main()
