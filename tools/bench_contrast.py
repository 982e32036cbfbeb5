#!/usr/bin/env python3
"""Cost of the slot contrast at the headline shape (10 x Linear(1536, 1536), S = 3 slots of E = 512, batch 8192): the whole fused
training step with the term off (the default step, loss in the last forward GEMM's epilogue), off with the MSE loss as the
stand-alone kernel (CODAE_NO_FUSED_LOSS: the route the step takes while the term is on), and on with K = 256 and K = 1024 - one
process, one box, the settings alternating inside every round - and then the term's own launches from the engine's event pairs
around its loss class (per step, in order: the criterion's kernel, the prepare launch, the contrast launch).

  python tools/bench_contrast.py [--precision bf16|f32] [--steps K] [--warmup W] [--rounds N]      JSON lines

Arithmetic of the contrast launch: two products of B x K x E per slot, one of them formed twice (the kernel makes two passes over
the logits): 2 * 2 * B * K * E * S = 51.5 GFLOP per step at K = 1024 as the definition counts it, 1.5 x that as executed.  The
`contrast` lines give the fraction of the dense MFMA peak (2.5 PFLOP/s bf16, 157 TFLOP/s fp32) the definition's count reaches.
DESIGN.md section 6 holds the numbers."""
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
from codae.tool import SlotContrast  # noqa: E402
from codae.train import HipEmbeddingTrainer  # noqa: E402

DEV = "cuda:0"
PEAK = {"bf16": 2.5e15, "f32": 157.3e12}


def settings(ks):
    """(name, contrast, stand-alone MSE loss).  distinct=False: random rows are all distinct items, and torch.unique over the
    dataset is not what is measured here."""
    on = [("K%d" % k, SlotContrast(negatives=k, temperature=0.1, seed=1, distinct=False), False) for k in ks]
    return [("off", None, False), ("off-standalone-loss", None, True)] + on


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--io", type=int, default=1536)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--negatives", default="256,1024")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    B, io, S = args.batch, args.io, 3
    ks = [int(k) for k in args.negatives.split(",")]
    rng = np.random.default_rng(1234)
    data = torch.from_numpy(rng.random((4 * B, io), dtype=np.float32)).to(DEV)
    table = torch.ones((S, io), dtype=torch.uint8, device=DEV)
    for c in range(S):
        table[c, c * (io // S):(c + 1) * (io // S)] = 0
    mtu = torch.from_numpy(rng.integers(0, S, (4 * B, 1)).astype(np.int32)).to(DEV)
    idx = [torch.tensor(rng.permutation(4 * B)[:B], dtype=torch.int32, device=DEV) for _ in range(8)]
    enc, dec = linear_stack(io, io, 4, 4, False, False)
    trainers = {}
    for name, contrast, standalone in settings(ks):
        if standalone:                      # (the switches are copied into the engine when it is created)
            os.environ["CODAE_NO_FUSED_LOSS"] = "1"
            hip.check(hip.lib().codae_reload_env())
        tr = HipEmbeddingTrainer(enc + dec, data, table, mtu, 1e-5, 1e-4, 1.0, max_batch=B, precision=args.precision, device=DEV,
                                 contrast=contrast)
        if standalone:
            del os.environ["CODAE_NO_FUSED_LOSS"]
            hip.check(hip.lib().codae_reload_env())
        tr.init_params(seed=0)
        for s in range(args.warmup):
            tr.train_batch(idx[s % 8], run=0)
        trainers[name] = tr
    torch.cuda.synchronize()
    for rnd in range(args.rounds):
        for name, *_ in settings(ks):
            tr = trainers[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(args.steps):
                tr.train_batch(idx[s % 8], run=0)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            print(json.dumps({"what": "fused_step", "round": rnd, "setting": name, "precision": args.precision, "batch": B, "io": io,
                              "layers": len(enc + dec), "ms_per_step": round(ms, 4), "loss": tr.engine.read_scalars()[3],
                              "path": tr.engine.step_path(B)}), flush=True)
    # the loss-class launches of each setting, in a pass of its own (an event pair costs 2-4 us of stream time)
    for rnd in range(args.rounds):
        for name, contrast, _ in settings(ks):
            tr = trainers[name]
            tr.engine.profile_begin(classes=("loss",), max_records=3 * args.steps)
            for s in range(args.steps):
                tr.train_batch(idx[s % 8], run=0)
            us = [1e3 * v for v in tr.engine.profile_end().get("loss", [])]
            if contrast is None:
                print(json.dumps({"what": "loss_launch", "round": rnd, "setting": name, "launches": len(us),
                                  "us_median": round(float(np.median(us)), 2), "us_min": round(min(us), 2)}), flush=True)
                continue
            for i, part in enumerate(("criterion", "prepare", "contrast")):
                v = us[i::3]
                line = {"what": "loss_launch", "round": rnd, "setting": name, "launch": part, "launches": len(v),
                        "us_median": round(float(np.median(v)), 2), "us_min": round(min(v), 2)}
                if part == "contrast":
                    flop = 2.0 * 2.0 * B * contrast.negatives * (io // S) * S
                    line["gflop_as_defined"] = round(flop / 1e9, 2)
                    line["fraction_of_mfma_peak"] = round(flop / (float(np.median(v)) * 1e-6) / PEAK[args.precision], 4)
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
