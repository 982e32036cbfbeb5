#!/usr/bin/env python3
"""ms per fused training step at C3 (3 slots x 512: io 1536, 10 x Linear(1536, 1536), batch 8192) for ReLU and the
generic-activation path (ELU, SELU, LeakyReLU), bf16 and fp32 engines.  One JSON line per (precision, activation).

  python tools/bench_activation.py [--steps K] [--warmup W] [--batch B]

ReLU runs the pinned pipelined kernels, 1-bit masks and all; every other kind the one-barrier 128 x 128 / 64 x 64 kernels'
generic epilogues (activations)."""
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
from codae.train import HipEmbeddingTrainer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--precision", default="bf16,f32")
    args = ap.parse_args()
    io, B = 1536, args.batch
    enc, dec = linear_stack(io, io, 4, 4, False, False)
    rng = np.random.default_rng(1234)
    data = torch.from_numpy(rng.random((4 * B, io), dtype=np.float32))
    idx = [torch.tensor(rng.permutation(len(data))[:B], dtype=torch.int32, device="cuda:0") for _ in range(8)]
    acts = [("ReLU", None), ("ELU", torch.nn.ELU), ("SELU", torch.nn.SELU),
            ("LeakyReLU", lambda inplace: torch.nn.LeakyReLU(0.01, inplace))]
    for prec in args.precision.split(","):
        for name, act in acts:
            tr = HipEmbeddingTrainer(enc + dec, data, None, None, 1e-5, 1e-4, 1.0, max_batch=B, precision=prec,
                                     device="cuda:0", activation=act)
            tr.init_params(seed=0)
            for s in range(args.warmup):
                tr.train_batch(idx[s % 8], run=None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(args.steps):
                tr.train_batch(idx[s % 8], run=None)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            loss = tr.engine.read_scalars()[3]
            print(json.dumps({"precision": prec, "activation": name, "batch": B, "ms_per_step": round(ms, 4),
                              "loss": loss, "path": tr.engine.step_path(B)}), flush=True)
            del tr
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
