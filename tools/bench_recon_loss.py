#!/usr/bin/env python3
"""Cost of the training criteria at the headline shape (10 x Linear(1536, 1536), batch 8192, bf16): the whole fused training
step under each criterion (L1, SmoothL1, Huber, slot_cosine, slot_cosine + MSE anchor, slot_cosine + emphasis + MASKING noise)
against two baselines of the same commit on the same box in the same run - the MSE step with its loss as the stand-alone kernel
(CODAE_NO_FUSED_LOSS: the route every criterion takes) and the default step with the loss in the last forward GEMM's epilogue -
and the loss launch of each setting on its own (the engine's own event pairs around its loss class: for a criterion that is
recon_elem_kernel or slot_cosine_kernel alone, for `mse-standalone` mse_loss_kernel, for `mse-fused` the last GEMM with the loss).

  python tools/bench_recon_loss.py [--steps K] [--warmup W] [--rounds N]      JSON lines

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

from codae import hip  # noqa: E402
from codae.model.schedule import linear_stack  # noqa: E402
from codae.tool import InputNoise, LossEmphasis, ReconstructionLoss  # noqa: E402
from codae.train import HipEmbeddingTrainer  # noqa: E402

DEV = "cuda:0"


def settings():
    """(name, criterion, emphasis, noise, stand-alone MSE loss)"""
    emph = LossEmphasis(3.0, 1.0, slot_weight=[1.0, 1.0, 2.0])
    return [("mse-fused", None, None, None, False), ("mse-standalone", None, None, None, True),
            ("l1", ReconstructionLoss("l1"), None, None, False), ("smooth_l1", ReconstructionLoss("smooth_l1", beta=0.5), None, None, False),
            ("huber", ReconstructionLoss("huber", delta=1.0), None, None, False),
            ("slot_cosine", ReconstructionLoss("slot_cosine"), None, None, False),
            ("slot_cosine+mse", ReconstructionLoss("slot_cosine", mse_weight=0.1), None, None, False),
            ("slot_cosine+mse+emphasis+masking", ReconstructionLoss("slot_cosine", mse_weight=0.1), emph, InputNoise("masking", p=0.25, seed=1), False)]


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
    trainers = {}
    for name, crit, emph, noise, standalone in settings():
        if standalone:                      # (the switches are copied into the engine when it is created)
            os.environ["CODAE_NO_FUSED_LOSS"] = "1"
            hip.check(hip.lib().codae_reload_env())
        tr = HipEmbeddingTrainer(enc + dec, data, table, mtu, 1e-5, 1e-4, 1.0, max_batch=B, precision="bf16", device=DEV,
                                 input_noise=noise, loss_emphasis=emph, criterion=crit)
        if standalone:
            del os.environ["CODAE_NO_FUSED_LOSS"]
            hip.check(hip.lib().codae_reload_env())
        tr.init_params(seed=0)
        for s in range(args.warmup):
            tr.train_batch(idx[s % 8], run=0)
        trainers[name] = tr
    torch.cuda.synchronize()
    for rnd in range(args.rounds):
        for name, *_ in settings():
            tr = trainers[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(args.steps):
                tr.train_batch(idx[s % 8], run=0)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            print(json.dumps({"what": "fused_step", "round": rnd, "setting": name, "batch": B, "io": io, "layers": len(enc + dec),
                              "ms_per_step": round(ms, 4), "loss": tr.engine.read_scalars()[3], "path": tr.engine.step_path(B)}), flush=True)
    # the loss launch of each setting, in a pass of its own (an event pair costs 2-4 us of stream time)
    for rnd in range(args.rounds):
        for name, *_ in settings():
            tr = trainers[name]
            tr.engine.profile_begin(classes=("loss",), max_records=args.steps)
            for s in range(args.steps):
                tr.train_batch(idx[s % 8], run=0)
            us = [1e3 * v for v in tr.engine.profile_end().get("loss", [])]
            print(json.dumps({"what": "loss_launch", "round": rnd, "setting": name, "launches": len(us),
                              "us_median": round(float(np.median(us)), 2), "us_min": round(min(us), 2)}), flush=True)


if __name__ == "__main__":
    main()
