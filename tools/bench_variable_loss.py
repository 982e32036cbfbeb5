#!/usr/bin/env python3
"""Cost of a mixed-variable training step three ways, alternating inside every round in one process: the drop-in loop body of
script/train_dae_on_abalone.py (model + CombinedCriterion through autograd + torch clip_grad_norm_ + torch Adam), the fused HIP step
with the criterion in it (codae.tool.VariableLoss), and that step replayed from a hipGraph.  Two shapes, fp32:
  abalone   the abalone_k2 shape: batch 64, 6 x Linear(11, 11), 9 variables (one 3-wide one-hot, 8 numeric)
  table     a synthetic table of 1 M rows x io 64 at batch 8192: 6 x Linear(64, 64), 32 variables (8 one-hots of 5, 24 numeric)
and the three loss launches' own times from the engine's profile, in a pass of its own.

  python tools/bench_variable_loss.py [--steps K] [--warmup W] [--rounds N]      JSON lines, then one summary line per case

The spread across rounds (min - max) is the noise floor of every comparison.  DESIGN.md section 6 holds the numbers."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mui-deepautoencoder_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from codae.model import MixedVariableDenoisingAutoencoder  # noqa: E402
from codae.tool import CombinedCriterion, Corrupter, VariableLoss  # noqa: E402
from codae.train import HipEmbeddingTrainer  # noqa: E402

DEV = "cuda:0"
RESULTS = {}


def record(case, value, line):
    RESULTS.setdefault(case, []).append(value)
    print(json.dumps(line), flush=True)


def table_rows(arch, n, rng):
    io = arch[-1]["position"] + arch[-1]["size"]
    x = rng.random((n, io), dtype=np.float32)
    for v in arch:
        if v["type"] == "classification":
            p, s = v["position"], v["size"]
            x[:, p:p + s] = 0
            x[np.arange(n), p + rng.integers(0, s, n)] = 1
    return x


def shapes():
    abalone = [{"position": 0, "size": 3, "type": "classification"}] + [{"position": 3 + i, "size": 1, "type": "regression"} for i in range(8)]
    table = [{"position": 5 * i, "size": 5, "type": "classification"} for i in range(8)]
    table += [{"position": 40 + i, "size": 1, "type": "regression"} for i in range(24)]
    return {"abalone": dict(arch=abalone, rows=4177, batch=64, layers=2), "table": dict(arch=table, rows=1 << 20, batch=8192, layers=2)}


class DropIn:
    """The loop body of the script."""

    def __init__(self, model, arch, weight, corrupter, data, lr, wd):
        dev = torch.device(DEV)
        self.model, self.corrupter, self.data = model, corrupter, data
        self.opt = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=wd)
        type_mask = torch.cat([torch.zeros(v["size"]) if v["type"] == "classification" else torch.ones(v["size"]) for v in arch])
        self.crit = CombinedCriterion(arch=arch, k_max=1, device=dev, observation_mask=type_mask, weight=weight, reduction="mean")

    def step(self, rows, run):
        x = self.data[rows]
        _, fmask = self.corrupter.get_masks(rows, run)
        y = self.model(self.model.corrupt(input_data=x, mask=fmask))
        loss = self.crit(x=x, y=y)
        self.opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(self.model.parameters(), 1)
        self.opt.step()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device(DEV)
    rng = np.random.default_rng(1234)
    for name, sh in shapes().items():
        arch, N, B = sh["arch"], sh["rows"], sh["batch"]
        io = arch[-1]["position"] + arch[-1]["size"]
        weight = [0.4] + [1] * (len(arch) - 1)
        data = torch.from_numpy(table_rows(arch, N, rng)).to(dev)
        # (the Corrupter draws a row's mask order with Python's random, row by row: at 1 M rows the table is drawn here instead)
        corrupter = Corrupter(nb_observation=8, arch=arch, k_max=1, device=dev)
        corrupter.mask_to_use = torch.from_numpy(rng.random((N, corrupter.nb_run)).argsort(axis=1))
        corrupter.mask_to_use_i32 = corrupter.mask_to_use.to(torch.int32).contiguous().to(dev)
        torch.manual_seed(0)
        model = MixedVariableDenoisingAutoencoder(arch, io, io, dev, sh["layers"], sh["layers"], False)
        model.to(dev)
        params = [(l.weight.detach().clone(), l.bias.detach().clone()) for l in model._linears()]
        idx = [torch.tensor(rng.permutation(N)[:B], dtype=torch.int64, device=dev) for _ in range(8)]
        idx32 = [i.to(torch.int32) for i in idx]
        runners = {"dropin": DropIn(model, arch, weight, corrupter, data, 1e-4, 1e-6)}
        for form, graph in (("fused", False), ("fused_graph", True)):
            tr = HipEmbeddingTrainer(model._schedule, data, corrupter.mask_table_u8, corrupter.mask_to_use_i32, 1e-4, 1e-6, clip=1.0, max_batch=B,
                                     precision="f32", device=DEV, use_graph=graph, criterion=VariableLoss(arch, weight))
            tr.load_params(params)
            runners[form] = tr

        def run_steps(form, n):
            r = runners[form]
            for s in range(n):
                if form == "dropin":
                    r.step(idx[s % 8], 0)
                else:
                    r.train_batch(idx32[s % 8], run=0)
        for form in runners:
            run_steps(form, args.warmup)
        torch.cuda.synchronize()
        for rnd in range(args.rounds):
            for form in runners:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run_steps(form, args.steps)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3 / args.steps
                record("%s %s" % (name, form), ms, {"what": "step", "round": rnd, "shape": name, "form": form, "batch": B, "io": io,
                                                    "n_var": len(arch), "layers": len(model._schedule), "ms_per_step": round(ms, 4)})
        n = 10
        tr = runners["fused"]
        tr.engine.profile_begin(classes=("loss",), max_records=16 * n)
        for s in range(n):
            tr.train_batch(idx32[s % 8], run=0)
        us = [1e3 * v for v in tr.engine.profile_end().get("loss", [])]
        per = max(len(us) // n, 1)
        print(json.dumps({"what": "loss_launches", "shape": name, "per_step": len(us) // n,
                          "partials_us_median": round(float(np.median(us[0::per])), 2) if us else None,
                          "finish_us_median": round(float(np.median(us[1::per])), 2) if len(us) > 1 else None,
                          "grad_us_median": round(float(np.median(us[2::per])), 2) if len(us) > 2 else None}), flush=True)
        del runners, tr, data
    for case, vals in RESULTS.items():
        print("SUMMARY %-24s median %9.4f   min - max %9.4f - %9.4f   (ms per step, %d rounds)" % (
            case, float(np.median(vals)), min(vals), max(vals), len(vals)))


if __name__ == "__main__":
    main()
