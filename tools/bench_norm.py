#!/usr/bin/env python3
"""Cost of normalisation at the headline shape (10 x Linear(1536, 1536) = 3 slots x 512, batch 8192, bf16): the whole fused training
step with the norm off and with Norm("layer"), Norm("rms"), each alone and with Residual("hidden"), alternating inside every round in
one process, and the two new kernels on their own beside the residual and dropout kernels on the same [8192][1536] bf16 matrix
(device events around `reps` back-to-back launches of the stand-alone launchers).

  python tools/bench_norm.py [--steps K] [--warmup W] [--rounds N] [--only SETTING]      JSON lines

Bytes per launch are counted from the shapes (what the algorithm must move once, not what the caches served on the later passes):
  norm_fwd       read and write act[l + 1], write r, write the bits                              2 B W e + 4 B (+ B W / 8)
  norm_bwd       read U, write D, read xhat (working precision), read r, read the bits           3 B W e + 4 B + B W / 8
  norm_bwd + G   ... and read + write G (fp32)                                                   3 B W e + 8 B W + 4 B + B W / 8
  residual_fwd / residual_bwd / dropout_fwd / dropout_bwd   as tools/bench_residual.py counts them
The spread across rounds is the noise floor of every comparison.  DESIGN.md section 6 holds the numbers.
`in_step_launches` counts the launches of the streaming class per step from the engine's own profile: with a norm and a skip on the
same layers the backward has ONE launch per data-gradient site (the norm kernel takes the residual kernel's place)."""
import argparse
import ctypes as C
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
from codae.tool import Norm, Residual  # noqa: E402
from codae.train import HipEmbeddingTrainer  # noqa: E402

DEV = "cuda:0"


def time_launches(fn, reps):
    """us per launch of `reps` back-to-back launches between two device events (after two unrecorded ones)"""
    fn(); fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def kernels(B, W, reps, rounds):
    lib = hip.lib()
    s = hip.current_stream()
    y = torch.randn((B, W), device=DEV).to(torch.bfloat16)
    x = torch.randn((B, W), device=DEV).to(torch.bfloat16)
    g = torch.randn((B, W), device=DEV)
    r = torch.ones((B,), device=DEV)
    bits = torch.zeros((B, W // 8), dtype=torch.uint8, device=DEV)
    parts = torch.zeros((lib.codae_norm_blocks(B), W), device=DEV)
    p = (C.c_float * 3)(0.0, 0.0, 0.0)
    e = 2
    cases = {}
    for kind, kid in (("layer", 1), ("rms", 2)):
        cases["norm_fwd_" + kind] = (lambda kid=kid: hip.check(lib.codae_norm_fwd(hip.ptr(y), 1, W, B, W, kid, 1e-5, hip.ptr(r), hip.ptr(bits), W // 8, s)),
                                     2 * B * W * e + 4 * B + B * W // 8)
        cases["norm_fwd_eval_" + kind] = (lambda kid=kid: hip.check(lib.codae_norm_fwd(hip.ptr(y), 1, W, B, W, kid, 1e-5, hip.ptr(r), None, 0, s)),
                                          2 * B * W * e + 4 * B)
        cases["norm_bwd_" + kind] = (lambda kid=kid: hip.check(lib.codae_norm_bwd(hip.ptr(y), 1, W, B, W, kid, hip.ptr(x), W, hip.ptr(r), None, None, 0,
                                                                                  hip.ptr(bits), W // 8, 1, p, hip.ptr(parts), s)),
                                     3 * B * W * e + 4 * B + B * W // 8)
        cases["norm_bwd_g_" + kind] = (lambda kid=kid: hip.check(lib.codae_norm_bwd(hip.ptr(y), 1, W, B, W, kid, hip.ptr(x), W, hip.ptr(r), hip.ptr(g),
                                                                                    hip.ptr(g), W, hip.ptr(bits), W // 8, 1, p, hip.ptr(parts), s)),
                                       3 * B * W * e + 8 * B * W + 4 * B + B * W // 8)
    cases.update({
        "residual_fwd": (lambda: hip.check(lib.codae_residual_fwd(hip.ptr(y), hip.ptr(x), 1, W, W, B, W, hip.ptr(bits), W // 8, s)),
                         3 * B * W * e + B * W // 8),
        "residual_bwd": (lambda: hip.check(lib.codae_residual_bwd(hip.ptr(y), 1, W, B, W, hip.ptr(g), hip.ptr(g), W, hip.ptr(bits), W // 8, None, 0,
                                                                  1, p, hip.ptr(parts), s)), 2 * B * W * e + 8 * B * W + B * W // 8),
        "dropout_fwd": (lambda: hip.check(lib.codae_dropout_fwd(hip.ptr(y), 1, W, B, W, None, 1, 1, 0.5, 7, s)), 2 * B * W * e),
        "dropout_bwd": (lambda: hip.check(lib.codae_dropout_bwd(hip.ptr(y), 1, W, B, W, None, 1, 1, 0.5, 7, hip.ptr(parts), s)), 2 * B * W * e),
    })
    for rnd in range(rounds):
        for name, (fn, nbytes) in cases.items():
            y.normal_(); g.normal_(); x.normal_(); r.fill_(1.0)      # (the in-place kernels would otherwise drive the values to inf / 0)
            us = time_launches(fn, reps)
            print(json.dumps({"what": "kernel", "round": rnd, "kernel": name, "rows": B, "width": W, "reps": reps, "us": round(us, 2),
                              "bytes": nbytes, "TB_per_s": round(nbytes / us * 1e-6, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--io", type=int, default=1536)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default=None, help="run the fused step of this one setting only (for a kernel trace), no stand-alone kernels")
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
    settings = [("off", None, None), ("layer", Norm("layer"), None), ("rms", Norm("rms"), None), ("skips", None, Residual("hidden")),
                ("layer+skips", Norm("layer"), Residual("hidden")), ("rms+skips", Norm("rms"), Residual("hidden"))]
    if args.only is not None:
        settings = [s for s in settings if s[0] == args.only]
        assert settings, "unknown setting %r" % args.only
    trainers = {}
    for name, norm, res in settings:
        tr = HipEmbeddingTrainer(enc + dec, data, table, mtu, 1e-5, 1e-4, 1.0, max_batch=B, precision="bf16", device=DEV, residual=res, norm=norm)
        tr.init_params(seed=0)
        for s in range(args.warmup):
            tr.train_batch(idx[s % 8], run=0)
        trainers[name] = tr
    torch.cuda.synchronize()
    for rnd in range(args.rounds):
        for name, _, _ in settings:
            tr = trainers[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(args.steps):
                tr.train_batch(idx[s % 8], run=0)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            print(json.dumps({"what": "fused_step", "round": rnd, "setting": name, "batch": B, "io": io, "layers": len(enc + dec),
                              "normalised": tr.engine.norm_layers, "skipped": tr.engine.residual_layers, "ms_per_step": round(ms, 4),
                              "loss": tr.engine.read_scalars()[3], "path": tr.engine.step_path(B)}), flush=True)
    if args.only is not None:
        return
    # the streaming class per step, in a pass of its own (an event pair costs 2-4 us of stream time): forward launches first (one per
    # skipped layer, one per normalised layer), then the backward ones - one per data-gradient site next to a skip or behind a norm
    n = 5
    for name in ("layer", "skips", "layer+skips"):
        tr = trainers[name]
        tr.engine.profile_begin(classes=("dropout",), max_records=64 * n)
        for s in range(n):
            tr.train_batch(idx[s % 8], run=0)
        us = [1e3 * v for v in tr.engine.profile_end().get("dropout", [])]
        per = len(us) // n
        n_fwd = len(tr.engine.residual_layers) + len(tr.engine.norm_layers)
        fwd = [v for i, v in enumerate(us) if i % per < n_fwd]
        bwd = [v for i, v in enumerate(us) if i % per >= n_fwd]
        print(json.dumps({"what": "in_step_launches", "setting": name, "per_step": per, "forward": n_fwd, "backward": per - n_fwd,
                          "fwd_us_median": round(float(np.median(fwd)), 2), "bwd_us_median": round(float(np.median(bwd)), 2)}), flush=True)
    kernels(B, io, args.reps, args.rounds)


if __name__ == "__main__":
    main()
