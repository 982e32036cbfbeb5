#!/usr/bin/env python3
"""Cost of a checkpoint on the fused training step (include/codae_hip.h, "State digest"; HipEmbeddingTrainer.snapshot), at BASELINE's
C3 shape (10 x Linear(1536, 1536), 3 slots of 512, batch 8192, bf16, EMA on: four state tensors of 94 MB and the scalars), in one
process on one device.

  python tools/bench_snapshot.py [--steps K] [--warmup W] [--rounds N] [--dir D]      JSON lines

kernel:      codae_state_digest on one parameter-sized tensor, digest only and digest + copy, us per call and the bytes it moves per
             second; beside it, per step, the engine's own event pairs around the update class (the flat update: the project's
             memory-bound reference kernel, 40 bytes per parameter with the EMA on) on the same device.
snapshot:    what one snapshot() puts on the training stream (an event pair around the call), and how long the call holds the host.
stall:       wall time of K steps; of K steps with one snapshot() in the middle (the device-to-host copies run beside the steps that
             follow; write() comes after the loop and is timed by itself: the wait for the copies and the file); of K steps with the
             blocking alternative in the middle - .cpu() of the same tensors.  The three alternate inside every round.
DESIGN.md section 6 holds the numbers."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mui-deepautoencoder_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from codae.tool import WeightAverage  # noqa: E402
from codae.train import HipEmbeddingTrainer  # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the checkpoint files go (default: a temporary directory)")
    args = ap.parse_args()
    io, L, B, S = 1536, 10, 8192, 3
    rng = np.random.default_rng(1234)
    n_rows = 2 * B
    data = torch.from_numpy(rng.random((n_rows, io), dtype=np.float32)).to(DEV)
    table = torch.ones((S, io), dtype=torch.uint8, device=DEV)
    for c in range(S):
        table[c, c * (io // S):(c + 1) * (io // S)] = 0
    mtu = torch.from_numpy(rng.integers(0, S, (n_rows, 1)).astype(np.int32)).to(DEV)
    idx = [torch.tensor(rng.permutation(n_rows)[:B], dtype=torch.int32, device=DEV) for _ in range(8)]
    sched = [(io, io, l + 1 < L and l != L // 2 - 1) for l in range(L)]
    tr = HipEmbeddingTrainer(sched, data, table, mtu, 1e-5, 1e-4, 1.0, max_batch=B, precision="bf16", device=DEV, n_slots=S,
                             weight_average=WeightAverage("ema", decay=0.999))
    tr.init_params(seed=0)
    eng = tr.engine

    def steps(n, s0=0):
        for s in range(n):
            tr.train_batch(idx[(s0 + s) % 8], run=0)

    steps(args.warmup)
    tr.snapshot().release()                 # (allocates the staging set and the pinned buffers)
    torch.cuda.synchronize()
    state = eng.state_tensors()
    state_bytes = sum(t.numel() * t.element_size() for t in state.values())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    # ---- the kernel alone, and the flat update beside it -------------------------------------------------------------------
    src, dst, out = eng._params, torch.empty_like(eng._params), torch.empty(2, dtype=torch.int64, device=DEV)
    n_bytes = src.numel() * 4
    for rnd in range(args.rounds):
        for what, d, moved in (("digest", None, n_bytes), ("digest+copy", dst, 2 * n_bytes)):
            for _ in range(3):
                eng.digest_into(src, out, dst=d)
            e0.record()
            for _ in range(20):
                eng.digest_into(src, out, dst=d)
            e1.record()
            torch.cuda.synchronize()
            us = 1e3 * e0.elapsed_time(e1) / 20
            print(json.dumps({"what": "kernel", "round": rnd, "kernel": what, "tensor_bytes": n_bytes, "us": round(us, 2),
                              "moved_TB_per_s": round(moved / us / 1e6, 3)}), flush=True)
        eng.profile_begin(classes=("adam",), max_records=4 * args.steps)
        steps(args.steps)
        rec = eng.profile_end().get("adam", [])
        us = 1e3 * float(np.sum(rec)) / args.steps
        print(json.dumps({"what": "kernel", "round": rnd, "kernel": "flat update (adam + ema + shadows)", "us_per_step": round(us, 2),
                          "records_per_step": len(rec) / args.steps,
                          "moved_TB_per_s": round(40.0 * eng.n_param / us / 1e6, 3)}), flush=True)

    # ---- what a snapshot puts on the training stream ------------------------------------------------------------------------
    for rnd in range(args.rounds):
        steps(4)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        snap = tr.snapshot()
        e1.record()
        host_us = (time.perf_counter() - t0) * 1e6
        torch.cuda.synchronize()
        snap.release()
        print(json.dumps({"what": "snapshot", "round": rnd, "state_bytes": state_bytes, "tensors": len(state),
                          "stream_us": round(1e3 * e0.elapsed_time(e1), 2), "host_call_us": round(host_us, 1)}), flush=True)

    # ---- the step loop's stall: snapshot() now and write() later, against a blocking .cpu() ----------------------------------
    out_dir = args.dir or tempfile.mkdtemp(prefix="codae_snapshot_")
    half = args.steps // 2

    def loop(kind):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps(half)
        snap = host = None
        if kind == "snapshot":
            snap = tr.snapshot()
        elif kind == "cpu":
            host = {n: t.cpu() for n, t in eng.state_tensors().items()}
        steps(args.steps - half, half)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, snap, host

    for rnd in range(args.rounds):
        base = None
        for kind in ("plain", "snapshot", "cpu"):
            ms, snap, host = loop(kind)
            row = {"what": "stall", "round": rnd, "kind": kind, "steps": args.steps, "loop_ms": round(ms, 3)}
            if kind == "plain":
                base = ms
            else:
                row["stall_ms"] = round(ms - base, 3)
            if snap is not None:
                t0 = time.perf_counter()
                snap.wait()
                t1 = time.perf_counter()
                path = os.path.join(out_dir, "bench_snapshot.npz")
                row["file_bytes"] = snap.write(path)
                row["write_wait_ms"], row["write_file_ms"] = round((t1 - t0) * 1e3, 3), round((time.perf_counter() - t1) * 1e3, 1)
                os.remove(path)
            del host
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
