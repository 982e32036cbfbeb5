#!/usr/bin/env python3
"""How the SEEDS table of tests/test_gpu_slot_contrast.py was filled: for every (io, K) of its CASES, the first seed from
0x5EED0000C0DA0001 under which both row sets of the B = 33 fixture (the permuted rows and rows 0 .. 32) meet the fixture conditions
that depend on the draw - a pair with a candidate left out, a pair with none left out, a row among its own candidates.  CPU only.

  python tools/find_contrast_seeds.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mui-deepautoencoder_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import contrast_ref as CR  # noqa: E402
import test_gpu_slot_contrast as T  # noqa: E402


def find_seed(io, K, ids_on, pool_on, start):
    p = T._problem_host(io)
    for seed in range(start, start + 100000):
        ok = True
        for rows in (p["rows"], np.arange(p["B"])):
            cand = np.stack([CR.candidate_rows(T.STEP, s, K, seed, 120, p["pool"] if pool_on else None) for s in range(T.S)])
            if ids_on:
                left = np.stack([p["ids"][s][cand[s]][None, :] == p["ids"][s][rows][:, None] for s in range(T.S)], axis=1)
            else:
                left = np.stack([cand[s][None, :] == rows[:, None] for s in range(T.S)], axis=1)
            per_pair = left.any(axis=2)
            own = (cand[None] == rows[:, None, None]).any(axis=(1, 2))
            ok = ok and per_pair.any() and (~per_pair).any() and own.any()
        if ok:
            return seed
    raise SystemExit("no seed for %r" % ((io, K),))


if __name__ == "__main__":
    for (io, K), (tau, emph_on, ids_on, pool_on, pad) in sorted(T.CASES.items()):
        print("    (%d, %d): 0x%X," % (io, K, find_seed(io, K, ids_on, pool_on, 0x5EED0000C0DA0001)))
