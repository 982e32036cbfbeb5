#!/usr/bin/env python3
"""Exhaustive accuracy of the Gaussian input noise's device arithmetic (csrc/gather.hip, box_muller_parts) against a
float64 evaluation of the same formulas (include/codae_hip.h, "Input noise").

Every one of the 2^24 values of u1 = (k + 1) 2^-24 goes through rho = sqrt(-2 ln u1), every one of the 2^24 values of
u2 = k 2^-24 through cos / sin(2 pi u2), on the GPU (codae_noise_box_muller; the float64 side is torch on the same device).

  e_rho   max |rho_device - rho_f64|
  e_trig  max(|cos_device - cos_f64|, |sin_device - sin_f64|)
  e_n     e_rho + rho_max e_trig, rho_max = sqrt(48 ln 2): the bound on the unit normal's absolute error; the condition the
          kernels are held to is e_n <= 1e-5 (the parity atol), so that a noised input with sigma <= 1 stays inside the
          parity tolerance of its definition.  Exit code 1 when it does not hold.

  python tools/noise_accuracy.py            one JSON line; the numbers are recorded in DESIGN.md section 6
"""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mui-deepautoencoder_amd")]

import torch  # noqa: E402

from codae import hip  # noqa: E402


def main():
    dev = "cuda:0"
    n = 1 << 24
    k = torch.arange(n, dtype=torch.int64, device=dev)
    w = k << 8                                 # the word whose top 24 bits are k ...
    words = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)      # ... as the int32 with the same bit pattern
    rho = torch.empty(n, dtype=torch.float32, device=dev)
    c = torch.empty_like(rho)
    s = torch.empty_like(rho)
    with torch.cuda.device(dev):
        hip.check(hip.lib().codae_noise_box_muller(hip.ptr(words), hip.ptr(words), hip.ptr(rho), hip.ptr(c), hip.ptr(s), n,
                                                   hip.current_stream()))
    torch.cuda.synchronize()
    kd = k.to(torch.float64)
    u1 = (kd + 1.0) * 2.0 ** -24
    rho64 = torch.sqrt(-2.0 * torch.log(u1))
    ang = (2.0 * math.pi) * (kd * 2.0 ** -24)
    d_rho = (rho.double() - rho64).abs()
    d_cos = (c.double() - torch.cos(ang)).abs()
    d_sin = (s.double() - torch.sin(ang)).abs()
    e_rho, e_trig = float(d_rho.max()), float(torch.maximum(d_cos, d_sin).max())
    rho_max = math.sqrt(48.0 * math.log(2.0))
    # where u1 is next to 1 rho is a square root of a tiny logarithm: report the relative error there too
    top = slice(n - 4096, n - 1)
    rel_top = float((d_rho[top] / rho64[top]).max())
    out = {"n_u1": n, "n_u2": n, "e_rho": e_rho, "argmax_u1_k": int(d_rho.argmax()), "rho_max_seen": float(rho.max()),
           "rho_max": rho_max, "e_rho_rel_last_4096_u1": rel_top, "e_cos": float(d_cos.max()), "e_sin": float(d_sin.max()),
           "e_trig": e_trig, "e_n": e_rho + rho_max * e_trig, "bound": 1e-5}
    out["ok"] = bool(out["e_n"] <= out["bound"] and math.isfinite(out["e_n"]))
    print(json.dumps(out), flush=True)
    return 0 if out["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
