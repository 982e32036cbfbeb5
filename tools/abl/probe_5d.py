"""DESIGN.md section 5d probe: does the 64 x 64 fused-loss tile ever lose a contribution?

Repeats the SAME training forward (3 x 256, batch 4096: 768 workgroups of 64 x 64) on the library that is loaded and counts the
launches in which a workgroup's partial sum differs from the first launch (none, with the scalar-chain guard of gemm_bf16.hip)."""
import ctypes as C
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "mui-deepautoencoder_amd"))
import numpy as np
import torch
from codae import hip
from codae.train import HipEmbeddingTrainer
from oracle import dae_oracle as O

DEV = "cuda:0"
S, E, B = 3, 256, 4096
N_LAUNCH = int(sys.argv[1]) if len(sys.argv) > 1 else 300
io = S * E
rng = np.random.default_rng(77)
N = 2 * B
data = rng.random((N, io), dtype=np.float32)
sched = O.layer_schedule(io, io, 2, 2, False, "embedding")
params = O.init_params(sched, rng)
bm, _, _ = O.corrupter_tables([{"size": E, "position": s * E} for s in range(S)], 1)
mtu = rng.integers(0, S, (N, 1)).astype(np.int32)
idx = torch.tensor(rng.permutation(N)[:B], dtype=torch.int32, device=DEV)
tr = HipEmbeddingTrainer(sched, torch.tensor(data), torch.tensor(bm).to(torch.uint8), torch.tensor(mtu), 1e-3, 1e-4, 1.0,
                         max_batch=B, precision="bf16", device=DEV)
tr.load_params(params)
eng = tr.engine
lib = hip.lib()
batch = tr._batch(idx, 0)
hyper = eng.hyper(1e-3, 1e-4, 1.0, global_rows=B)

first_parts = None
bad_launches = 0
for i in range(N_LAUNCH):
    eng.zero_metric_sums()
    hip.check(lib.codae_step_forward_loss(eng._h, C.byref(eng.bufs), C.byref(batch), C.byref(hyper), None, hip.current_stream()))
    torch.cuda.synchronize()
    allp = eng.bias_parts.view(torch.float64).clone().cpu().numpy()
    if i == 0:
        first_parts = allp
        continue
    diff = np.nonzero((allp != first_parts) & ~(np.isnan(allp) & np.isnan(first_parts)))[0]
    if diff.size == 0:
        continue
    bad_launches += 1
    msg = "launch %d: %d doubles differ, first at %s: %r vs %r (delta %.6g)" % (
        i, diff.size, diff[:4].tolist(), allp[diff[0]], first_parts[diff[0]], allp[diff[0]] - first_parts[diff[0]])
    if bad_launches <= 8:
        print(msg, flush=True)
print("probe_5d: lib %s, %d launches, %d with a differing partial sum" % (os.path.basename(hip.LIB_PATH), N_LAUNCH, bad_launches))
