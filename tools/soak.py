"""Soak / race check at the full C3 size: N optimizer steps of the fused bf16 step, no host sync inside the loop, several times
over from the same seeds.  The default step (round 3: one stream, grouped unsplit weight gradients, 1-bit ReLU masks, weights
touched under the previous epilogue) must end on the SAME BITS every time - parameters, both Adam moments, the loss at every
50th step - and with the 1-bit masks off (CODAE_NO_RELU_BITS=1) or any output store policy forced (CODAE_STORE_POLICY) or the loss finish as a launch of its own (CODAE_NO_FOLDED_LOSS_FINISH=1); the per-layer two-stream backward (CODAE_NO_DEFER_WGRAD=1) and
the single-stream form of it sum the weight gradients in another order (split-K slabs): bit-identical to EACH OTHER, their loss
curve drifts from the default one like any two bf16 runs whose gradients differ in the last bit (5e-3 bound; measured 2e-3 after 400
steps, 1e-6 over the first 100).
Usage: python tools/soak.py [steps]"""
import os, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "mui-deepautoencoder_amd"))
import numpy as np, torch
import bench
from codae.train import HipEmbeddingTrainer
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 300
S, E, B = 3, 512, 8192
io = S * E
sched = bench.square_schedule(io, 4, 4)
data, blank = bench.make_inputs(4 * B, io, S)
dev = torch.device("cuda:0")
table = np.ones((S, io), dtype=np.uint8)
for s in range(S): table[s, s * E:(s + 1) * E] = 0
rng = np.random.default_rng(3)
order = [torch.tensor(rng.permutation(4 * B)[:B], dtype=torch.int32, device=dev) for _ in range(steps)]
VARS = ("CODAE_SINGLE_STREAM", "CODAE_NO_DEFER_WGRAD", "CODAE_NO_RELU_BITS", "CODAE_NO_PREFETCH", "CODAE_STORE_POLICY", "CODAE_NO_FOLDED_LOSS_FINISH")


def run(env):
    for v in VARS: os.environ.pop(v, None)
    os.environ.update(env)
    tr = HipEmbeddingTrainer(sched, torch.tensor(data), torch.tensor(table), torch.tensor(blank.reshape(-1, 1)), 1e-4, 1e-4, 1.0,
                             max_batch=B, precision="bf16", device=str(dev))
    tr.init_params(0)
    ls = []
    for s in range(steps):
        tr.train_batch(order[s], run=0)
        if s % 50 == 49: ls.append(tr.engine.read_scalars()[3])
    eng = tr.engine
    out = (ls, eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone())
    del tr
    return out


ref = run({})
print("default       ", " ".join("%.7f" % v for v in ref[0]))
ok = True
per_layer = None
for name, env, exact in (("default again", {}, True), ("default #3", {}, True), ("no 1-bit masks", {"CODAE_NO_RELU_BITS": "1"}, True),
                         ("no prefetch", {"CODAE_NO_PREFETCH": "1"}, True),
                         ("plain stores", {"CODAE_STORE_POLICY": "plain"}, True), ("sc1 stores", {"CODAE_STORE_POLICY": "wt"}, True),
                         ("own loss finish", {"CODAE_NO_FOLDED_LOSS_FINISH": "1"}, True),
                         ("per-layer bwd ", {"CODAE_NO_DEFER_WGRAD": "1"}, False), ("single stream ", {"CODAE_NO_DEFER_WGRAD": "1", "CODAE_SINGLE_STREAM": "1"}, False)):
    got = run(env)
    same = got[0] == ref[0] and all(torch.equal(a, b) for a, b in zip(got[1:], ref[1:]))
    rel = max(abs(a - b) / abs(a) for a, b in zip(got[0], ref[0]))
    print("%-14s" % name, " ".join("%.7f" % v for v in got[0]), "| bit-identical to the default run: %s, max relative loss difference %.2e" % (same, rel))
    ok = ok and (same if exact else rel <= 5e-3)
    if not exact:
        if per_layer is None:
            per_layer = got
        else:
            same_pl = got[0] == per_layer[0] and all(torch.equal(a, b) for a, b in zip(got[1:], per_layer[1:]))
            print("single-stream per-layer backward bit-identical to the two-stream one: %s" % same_pl)
            ok = ok and same_pl
print("SOAK", "OK" if ok else "FAILED")
sys.exit(0 if ok else 1)
