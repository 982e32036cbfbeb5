"""The counts the engine adds up agree with what the bf16 GEMM kernels write, on a real MI355X.

A data-gradient launch writes one partial column-sum row per tile along the batch, the fused-loss launch one pair of metric sums
per workgroup; the bias finish and the loss finish add up as many as gemm_bf16_plan (csrc/gemm_bf16.hip) says the launch has.
If the two disagree the result is a silently wrong bias gradient or loss, so this file checks both END results, for every tile
the data gradient and the fused loss can take - 64 x 64, 128 x 192, 256 x 192 by batch size - and under the switches that force
a tile (CODAE_GEMM_TILE=m: the commit before gemm_bf16_plan counted one row per 256 batch rows there while the 128 x 192 kernel
wrote one per 128; tests/test_gemm_plan_host.py pins the same on the host).

Everything is integer-valued and small enough to be exact in bf16 (integers up to 256) and in fp32 sums (below 2^24) in any
order, so the bias gradients are compared for EQUALITY with a float64 evaluation: x in {0, 1}; weights and dy in {-1, 0, 1} with
at most 254 non-zeros per row and column of a weight matrix, so that every hidden pre-activation (+ a bias in [-2, 2]) and every
element of the data gradient is an integer of at most 256 in magnitude; a column sum over at most 6912 rows stays below 2^21.
The loss is compared at the relative tolerance tests/test_gpu_parity.py uses for the bf16 first-step loss (1e-6): the engine
rounds nothing on the way to y here, and adds the squares up in fp32 per workgroup, then in double.
"""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
IO = 1024
SCHEDULE = [(IO, IO, True), (IO, IO, False)]
BF16_FIRST_STEP_LOSS_RTOL = 1e-6          # tests/test_gpu_parity.py: the bf16 engine's first-step loss against its rounding oracle


@pytest.fixture
def env_toggle():
    """Sets CODAE_* variables (before the engine is created: codae_create snapshots them); restores them afterwards."""
    from codae import hip
    saved = {}

    def set_(name, value):
        saved.setdefault(name, os.environ.get(name))
        os.environ[name] = value
        hip.lib().codae_reload_env()
    yield set_
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    hip.lib().codae_reload_env()


@functools.lru_cache(maxsize=None)
def stack():
    """[(W0, b0), (W1, b1)] as float64 tensors on the device: entries of W in {-1, 0, 1} at density 1/8, biases in [-2, 2]."""
    g = torch.Generator().manual_seed(1024)
    params = []
    for _ in SCHEDULE:
        W = (torch.randint(0, 8, (IO, IO), generator=g) == 0).to(torch.float64) * (torch.randint(0, 2, (IO, IO), generator=g) * 2 - 1)
        b = torch.randint(-2, 3, (IO,), generator=g).to(torch.float64)
        nnz = max(int((W != 0).sum(0).max()), int((W != 0).sum(1).max()))
        assert nnz <= 254, nnz                      # |x W^T + b| and |dy W| stay <= 256: exact in bf16
        params.append((W.to(DEV), b.to(DEV)))
    return params


@functools.lru_cache(maxsize=None)
def batch_data(B):
    """x in {0, 1} [B][IO] and dy in {-1, 0, 1} [B][IO], float64 on the device."""
    g = torch.Generator().manual_seed(B)
    x = torch.randint(0, 2, (B, IO), generator=g).to(torch.float64)
    dy = (torch.randint(0, 3, (B, IO), generator=g) - 1).to(torch.float64)
    return x.to(DEV), dy.to(DEV)


def check_bias_gradients(B):
    from codae.hip.engine import DaeEngine
    (W0, b0), (W1, b1) = stack()
    x, dy = batch_data(B)
    eng = DaeEngine(SCHEDULE, B, "bf16", DEV, with_optimizer_state=False)
    eng.load_params([(W0.float(), b0.float()), (W1.float(), b1.float())])
    eng.forward(x.float())
    eng.backward(dy.float(), need_dx=False)
    got0, got1 = eng.bias_grad(0).double(), eng.bias_grad(1).double()
    torch.cuda.synchronize()
    dh = dy @ W1
    assert float(dh.abs().max()) <= 256
    want0 = (dh * ((x @ W0.T + b0) > 0)).sum(0)
    want1 = dy.sum(0)
    bad0, bad1 = int((got0 != want0).sum()), int((got1 != want1).sum())
    print("MEASURE bias gradients at batch %d: %d / %d of %d columns differ; layer 0 sums got %.0f want %.0f" %
          (B, bad0, bad1, IO, float(got0.abs().sum()), float(want0.abs().sum())))
    assert float(want0.abs().sum()) > 0 and float(want1.abs().sum()) > 0
    assert torch.equal(got0, want0), (B, bad0)
    assert torch.equal(got1, want1), (B, bad1)


# 96 rows (128 padded): the data gradient on 64 x 64 tiles; 3328: 208 tiles of 128 x 128 > 200, 78 of 256 x 192 < 160: 128 x 192;
# 6912: 27 x 6 = 162 tiles of 256 x 192
@pytest.mark.parametrize("B", [96, 3328, 6912])
def test_bias_gradients_add_up_every_partial_row(B):
    check_bias_gradients(B)


@pytest.mark.parametrize("tile", ["m", "x"])
def test_bias_gradients_under_a_forced_tile(tile, env_toggle):
    """256 rows on the forced 128 x 192 tile (two partial rows; the instantiation is forward-form only, so the fp32 output
    layer and the grouped weight gradients keep their own tiles) and on the forced 256 x 192 tile (one row)."""
    env_toggle("CODAE_GEMM_TILE", tile)
    check_bias_gradients(256)


# 96 rows: the fused loss on 64 x 64 tiles (2 x 16 workgroups); 6912: 27 x 6 = 162 tiles of 256 x 192
@pytest.mark.parametrize("B", [96, 6912])
def test_fused_loss_adds_up_every_workgroup(B):
    from codae.train import HipEmbeddingTrainer
    from oracle import dae_oracle as O
    (W0, b0), (W1, b1) = stack()
    x, _ = batch_data(B)
    S, E = 4, IO // 4
    bm, _, _ = O.corrupter_tables([{"size": E, "position": s * E} for s in range(S)], 1)
    rng = np.random.default_rng(B)
    mtu = np.stack([rng.permutation(S) for _ in range(B)]).astype(np.int32)
    tr = HipEmbeddingTrainer(SCHEDULE, x.float().cpu(), torch.tensor(bm).to(torch.uint8), torch.tensor(mtu), 1e-3, 1e-4, 1.0,
                             max_batch=B, precision="bf16", device=DEV)
    tr.load_params([(W0.float().cpu().numpy(), b0.float().cpu().numpy()), (W1.float().cpu().numpy(), b1.float().cpu().numpy())])
    assert tr.engine.step_path(B) == "layers"
    idx = torch.arange(B, dtype=torch.int32, device=DEV)
    tr.train_batch(idx, run=0)
    _, _, _, loss = tr.engine.read_scalars()
    fmask = torch.tensor(bm[mtu[:, 0]], dtype=torch.float64, device=DEV)          # the slot mask of run 0, row by row
    h = torch.clamp((x * fmask) @ W0.T + b0, min=0)
    assert float(h.max()) <= 256
    want = float(((x - (h @ W1.T + b1)) ** 2).mean())
    print("MEASURE fused loss at batch %d: got %.9g want %.9g rel %.3g" % (B, loss, want, abs(loss - want) / want))
    assert abs(loss - want) <= BF16_FIRST_STEP_LOSS_RTOL * want, (B, loss, want)
