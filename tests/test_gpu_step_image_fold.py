"""The fused bf16 step with the gather reading the dataset's bf16 image (codae_set_dataset_image) and with the bias finish riding
in the pipelined grouped weight-gradient launch (BiasFold, gemm_bf16_pipe.hip), against the step without either: both are
reorganisations that must change no bit - the image holds what the gather would have rounded, the trailing workgroups add the
rows, the block sums and the loss sums in bias_finish_kernel's order.

Shape: the smallest that takes the pipelined grouped launch - 3 x 512 wide, five square layers (5 x 48 = 240 tiles of 256 x 192,
200 needed), 72 rows (one 64-row pad block past the first).  15 trailing workgroups then finish 7680 bias columns (30 blocks of
256) and a 16th the loss.  max_grad_norm is far below the gradient's norm, so the clip coefficient - every norm slot the
trailing workgroups add to - reaches every parameter.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
S, E, L, B = 3, 512, 5, 72
IO = S * E
LR, WD, CLIP = 1e-3, 1e-4, 1e-3
SWITCHES = ("CODAE_NO_DATASET_IMAGE", "CODAE_NO_FOLDED_BIAS_FINISH")


@pytest.fixture(scope="module")
def hip():
    from codae import hip as H
    H.lib()
    return H


@pytest.fixture(scope="module")
def problem():
    import bench
    from oracle import dae_oracle as O
    rng = np.random.default_rng(512)
    N = 2 * B
    sched = bench.square_schedule(IO, (L - 1) // 2, (L - 2) // 2)
    assert len(sched) == L
    bm, _, _ = O.corrupter_tables([{"size": E, "position": s * E} for s in range(S)], 1)
    return dict(sched=sched, data=rng.standard_normal((N, IO)).astype(np.float32), bm=bm,
                mtu=np.stack([rng.permutation(S) for _ in range(N)]).astype(np.int32),
                idx=[torch.tensor(rng.permutation(N)[:B], dtype=torch.int32, device=DEV) for _ in range(3)])


def _run(hip, p, image, fold, noise=None, other_data=None, steps=3):
    """three training steps and one evaluation step under the two switches -> everything the step leaves behind"""
    from codae.train import HipEmbeddingTrainer
    saved = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k, on in zip(SWITCHES, (image, fold)):
            if on:
                os.environ.pop(k, None)
            else:
                os.environ[k] = "1"
        hip.check(hip.lib().codae_reload_env())
        tr = HipEmbeddingTrainer(p["sched"], torch.tensor(p["data"]), torch.tensor(p["bm"]).to(torch.uint8), torch.tensor(p["mtu"]), LR, WD, CLIP,
                                 max_batch=B, precision="bf16", device=DEV, input_noise=noise)
        assert (tr.engine._dataset_image is not None) == image
        assert tr.engine.step_path(B) == "layers"
        tr.init_params(seed=3)
        if other_data is not None:
            tr.data = torch.tensor(other_data, device=DEV)         # batches now name a tensor the image was not registered with
        out = []
        for st in range(steps):
            tr.train_batch(p["idx"][st], run=st % S)
            out.append(tr.engine.read_scalars())
        tr.engine.zero_metric_sums()
        tr.eval_batch(p["idx"][0], run=0)
        out.append(tr.engine.read_scalars()[:2])
        torch.cuda.synchronize()
        return out, tr.engine.params.clone(), tr.engine.grads.clone()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        hip.check(hip.lib().codae_reload_env())


def _assert_same(a, b):
    (sa, pa, ga), (sb, pb, gb) = a, b
    assert sa == sb, (sa, sb)                                    # metric sums, sum g^2, loss of every step; the evaluation's sums
    assert torch.equal(ga.view(torch.int32), gb.view(torch.int32)), "gradients"
    assert torch.equal(pa.view(torch.int32), pb.view(torch.int32)), "parameters"


@pytest.fixture(scope="module")
def parent_form(hip, problem):
    """fp32 gather, bias finish as a launch of its own: what every other form must reproduce; computed once, never modified"""
    out = _run(hip, problem, image=False, fold=False)
    scalars, params, grads = out
    sq, sqp, gsq, loss = scalars[0]
    assert loss > 0 and gsq ** 0.5 > 10 * CLIP, (loss, gsq)      # clipping is active: the norm reaches every parameter
    nw = 5 * IO * IO
    assert float(grads[nw:].abs().max()) > 0                     # bias gradients were written
    return out


@pytest.mark.parametrize("image,fold", [(True, True), (True, False), (False, True)], ids=["image+fold", "image", "fold"])
def test_image_and_folded_bias_finish_change_no_bit(hip, problem, parent_form, image, fold):
    _assert_same(parent_form, _run(hip, problem, image=image, fold=fold))


def test_the_folded_finish_is_recorded_as_riding_in_the_weight_gradient_launch(hip, problem):
    """the launch profiler's records of one step: without the fold a bias_finish launch with a time of its own; with it the class is
    still listed where it was issued, with exactly 0 ms - its work is inside the gemm_wgrad launch in front of it"""
    from codae.train import HipEmbeddingTrainer
    counts = {}
    for fold in (True, False):
        saved = os.environ.get(SWITCHES[1])
        try:
            if fold:
                os.environ.pop(SWITCHES[1], None)
            else:
                os.environ[SWITCHES[1]] = "1"
            hip.check(hip.lib().codae_reload_env())
            tr = HipEmbeddingTrainer(problem["sched"], torch.tensor(problem["data"]), torch.tensor(problem["bm"]).to(torch.uint8),
                                     torch.tensor(problem["mtu"]), LR, WD, CLIP, max_batch=B, precision="bf16", device=DEV)
            tr.init_params(seed=3)
            tr.train_batch(problem["idx"][0], run=0)
            tr.engine.profile_begin(classes=("gemm_wgrad", "bias_finish"))
            tr.train_batch(problem["idx"][1], run=0)
            prof = tr.engine.profile_end()
            torch.cuda.synchronize()
            counts[fold] = prof
        finally:
            if saved is None:
                os.environ.pop(SWITCHES[1], None)
            else:
                os.environ[SWITCHES[1]] = saved
            hip.check(hip.lib().codae_reload_env())
    for fold in (True, False):
        assert len(counts[fold]["gemm_wgrad"]) == L and len(counts[fold]["bias_finish"]) == 1, counts
        assert all(ms > 0 for ms in counts[fold]["gemm_wgrad"]), counts
    assert counts[False]["bias_finish"][0] > 0 and counts[True]["bias_finish"][0] == 0.0, counts


def test_input_noise_ignores_the_image(hip, problem):
    """Gaussian noise is added in fp32 in front of the rounding: a noised step keeps the fp32 gather, image registered or not"""
    from codae.tool import InputNoise
    noise = InputNoise("gaussian", sigma=0.3, seed=11)
    with_image = _run(hip, problem, image=True, fold=True, noise=noise, steps=2)
    _assert_same(_run(hip, problem, image=False, fold=True, noise=noise, steps=2), with_image)
    clean = _run(hip, problem, image=True, fold=True, steps=2)
    assert with_image[0][0] != clean[0][0]                       # (the noise was really on)


def test_a_batch_of_another_tensor_takes_the_fp32_gather(hip, problem):
    """the image belongs to the tensor it was registered with: batches that name another one - here the same rows times 1.5 - are
    gathered from THEIR data, as without an image"""
    other = (problem["data"] * 1.5).astype(np.float32)
    with_image = _run(hip, problem, image=True, fold=True, other_data=other, steps=2)
    _assert_same(_run(hip, problem, image=False, fold=True, other_data=other, steps=2), with_image)
    assert with_image[0][0] != _run(hip, problem, image=True, fold=True, steps=2)[0][0]
