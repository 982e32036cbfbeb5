"""Swap noise on a real MI355X: the swap instantiations of the gather kernels (codae_corrupt_batch_swap, fp32 rows and bf16 image)
against the plain-Python loop of tests/swap_ref.py, bit for bit; the fused step against the oracle fed the reference-swapped input
and the clean target; the emphasised loss and two criteria against float64; and the step forms (graph replay, forward with a hyper,
shards, chain fall-back, evaluation, refusals).

Tolerances.  Inputs: none - a swap moves values and computes nothing.  Fused steps: the bounds of tests/test_gpu_noise.py's MASKING
cases, which carry over because the inputs are bit-identical on both sides.  Emphasised loss / criteria: the bounds
tests/test_gpu_emphasis.py and tests/test_gpu_recon_loss.py derive (fp32 dY rtol 1e-6; slot_cosine (E + 8) 2^-23 k (|x_c| / (nx ny)
+ |y_c| / |y|^2); the loss relative B io 2^-24, plus E (E + 8) 2^-24 sum W for the cosines).
"""
import ctypes as C
import math

import numpy as np
import pytest

import swap_ref as R
from golden_util import Golden, close, max_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
N = R.N_ROWS


def _noise(p, pool=None, seed=R.SEED):
    from codae.tool import InputNoise
    return InputNoise("swap", p=p, seed=seed, pool=pool)


def _bits(t):
    return t.contiguous().view({torch.bfloat16: torch.int16, torch.float32: torch.int32}[t.dtype])


def corrupt_swap(src, noise, step, S, n_rows, row_idx=None, mask_id=None, table=None, out_bf16=False, out_ld=None, noise_rows=None,
                 dataset=None, present=None, image=False):
    """codae_corrupt_batch_swap on device tensors -> the [B, out_ld] output (allocated zeroed)."""
    from codae import hip
    io = int(src.shape[1])
    B = int(row_idx.numel()) if row_idx is not None else int(src.shape[0])
    ld = io if out_ld is None else out_ld
    out = torch.zeros((B, ld), dtype=torch.bfloat16 if out_bf16 else torch.float32, device=DEV)
    batch = hip.Batch(hip.ptr(src), hip.ptr(row_idx), hip.ptr(mask_id), hip.ptr(table), B, io, None, 0, 0)
    st = noise.as_struct()
    pool = None if noise.pool is None else torch.tensor(noise.pool.astype(np.int32), device=DEV)
    sw = hip.Swap(hip.ptr(pool), n_rows if pool is None else int(pool.numel()), S)
    hip.check(hip.lib().codae_corrupt_batch_swap(C.byref(batch), C.byref(st), step, hip.ptr(noise_rows), hip.ptr(dataset), C.byref(sw),
                                                 hip.ptr(out), int(out_bf16), ld, hip.ptr(present), int(image), hip.current_stream()))
    torch.cuda.synchronize()
    return out


_PROBLEMS = {}


def problem(io, S):
    """The draw fixture (64 rows, a pool of 8, a quarter of the slots absent) with data of this width, a batch order that is a
    permutation of the rows, and one blanked slot per row (mask id = row % S); shared by the cases of one shape."""
    if (io, S) not in _PROBLEMS:
        fx = R.fixture(S)
        rng = np.random.default_rng(100 * io + S)
        E = io // S
        table = np.ones((S, io), dtype=np.uint8)
        for s in range(S):
            table[s, s * E:(s + 1) * E] = 0
        rows = rng.permutation(N).astype(np.int32)
        _PROBLEMS[(io, S)] = dict(fx, io=io, E=E, data=rng.standard_normal((N, io)).astype(np.float32), table=table, order=rows,
                                  mask_id=(rows % S).astype(np.int32))
    return _PROBLEMS[(io, S)]


SHAPES = [(48, 3, True, None), (72, 3, True, 128), (24, 2, True, None), (12, 2, False, None), (44, 11, False, None), (9, 3, False, None)]


@pytest.mark.parametrize("io,S,out_bf16,out_ld", SHAPES,
                         ids=["x8-io48", "x8-io72-ld128", "x8-io24-E12-straddles", "x4-io12-E6-straddles", "x4-io44-E4", "scalar-io9"])
def test_corrupt_batch_swap_matches_the_definition(io, S, out_bf16, out_ld):
    p = problem(io, S)
    rows, data = p["order"], p["data"]
    data_t = torch.tensor(data, device=DEV)
    rows_t = torch.tensor(rows, device=DEV)
    gathered_t = torch.tensor(data[rows], device=DEV)
    table_t, mid_t = torch.tensor(p["table"], device=DEV), torch.tensor(p["mask_id"], device=DEV)
    pres_t = torch.tensor(p["present"].astype(np.uint8), device=DEV)
    keep = p["table"][p["mask_id"]]
    for step in (1, 2):
        cls, _ = R.classify(rows, step, S, p["p"], R.SEED, N, p["pool"], p["present"])
        R.assert_all_classes(cls)                                              # not hit, self, presence, accepted: all occur
        for pool in (p["pool"], None):
            noise = _noise(p["p"], pool)
            for pres in (p["present"], None):
                for mask in (keep, None):
                    ref, c = R.corrupt(data[rows], data, rows, step, S, p["p"], R.SEED, pool, pres, mask)
                    assert (c == 3).any() and not np.array_equal(ref, data[rows] if mask is None else data[rows] * mask)
                    want = torch.tensor(ref).to(torch.bfloat16 if out_bf16 else torch.float32)
                    kw = dict(out_bf16=out_bf16, out_ld=out_ld, present=None if pres is None else pres_t,
                              mask_id=None if mask is None else mid_t, table=None if mask is None else table_t)
                    # through row_idx, and on a batch the caller gathered (noise_rows + the dataset)
                    a = corrupt_swap(data_t, noise, step, S, N, row_idx=rows_t, **kw)
                    b = corrupt_swap(gathered_t, noise, step, S, N, noise_rows=rows_t, dataset=data_t, **kw)
                    for got in (a, b):
                        assert torch.equal(_bits(got[:, :io].cpu()), _bits(want)), (step, pool is None, pres is None, mask is None)
                        if out_ld is not None:
                            assert (got[:, io:] == 0).all()                    # pad columns stay zero


@pytest.mark.parametrize("out_bf16", [False, True], ids=["f32", "bf16"])
def test_absent_nan_never_reaches_the_output_and_a_blanked_swapped_slot_is_plus_zero(out_bf16):
    io, S = 48, 3
    p = problem(io, S)
    rows, E = p["order"], p["E"]
    data = p["data"].copy()
    for r in range(N):
        for s in range(S):
            if not p["present"][r, s]:
                data[r, s * E:(s + 1) * E] = np.nan                           # what an absent slot holds is never used
    data = -np.abs(data)                                                       # every present value negative: a cleared one must be +0, not -0
    noise = _noise(p["p"], p["pool"])
    keep = p["table"][p["mask_id"]]
    ref, cls = R.corrupt(data[rows], data, rows, 1, S, p["p"], R.SEED, p["pool"], p["present"], keep)
    R.assert_all_classes(cls)
    blanked_and_swapped = [(b, s) for b in range(N) for s in range(S) if cls[b, s] == 3 and p["mask_id"][b] == s]
    assert blanked_and_swapped and not np.isnan(ref).any()
    got = corrupt_swap(torch.tensor(data, device=DEV), noise, 1, S, N, row_idx=torch.tensor(rows, device=DEV),
                       mask_id=torch.tensor(p["mask_id"], device=DEV), table=torch.tensor(p["table"], device=DEV), out_bf16=out_bf16,
                       present=torch.tensor(p["present"].astype(np.uint8), device=DEV)).cpu()
    assert not torch.isnan(got.float()).any()
    assert torch.equal(_bits(got), _bits(torch.tensor(ref).to(got.dtype)))
    for b, s in blanked_and_swapped:
        assert (_bits(got[b, s * E:(s + 1) * E]) == 0).all()                   # exactly +0
    absent = np.repeat(~p["present"][rows], E, axis=1)
    assert (_bits(got)[torch.tensor(absent)] == 0).all()


@pytest.mark.parametrize("io,S", [(48, 3), (24, 2)], ids=["io48", "io24-E12-straddles"])
def test_image_route_equals_fp32_route(io, S):
    """The launcher on the bf16 image against the launcher on the fp32 rows, and a bf16 engine's layer-0 input with the image
    registered against the same engine without it: the same bits, and those of the reference."""
    from codae.tool import SlotPresence
    from codae.train import HipEmbeddingTrainer
    from oracle import dae_oracle as O
    p = problem(io, S)
    rows, E = p["order"], p["E"]
    data_t = torch.tensor(p["data"], device=DEV)
    image_t = data_t.to(torch.bfloat16)
    rows_t = torch.tensor(rows, device=DEV)
    pres_t = torch.tensor(p["present"].astype(np.uint8), device=DEV)
    noise = _noise(p["p"], p["pool"])
    keep = p["table"][p["mask_id"]]
    kw = dict(row_idx=rows_t, mask_id=torch.tensor(p["mask_id"], device=DEV), table=torch.tensor(p["table"], device=DEV), out_bf16=True)
    for pres, pt in ((p["present"], pres_t), (None, None)):
        ref, cls = R.corrupt(p["data"][rows], p["data"], rows, 2, S, p["p"], R.SEED, p["pool"], pres, keep)
        if pres is not None:
            R.assert_all_classes(cls)
        a = corrupt_swap(data_t, noise, 2, S, N, present=pt, **kw)
        b = corrupt_swap(image_t, noise, 2, S, N, present=pt, image=True, **kw)
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a.cpu()), _bits(torch.tensor(ref).to(torch.bfloat16)))
    # the engine: io -> 8 -> io in bf16, masks read through mask_to_use, the trainer's own presence table
    bm, _, _ = O.corrupter_tables([{"size": E, "position": s * E} for s in range(S)], 1)
    assert np.array_equal(bm[:S], p["table"])
    mtu = (np.arange(N) % S).astype(np.int32).reshape(N, 1)
    sched = [(io, 8, True), (8, io, False)]
    params = O.init_params(sched, np.random.default_rng(3))
    acts = []
    for image in (True, False):
        t = HipEmbeddingTrainer(sched, torch.tensor(p["data"]), torch.tensor(bm).to(torch.uint8), torch.tensor(mtu), 1e-3, 1e-4, 1.0,
                                max_batch=N, precision="bf16", device=DEV, input_noise=noise, presence=SlotPresence(p["present"]),
                                dataset_image=image)
        t.load_params(params)
        assert (t.engine._dataset_image is not None) == image
        eng = t.engine
        eng.step_forward_loss(t._batch(rows_t, 0), eng.hyper(1e-3, 1e-4, 1.0, global_rows=N, step=2))
        torch.cuda.synchronize()
        acts.append(eng.acts.clone().cpu())
    assert torch.equal(acts[0], acts[1])
    ref, cls = R.corrupt(p["data"][rows], p["data"], rows, 2, S, p["p"], R.SEED, p["pool"], p["present"], p["table"][mtu[rows, 0]])
    R.assert_all_classes(cls)
    ld = 64                                                                    # bf16 activations pad their rows to multiples of 64
    act0 = acts[0][:N * ld * 2].view(torch.bfloat16).view(N, ld)
    assert torch.equal(_bits(act0[:, :io]), _bits(torch.tensor(ref).to(torch.bfloat16))) and (act0[:, io:] == 0).all()


# ---- the fused step against the oracle -----------------------------------------------------------------------------------------

class SwapOracle:
    """tests/test_gpu_noise.py's NoisyOracle: forward on the corrupted input c, loss against the clean x."""

    def __init__(self, params, relu_flags, lr, weight_decay, quant=None):
        from oracle import dae_oracle as O
        self.O = O
        self.params = [(w.astype(np.float32).copy(), b.astype(np.float32).copy()) for w, b in params]
        self.relu, self.lr, self.wd, self.quant = list(relu_flags), lr, weight_decay, quant
        self.adam = O.adam_init(self.params)
        self.last_grads = None

    def step(self, x, c, fmask):
        O = self.O
        y, acts = O.forward(self.params, self.relu, c, keep=True, quant=self.quant)
        loss = O.mse_mean(x, y)
        grads = O.backward(self.params, self.relu, acts, O.mse_mean_grad_y(x, y), quant=self.quant)
        self.last_grads = grads
        clipped, gnorm = O.clip_grad_norm(grads, 1.0)
        self.params = O.adam_step(self.params, clipped, self.adam, self.lr, self.wd)
        se = ((x - y) ** 2).astype(np.float32)
        return {"loss": float(loss), "grad_norm": float(gnorm), "sq_full": float(np.sum(se)), "sq_partial": float(np.sum((1 - fmask) * se))}


def _golden_setup(g, precision):
    """(trainer, noise, S): swap noise p = 0.25 whose pool is the golden run's training rows."""
    from codae.train import HipEmbeddingTrainer
    m = g.meta
    pool = np.unique(np.concatenate([np.asarray(idx) for idx, _ in g.calls()]))
    noise = _noise(0.25, pool, seed=20260)
    sched = [(w.shape[1], w.shape[0], r) for (w, _), r in zip(g.params("init"), g.relu_flags())]
    t = HipEmbeddingTrainer(sched, torch.tensor(g["data"]), torch.tensor(g["binary_masks"]).to(torch.uint8),
                            torch.tensor(g["mask_to_use"]).to(torch.int32), m["lr"], m["weight_decay"], clip=1.0, max_batch=m["batch"],
                            precision=precision, device=DEV, input_noise=noise)
    t.load_params(g.params("init"))
    return t, noise, t._slots()[0]


def _golden_input(g, idx, run, step, noise, S):
    from oracle import dae_oracle as O
    _, fmask = O.get_masks(g["binary_masks"], g["nb_missing_per_run"], g["mask_to_use"], 1, idx, run)
    x = g["data"][idx]
    c, cls = R.corrupt(x, g["data"], idx, step, S, noise.p, noise.seed, noise.pool, None, fmask)
    assert (cls == 3).sum() > 0 and (cls == 0).sum() > 0 and not np.array_equal(c, x * fmask)     # some slots swapped, not all
    return x, c, fmask


@pytest.mark.parametrize("name,steps", [("embedding_wide_square", 3), ("embedding_taper", 1)])
def test_fused_f32_step_with_swap_noise_matches_the_oracle(name, steps):
    g = Golden(name)
    t, noise, S = _golden_setup(g, "f32")
    eng = t.engine
    orc = SwapOracle(g.params("init"), g.relu_flags(), g.meta["lr"], g.meta["weight_decay"])
    for s, (idx, run) in enumerate(g.calls()[:steps]):
        x, c, fmask = _golden_input(g, idx, run, s + 1, noise, S)
        ro = orc.step(x, c, fmask)
        eng.zero_metric_sums()
        t.train_batch(torch.tensor(idx, dtype=torch.int32, device=DEV), run=run)
        sq, sqp, gsq, loss = eng.read_scalars()
        print(name, s, "loss", loss, ro["loss"], "gnorm", math.sqrt(gsq), ro["grad_norm"], "sums", sq, ro["sq_full"], sqp, ro["sq_partial"])
        assert close(loss, ro["loss"]), (s, loss, ro["loss"])
        assert close(math.sqrt(gsq), ro["grad_norm"]), (s, math.sqrt(gsq), ro["grad_norm"])
        assert close(sq, ro["sq_full"]) and close(sqp, ro["sq_partial"]), (s, sq, ro["sq_full"], sqp, ro["sq_partial"])
        if s == 0 and name == "embedding_wide_square":
            for l, (gw, gb) in enumerate(orc.last_grads):
                assert close(eng.weight_grad(l).cpu().numpy(), gw, atol=1e-8), ("dW", l, max_err(eng.weight_grad(l).cpu().numpy(), gw))
                assert close(eng.bias_grad(l).cpu().numpy(), gb, atol=1e-8), ("db", l)


def _rel_l2(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def test_fused_bf16_first_step_with_swap_noise_matches_the_bf16_rounded_oracle():
    """The bounds of test_fused_bf16_first_step_with_masking_noise_matches_the_bf16_rounded_oracle: loss 1e-6, gradient norm 1e-5,
    blanked-slot sum 1e-6 (relative), every gradient tensor 2e-3 relative L2.  The trainer keeps its dataset image: the swapped
    input comes from it."""
    from oracle import dae_oracle as O
    g = Golden("embedding_wide_square")
    t, noise, S = _golden_setup(g, "bf16")
    eng = t.engine
    assert eng.precision == 1 and eng.step_path(g.meta["batch"]) == "layers" and eng._dataset_image is not None
    orc = SwapOracle(g.params("init"), g.relu_flags(), g.meta["lr"], g.meta["weight_decay"], quant=O.bf16_round)
    idx, run = g.calls()[0]
    x, c, fmask = _golden_input(g, idx, run, 1, noise, S)
    ro = orc.step(x, c, fmask)
    eng.zero_metric_sums()
    t.train_batch(torch.tensor(idx, dtype=torch.int32, device=DEV), run=run)
    sq, sqp, gsq, loss = eng.read_scalars()
    print("loss", loss, ro["loss"], "gnorm", math.sqrt(gsq), ro["grad_norm"], "sq_partial", sqp, ro["sq_partial"])
    assert abs(loss - ro["loss"]) <= 1e-6 * ro["loss"], (loss, ro["loss"])
    assert abs(math.sqrt(gsq) - ro["grad_norm"]) <= 1e-5 * ro["grad_norm"], (math.sqrt(gsq), ro["grad_norm"])
    assert abs(sqp - ro["sq_partial"]) <= 1e-6 * ro["sq_partial"]
    for l, (gw, gb) in enumerate(orc.last_grads):
        assert _rel_l2(eng.weight_grad(l).cpu().numpy(), gw) <= 2e-3, ("dW", l)
        assert _rel_l2(eng.bias_grad(l).cpu().numpy(), gb) <= 2e-3, ("db", l)


# ---- emphasis sees the swap ------------------------------------------------------------------------------------------------------

def _small(io, z, B, seed, n_rows=120, S=3):
    """io -> z -> io, S one-slot masks, one mask run, a presence table with a fifth of the slots absent, a pool of 40 rows."""
    from oracle import dae_oracle as O
    rng = np.random.default_rng(seed)
    E = io // S
    data = rng.random((n_rows, io), dtype=np.float32)
    sched = [(io, z, True), (z, io, False)]
    params = O.init_params(sched, rng)
    bm, nmr, _ = O.corrupter_tables([{"size": E, "position": s * E} for s in range(S)], 1)
    mtu = rng.integers(0, S, (n_rows, 1)).astype(np.int32)
    present = rng.random((n_rows, S)) > 0.2
    pool = np.sort(rng.permutation(n_rows)[:40])
    order = [rng.permutation(n_rows)[:B].astype(np.int32) for _ in range(4)]
    return dict(io=io, S=S, E=E, data=data, sched=sched, params=params, bm=bm, nmr=nmr, mtu=mtu, order=order, B=B, present=present, pool=pool,
                N=n_rows)


def _small_trainer(p, precision, **kw):
    from codae.train import HipEmbeddingTrainer
    t = HipEmbeddingTrainer(p["sched"], torch.tensor(p["data"]), torch.tensor(p["bm"]).to(torch.uint8), torch.tensor(p["mtu"]), 1e-3,
                            1e-4, 1.0, max_batch=p["B"], precision=precision, device=DEV, **kw)
    t.load_params(p["params"])
    return t


@pytest.mark.parametrize("crit", ["mse", "l1", "slot_cosine"])
def test_emphasis_weights_the_swapped_slots_io24_z8_b33(crit):
    """fp32 engine, LossEmphasis(alpha 3, beta 1), swap p = 0.4 with a pool and the trainer's presence table: the step's loss and dY
    against the float64 loss of the host classes with corrupted = blank | swapped."""
    from codae.tool import LossEmphasis, ReconstructionLoss, SlotPresence
    from oracle import dae_oracle as O
    p = _small(24, 8, 33, seed=31)
    io, S, E, B = p["io"], p["S"], p["E"], p["B"]
    noise = _noise(0.4, p["pool"], seed=11)
    emph = LossEmphasis(3.0, 1.0)
    criterion = None if crit == "mse" else ReconstructionLoss(crit)
    t = _small_trainer(p, "f32", input_noise=noise, loss_emphasis=emph, criterion=criterion, presence=SlotPresence(p["present"]), n_slots=S)
    eng = t.engine
    idx = p["order"][0]
    cls, _ = R.classify(idx, 1, S, noise.p, noise.seed, p["N"], p["pool"], p["present"])
    R.assert_all_classes(cls)
    acc, _ = noise.swapped(idx, 1, S, n_rows=p["N"], presence=p["present"])
    assert np.array_equal(acc, cls == 3)
    y_t = torch.empty((B, io), dtype=torch.float32, device=DEV)
    eng.step_forward_loss(t._batch(torch.tensor(idx, device=DEV), 0), eng.hyper(1e-3, 1e-4, 1.0, global_rows=B, step=1), out_y=y_t)
    loss = eng.read_scalars()[3]
    one = eng.dacts.numel() // min(len(p["sched"]) + 1, 16)
    dy = eng.dacts[one:one + B * io * 4].clone().view(torch.float32).view(B, io).cpu().numpy().astype(np.float64)
    # float64 reference from the same y
    fmask = O.get_masks(p["bm"], p["nmr"], p["mtu"], 1, idx, 0)[1]
    pres = np.repeat(p["present"][idx], E, axis=1)
    corrupted = (fmask == 0) | np.repeat(acc, E, axis=1)
    x = torch.tensor(p["data"][idx], dtype=torch.float64) * torch.tensor(pres)            # an absent element: x = y = 0, no term
    y = (y_t.cpu().double() * torch.tensor(pres)).requires_grad_(True)
    w = emph.weights(torch.tensor(corrupted)).double()
    plain = emph.weights(torch.tensor(fmask == 0)).double()
    if crit == "mse":
        ref = emph.loss(x, y, torch.tensor(fmask), corrupted=torch.tensor(corrupted), global_rows=B)
    elif crit == "l1":
        assert (np.abs((x - y).detach().numpy())[pres] > 1e-6).all()                       # sign(d) is never in doubt
        ref = criterion.loss(x, y, weight=w, global_rows=B)
    else:
        # an absent pair has no term (not the term W of a zero target): weight its elements 0 on the reference side
        ref = criterion.loss(x, y, weight=w * torch.tensor(pres), n_slots=S, global_rows=B)
    ref.backward()
    ref = float(ref.detach())
    rdy = y.grad.numpy() * pres
    print(crit, "loss", loss, ref, "swapped slots", int(acc.sum()))
    assert abs(float((w - plain).abs().sum())) > 0                                         # the swap moves the weights
    if crit == "slot_cosine":
        xs, ys = x.numpy().reshape(B, S, E), y.detach().numpy().reshape(B, S, E)
        nx = np.maximum(np.linalg.norm(xs, axis=2), 1e-8)[:, :, None]
        ny = np.maximum(np.linalg.norm(ys, axis=2), 1e-8)[:, :, None]
        W = (w.numpy() * pres).reshape(B, S, E).mean(axis=2)[:, :, None]
        k = W / (B * S)
        tol = ((E + 8) * 2.0 ** -23 * k * (np.abs(xs) / (nx * ny) + np.abs(ys) / ny ** 2)).reshape(B, io)
        assert (np.abs(dy - rdy) <= tol).all(), float((np.abs(dy - rdy) / np.maximum(tol, 1e-300)).max())
        assert abs(loss - float(ref)) <= (E * (E + 8) * 2.0 ** -24 * float(W.sum()) / (B * io)) + B * io * 2.0 ** -24 * float(ref)
    else:
        np.testing.assert_allclose(dy, rdy, rtol=1e-6, atol=0)
        assert abs(loss - float(ref)) <= B * io * 2.0 ** -24 * float(ref), (loss, float(ref))
    # with alpha = beta the swap changes nothing in the loss kernel: the weights alone carry it
    assert (dy[~pres] == 0).all()


# ---- step forms (width 192, 10 layers, batch 128) ----------------------------------------------------------------------------------

def _stack(io, n_in, n_out, B, seed, n_rows=None):
    from oracle import dae_oracle as O
    rng = np.random.default_rng(seed)
    n_rows = n_rows or 3 * B
    S = 3
    E = io // S
    data = rng.random((n_rows, io), dtype=np.float32)
    sched = O.layer_schedule(io, io, n_in, n_out, False, "embedding")
    params = O.init_params(sched, rng)
    bm, _, _ = O.corrupter_tables([{"size": E, "position": s * E} for s in range(S)], 1)
    mtu = rng.integers(0, S, (n_rows, 1)).astype(np.int32)
    order = [torch.tensor(rng.permutation(n_rows)[:B], dtype=torch.int32, device=DEV) for _ in range(4)]
    pools = [np.sort(rng.permutation(n_rows)[:n_rows // 2]) for _ in range(2)]
    return dict(data=data, sched=sched, params=params, bm=bm, mtu=mtu, order=order, B=B, pools=pools, N=n_rows, S=S, E=E, io=io)


def _trainer(p, precision="bf16", **kw):
    from codae.train import HipEmbeddingTrainer
    t = HipEmbeddingTrainer(p["sched"], torch.tensor(p["data"]), torch.tensor(p["bm"]).to(torch.uint8), torch.tensor(p["mtu"]), 1e-3,
                            1e-4, 1.0, max_batch=p["B"], precision=precision, device=DEV, **kw)
    t.load_params(p["params"])
    return t


def test_graph_replay_with_swap_gives_the_bits_of_plain_steps_and_a_pool_change_recaptures_width192_10layers_batch128():
    p = _stack(192, 4, 4, 128, seed=41)
    assert len(p["sched"]) == 10
    na, nb = _noise(0.3, p["pools"][0], seed=5), _noise(0.3, p["pools"][1], seed=5)
    out = []
    for graph in (False, True):
        t = _trainer(p, input_noise=na, use_graph=graph)
        for s in range(4):
            if s == 2:
                t.set_input_noise(nb)                                          # the same p and seed, another pool
            t.train_batch(p["order"][s], run=0)
        out.append((t.engine.params.clone(), t.engine.read_scalars()))
        if graph:
            assert t.engine.graph_captures() == 2, t.engine.graph_captures()
    assert out[0][1] == out[1][1], (out[0][1], out[1][1])
    assert torch.equal(out[0][0], out[1][0]), float((out[0][0] - out[1][0]).abs().max())
    # it depends on the step and on the pool: neither replaying step 1's draws nor keeping the first pool gives these bits
    t = _trainer(p, input_noise=na, use_graph=True)
    for s in range(4):
        t.train_batch(p["order"][s], run=0)
    assert t.engine.graph_captures() == 1 and not torch.equal(t.engine.params, out[0][0])
    t = _trainer(p, input_noise=_noise(0.3, p["pools"][0], seed=6), use_graph=True)
    for s in range(2):
        t.train_batch(p["order"][s], run=0)
    u = _trainer(p, input_noise=na, use_graph=True)
    for s in range(2):
        u.train_batch(p["order"][s], run=0)
    assert not torch.equal(t.engine.params, u.engine.params)


def test_step_forward_loss_with_a_hyper_is_swapped_like_train_step():
    p = _stack(192, 2, 2, 256, seed=42)
    noise = _noise(0.3, p["pools"][0], seed=3)
    a, b, c = _trainer(p, input_noise=noise), _trainer(p, input_noise=noise), _trainer(p)
    idx = p["order"][0]
    a.train_batch(idx, run=0)
    losses = []
    for tr, step in ((b, 1), (b, 2), (c, 1)):
        eng = tr.engine
        eng.step_forward_loss(tr._batch(idx, 0), eng.hyper(1e-3, 1e-4, 1.0, global_rows=256, step=step))
        losses.append(eng.read_scalars()[3])
    assert losses[0] == a.engine.read_scalars()[3]
    assert losses[1] != losses[0] and losses[2] != losses[0]


def test_two_shards_build_the_rows_of_the_global_batch_width192_10layers_batch128():
    """The input rows and, through the emphasised loss kernel given the global batch's y, the gradient rows dY of two shards of 64
    are the bits of the same rows of the batch of 128 (loss_scale_rows = 128 on every side)."""
    from codae import hip
    from codae.tool import LossEmphasis
    p = _stack(192, 4, 4, 128, seed=43)
    io, S, B = p["io"], p["S"], 128
    noise = _noise(0.3, p["pools"][0], seed=9)
    idx = p["order"][0]
    ref, cls = R.corrupt(p["data"][idx.cpu().numpy()], p["data"], idx.cpu().numpy(), 1, S, noise.p, noise.seed, noise.pool, None,
                         p["bm"][p["mtu"][idx.cpu().numpy(), 0]])
    assert (cls == 3).any() and (cls == 0).any()
    acts = []
    for rows in (idx, idx[:64], idx[64:]):
        t = _trainer(p, input_noise=noise, loss_emphasis=LossEmphasis(3.0, 1.0))
        eng = t.engine
        eng.step_forward_loss(t._batch(rows.contiguous(), 0), eng.hyper(1e-3, 1e-4, 1.0, global_rows=B, step=1))
        torch.cuda.synchronize()
        acts.append(eng.acts[:rows.numel() * io * 2].clone().view(torch.bfloat16).view(-1, io).cpu())
    assert torch.equal(_bits(acts[0]), _bits(torch.cat(acts[1:]))) and torch.equal(_bits(acts[0]), _bits(torch.tensor(ref).to(torch.bfloat16)))
    # dY through codae_emph_loss_swap: the global batch, then its halves with the same inv_n
    data_t = torch.tensor(p["data"], device=DEV)
    table_t, mtu_t = torch.tensor(p["bm"]).to(torch.uint8).to(DEV), torch.tensor(p["mtu"], device=DEV)
    y = torch.tensor(np.random.default_rng(7).random((B, io), dtype=np.float32), device=DEV)
    pool_t = torch.tensor(noise.pool.astype(np.int32), device=DEV)
    sw, st, em = hip.Swap(hip.ptr(pool_t), int(pool_t.numel()), S), noise.as_struct(), hip.Emphasis(3.0, 1.0, None)

    def dy_of(rows, yy):
        n = int(rows.numel())
        blocks = hip.lib().codae_emph_loss_blocks(n)
        dy = torch.zeros((n, io), dtype=torch.bfloat16, device=DEV)
        parts = torch.zeros((blocks, 3), dtype=torch.float64, device=DEV)
        batch = hip.Batch(hip.ptr(data_t), hip.ptr(rows), None, hip.ptr(table_t), n, io, hip.ptr(mtu_t), 1, 0)
        hip.check(hip.lib().codae_emph_loss_swap(C.byref(batch), C.byref(st), 1, C.byref(em), hip.ptr(yy), hip.ptr(dy), 1, io,
                                                 1.0 / (B * io), None, hip.ptr(parts), C.byref(sw), None, 0, hip.current_stream()))
        torch.cuda.synchronize()
        return dy.cpu(), float(parts[:, 0].sum())
    full, wsum = dy_of(idx, y)
    lo, _ = dy_of(idx[:64].contiguous(), y[:64].contiguous())
    hi, _ = dy_of(idx[64:].contiguous(), y[64:].contiguous())
    assert torch.equal(_bits(full), _bits(torch.cat([lo, hi])))
    # ... and the swapped slots carry alpha: the weighted sum is that of the float64 statement
    rows = idx.cpu().numpy()
    acc = noise.swapped(rows, 1, S, n_rows=p["N"])[0]
    keep = p["bm"][p["mtu"][rows, 0]]
    w = np.where((keep == 0) | np.repeat(acc, p["E"], axis=1), 3.0, 1.0)
    want = float((w * (p["data"][rows].astype(np.float64) - y.cpu().numpy().astype(np.float64)) ** 2).sum())
    assert abs(wsum - want) <= B * io * 2.0 ** -24 * want, (wsum, want)


def test_swap_keeps_the_stack_off_the_chain_kernel_and_off_restores_it_3x64_batch256():
    p = _stack(192, 2, 2, 256, seed=44)
    fresh = _trainer(p)
    t = _trainer(p, input_noise=_noise(0.3, p["pools"][0], seed=1))
    assert fresh.engine.step_path(256) == "chain" and t.engine.step_path(256) == "layers"
    t.set_input_noise(None)
    assert t.engine.step_path(256) == "chain"
    for tr in (fresh, t):
        tr.train_batch(p["order"][0], run=0)
    assert fresh.engine.read_scalars() == t.engine.read_scalars()
    assert torch.equal(fresh.engine.params, t.engine.params)
    assert torch.equal(fresh.engine.adam_v, t.engine.adam_v)


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_evaluation_completion_and_scoring_never_swap(precision):
    p = _stack(192, 2, 2, 256, seed=45)
    clean = _trainer(p, precision)
    noisy = _trainer(p, precision, input_noise=_noise(0.5, p["pools"][0], seed=9))
    idx = p["order"][1]
    items = torch.stack([idx[:40], idx[40:80], idx[80:120]], dim=1).to(torch.int64)
    res = []
    for tr in (clean, noisy):
        tr.engine.zero_metric_sums()
        y = tr.eval_batch(idx, run=0, want_y=True)
        sums = tr.epoch_sums(reset=False)
        top = tr.complete(idx[:50], 1, 5)
        top_items = tr.complete_items(items, 1, 5)
        score = tr.score_outfits(items)["score"]
        res.append((y, sums, top, top_items, score))
    assert torch.equal(res[0][0].view(torch.int32), res[1][0].view(torch.int32)) and res[0][1] == res[1][1]
    for k in (2, 3):
        assert torch.equal(res[0][k][0], res[1][k][0]) and torch.equal(res[0][k][1], res[1][k][1])
    assert torch.equal(torch.as_tensor(res[0][4]), torch.as_tensor(res[1][4]))
    for tr in (clean, noisy):                                                  # ... while the training step of the same engine swaps
        tr.train_batch(idx, run=0)
    assert clean.engine.read_scalars()[3] != noisy.engine.read_scalars()[3]


def test_bad_swap_settings_are_refused_by_the_library_and_launch_nothing():
    from codae import hip
    from codae.hip import HipError
    p = _stack(192, 2, 2, 256, seed=46)
    good = _noise(0.3, p["pools"][0], seed=2)
    t = _trainer(p, input_noise=good)
    eng, lib = t.engine, hip.lib()
    pool_t = torch.tensor(p["pools"][0].astype(np.int32), device=DEV)

    def refused(rc, word):
        assert rc == -1 and word in lib.codae_last_error().decode(), (rc, lib.codae_last_error())
    refused(lib.codae_set_input_noise(eng._h, C.byref(hip.Noise(4, 1.5, 0.0, 0.0, 0))), "p 1.5")
    refused(lib.codae_set_input_noise(eng._h, C.byref(hip.Noise(4, -0.1, 0.0, 0.0, 0))), "p -0.1")
    refused(lib.codae_set_swap_pool(eng._h, hip.ptr(pool_t), int(pool_t.numel()), 0), "slot count")
    refused(lib.codae_set_swap_pool(eng._h, hip.ptr(pool_t), int(pool_t.numel()), 5), "does not divide")
    refused(lib.codae_set_swap_pool(eng._h, hip.ptr(pool_t), 0, 3), "pool of 0")
    refused(lib.codae_set_swap_pool(eng._h, None, 0, 0), "switch it off")
    assert eng.input_noise is good and eng.step_path(256) == "layers"                  # the previous setting stays ...
    u = _trainer(p, input_noise=good)
    for tr in (t, u):
        tr.train_batch(p["order"][0], run=0)
    assert t.engine.read_scalars() == u.engine.read_scalars() and torch.equal(t.engine.params, u.engine.params)     # ... and still trains as set
    fresh = _trainer(p)
    refused(lib.codae_set_input_noise(fresh.engine._h, C.byref(hip.Noise(4, 0.3, 0.0, 0.0, 0))), "slot count")     # SWAP without slots
    assert fresh.engine.step_path(256) == "chain"
    # the stand-alone launcher: nothing is written on a refusal
    data_t = torch.tensor(p["data"], device=DEV)
    out = torch.full((8, 192), 7.0, device=DEV)
    batch = hip.Batch(hip.ptr(data_t), None, None, None, 8, 192, None, 0, 0)
    st = good.as_struct()
    for sw, word in ((hip.Swap(None, p["N"], 0), "slot count"), (hip.Swap(None, p["N"], 7), "does not divide"), (hip.Swap(None, 0, 3), "pool of 0")):
        refused(lib.codae_corrupt_batch_swap(C.byref(batch), C.byref(st), 1, None, None, C.byref(sw), hip.ptr(out), 0, 192, None, 0,
                                             hip.current_stream()), word)
    refused(lib.codae_corrupt_batch(C.byref(batch), C.byref(st), 1, None, hip.ptr(out), 0, 192, hip.current_stream()), "slot count")
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    with pytest.raises(HipError, match="outside the dataset"):
        t.set_input_noise(_noise(0.3, [0, p["N"]]))
