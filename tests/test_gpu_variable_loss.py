"""The mixed-variable criterion on a real MI355X (include/codae_hip.h, "Mixed-variable criterion").

1. The kernel entry (codae_variable_loss_fwd_bwd) against the oracle's combined_mean / combined_mean_grad_y: the loss, dY, the last
   bias gradient's partial rows summed and the two monitor sums at the project's fp32 parity tolerance (rtol 1e-3 / atol 1e-5), at
   batch sizes around the 32- and 64-row block edges, on the abalone arch (io 11: nothing is a multiple of 4) and on an io-56 arch
   with a 40-wide one-hot, regressions of 5 columns and variables that straddle 16-byte groups; bf16 dY with a padded leading
   dimension = the fp32 dY rounded to nearest even, bit for bit; two calls give the same bits; an exactly reconstructed regression
   variable is NaN in its own columns only.
2. The reference's abalone run (golden fixture abalone_k2: 180 training steps, the validation sweeps, batches 64/64/64/18) through
   the fused step inside the script's sweep, against everything the fixture recorded; graph replay gives the plain run's state.
3. The bf16 engine's first step on the io-56 arch against the oracle with bf16 operands: 2e-3 relative L2 per gradient tensor
   (tests/test_gpu_parity.py's bound for that comparison), the loss within 1e-3.
4. One fp32 step each with masking noise, hidden dropout, layer norm, LAMB and tied weights against the host restatements those
   options' own tests use, the criterion being VariableLoss.loss under float64 autograd; save / load / resume bit for bit.  Graph
   replay takes the criterion on its own only: with any of those options the step is refused by name.  output_view on a bf16 stack
   whose rows are padded.
5. What assumes equal-width slots is refused, naming the option, and the trainer stays usable.
"""
import ctypes as C
import math

import numpy as np
import pytest

from golden_util import Golden, close, max_err
from oracle import dae_oracle as O
from test_variable_loss_host import ARCH_B, WEIGHT_B, rows_for

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
FILL = 7.0


def _bits(t):
    return t.view({torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}[t.dtype])


def _arch_a():
    m = Golden("abalone_k2").meta
    return m["arch"], m["weight"]


def _vl(arch, weight):
    from codae.tool import VariableLoss
    return VariableLoss(arch, weight)


# ---- 1. the kernel entry ------------------------------------------------------------------------------------------------------------

_PROBLEMS = {}


def _problem(name, B):
    """Dataset of B + 9 rows read through a permutation, an output y, the mask route of the step (mask_to_use, run 0), the oracle's
    answers: computed once per (arch, B), never modified."""
    if (name, B) not in _PROBLEMS:
        arch, weight = _arch_a() if name == "A" else (ARCH_B, WEIGHT_B)
        N = B + 9
        data, _ = rows_for(arch, N, 100 + B)
        rng = np.random.default_rng(7 * B + len(arch))
        rows = rng.permutation(N)[:B].astype(np.int32)
        x = data[rows]
        y = (x + rng.normal(0, 0.5, x.shape)).astype(np.float32)
        bm, nmr, _ = O.corrupter_tables(arch, 1)
        mtu = np.stack([rng.permutation(len(bm)) for _ in range(N)]).astype(np.int32)
        _, fmask = O.get_masks(bm, nmr, mtu, 1, rows, 0)
        se = ((x - y).astype(np.float64)) ** 2
        p = dict(arch=arch, weight=weight, B=B, io=x.shape[1], x=x, y=y, loss=float(O.combined_mean(arch, weight, x, y)),
                 dy=O.combined_mean_grad_y(arch, weight, x, y), sq=float(se.sum()), sqp=float(((1 - fmask) * se).sum()))
        p["dev"] = dict(data=torch.tensor(data, device=DEV), rows=torch.tensor(rows, device=DEV), y=torch.tensor(y, device=DEV),
                        table=torch.tensor(bm, device=DEV).to(torch.uint8).contiguous(), mtu=torch.tensor(mtu, device=DEV))
        _PROBLEMS[(name, B)] = p
    return _PROBLEMS[(name, B)]


def kernel(p, y=None, dy_bf16=False, dy_ld=None):
    """codae_variable_loss_fwd_bwd -> (rc, dy [B, ld] prefilled, colsum_part [blocks, io], scalars [S_COUNT] float64)"""
    from codae import hip
    d, B, io = p["dev"], p["B"], p["io"]
    lib = hip.lib()
    ld = io if dy_ld is None else dy_ld
    blocks = lib.codae_variable_loss_blocks(B)
    assert blocks == (B + 31) // 32
    vl = _vl(p["arch"], p["weight"])
    need = lib.codae_variable_loss_ws_bytes(vl.n_var, B)
    assert need == 16 * vl.n_var + 8 * (vl.n_var + blocks * (vl.n_var + 2))
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    dy = torch.full((B, ld), FILL, dtype=torch.bfloat16 if dy_bf16 else torch.float32, device=DEV)
    colsum = torch.full((blocks, io), FILL, dtype=torch.float32, device=DEV)
    scalars = torch.zeros(hip.S_COUNT, dtype=torch.float64, device=DEV)
    scalars[hip.S_GRAD_SQ] = 3.0
    batch = hip.Batch(hip.ptr(d["data"]), hip.ptr(d["rows"]), None, hip.ptr(d["table"]), B, io, hip.ptr(d["mtu"]), int(d["mtu"].shape[1]), 0)
    st = vl.as_struct(ws)
    yy = d["y"] if y is None else y
    rc = lib.codae_variable_loss_fwd_bwd(C.byref(batch), C.byref(st), hip.ptr(yy), hip.ptr(dy), int(dy_bf16), ld, hip.ptr(colsum),
                                         hip.ptr(scalars), hip.current_stream())
    torch.cuda.synchronize()
    return rc, dy, colsum, scalars


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("name", ["A", "B"])
def test_kernel_entry_matches_the_oracle(name, B):
    from codae import hip
    p = _problem(name, B)
    rc, dy, colsum, sc = kernel(p)
    assert rc == 0, hip.lib().codae_last_error()
    got = dy.cpu().numpy()
    s = sc.cpu().numpy()
    print("MEASURE variable loss %s B %d: loss %.8g oracle %.8g  dy worst %.3f  colsum worst %.3f  sq %.8g / %.8g  sqp %.8g / %.8g" % (
        name, B, s[hip.S_LAST_LOSS], p["loss"], max_err(got, p["dy"]), max_err(colsum.cpu().numpy().sum(axis=0), p["dy"].sum(axis=0)),
        s[hip.S_SQ_FULL], p["sq"], s[hip.S_SQ_PARTIAL], p["sqp"]))
    assert close(s[hip.S_LAST_LOSS], p["loss"])
    assert close(got, p["dy"])
    assert close(colsum.cpu().numpy().sum(axis=0), p["dy"].sum(axis=0, dtype=np.float64))
    assert close(s[hip.S_SQ_FULL], p["sq"]) and close(s[hip.S_SQ_PARTIAL], p["sqp"])
    assert s[hip.S_GRAD_SQ] == 0 and s[hip.S_STEP_SQ] == 0          # (the finish resets the per-step norm accumulators)
    # the same inputs, the same bits
    rc2, dy2, colsum2, sc2 = kernel(p)
    assert rc2 == 0
    assert torch.equal(_bits(dy), _bits(dy2)) and torch.equal(_bits(colsum), _bits(colsum2)) and torch.equal(_bits(sc), _bits(sc2))
    if name == "B":
        # bf16 dY, rows 64 elements apart: the fp32 dY rounded to nearest even, the pad columns untouched, the fp32 column sums
        rc3, dyb, colsum3, sc3 = kernel(p, dy_bf16=True, dy_ld=64)
        assert rc3 == 0
        assert torch.equal(_bits(dyb[:, :56].contiguous()), _bits(dy.to(torch.bfloat16).contiguous()))
        assert (dyb[:, 56:].float() == FILL).all()
        assert torch.equal(_bits(colsum), _bits(colsum3)) and torch.equal(_bits(sc), _bits(sc3))
        # fp32 dY with a padded leading dimension
        rc4, dyp, colsum4, _ = kernel(p, dy_ld=60)
        assert rc4 == 0 and torch.equal(_bits(dyp[:, :56].contiguous()), _bits(dy)) and (dyp[:, 56:] == FILL).all()


def test_exactly_reconstructed_regression_variable_is_nan_in_its_columns_only():
    from codae import hip
    p = _problem("B", 65)
    y = p["dev"]["y"].clone()
    y[:, 6:11] = torch.tensor(p["x"][:, 6:11], device=DEV)
    rc, dy, colsum, sc = kernel(p, y=y)
    assert rc == 0
    got = dy.cpu().numpy()
    keep = np.ones(56, dtype=bool); keep[6:11] = False
    assert np.isnan(got[:, 6:11]).all() and np.isfinite(got[:, keep]).all()
    cs = colsum.cpu().numpy()
    assert np.isnan(cs[:, 6:11]).all() and np.isfinite(cs[:, keep]).all()
    want = O.combined_mean_grad_y(ARCH_B, WEIGHT_B, p["x"], np.where(keep, y.cpu().numpy(), p["y"]))
    assert close(got[:, keep], want[:, keep])
    assert math.isfinite(float(sc[hip.S_LAST_LOSS]))          # (L_v = 0 adds nothing to the loss itself)


def test_kernel_entry_refuses_bad_tables():
    from codae import hip
    p = _problem("A", 64)
    lib = hip.lib()
    assert lib.codae_variable_loss_ws_bytes(0, 64) == -1 and lib.codae_variable_loss_ws_bytes(hip.VAR_MAX + 1, 64) == -1
    d = p["dev"]
    ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    dy = torch.full((64, 11), FILL, device=DEV)
    sc = torch.zeros(hip.S_COUNT, dtype=torch.float64, device=DEV)
    batch = hip.Batch(hip.ptr(d["data"]), hip.ptr(d["rows"]), None, None, 64, 11, None, 0, 0)

    def call(pos, size, typ, w, ws_=ws, nbytes=None):
        n = len(pos)
        st = hip.VariableLossStruct(n, 0, (C.c_int32 * n)(*pos), (C.c_int32 * n)(*size), (C.c_int32 * n)(*typ), (C.c_float * n)(*w),
                                    hip.ptr(ws_), int(ws_.numel()) if nbytes is None else nbytes)
        rc = lib.codae_variable_loss_fwd_bwd(C.byref(batch), C.byref(st), hip.ptr(d["y"]), hip.ptr(dy), 0, 11, None, hip.ptr(sc), hip.current_stream())
        return rc, lib.codae_last_error().decode()
    for args, word in ((([0, 2], [3, 9], [1, 0], [1, 1]), "overlaps"), (([0, 4], [3, 7], [1, 0], [1, 1]), "covered by no variable"),
                       (([0, 3], [3, 7], [1, 0], [1, 1]), "covered by no variable"), (([0, 3], [3, 0], [1, 0], [1, 1]), "size"),
                       (([0, 3], [3, 8], [1, 2], [1, 1]), "unknown type"), (([0, 3], [3, 8], [1, 0], [1, -1]), "weight"),
                       (([0, 3], [3, 8], [1, 0], [1, float("nan")]), "weight"), (([0, 3], [3, 9], [1, 0], [1, 1]), "past io")):
        rc, msg = call(*args)
        assert rc == -1 and word in msg, (args, rc, msg)
    rc, msg = call([0, 3], [3, 8], [1, 0], [1, 1], nbytes=64)
    assert rc == -1 and "work space" in msg
    torch.cuda.synchronize()
    assert (dy == FILL).all() and (sc == 0).all()          # (nothing was launched)
    rc, _ = call([0, 3], [3, 8], [1, 0], [1, 1])
    assert rc == 0


# ---- 2. the reference run through the fused step -------------------------------------------------------------------------------------

def _abalone_trainer(g, **kw):
    from codae.train import HipEmbeddingTrainer
    m = g.meta
    sched = [(w.shape[1], w.shape[0], r) for (w, _), r in zip(g.params("init"), g.relu_flags())]
    kw.setdefault("criterion", _vl(m["arch"], m["weight"]))
    t = HipEmbeddingTrainer(sched, torch.tensor(g["data"]), torch.tensor(g["binary_masks"]).to(torch.uint8),
                            torch.tensor(g["mask_to_use"]).to(torch.int32), m["lr"], m["weight_decay"], clip=1.0, max_batch=m["batch"],
                            precision="f32", device=DEV, **kw)
    t.load_params(g.params("init"))
    return t


def _abalone_run(g, t, monitored):
    """The sweep of script/train_dae_on_abalone.py with its step on the fused path: train_batch + last_output into the device monitor; the
    validation sweep through eval_batch(want_y=True).  -> (book, step losses, step gradient norms, gradients of the first step)"""
    from codae.tool import CombinedCriterion, Corrupter
    m = g.meta
    dev = torch.device(DEV)
    tm = torch.tensor(g["type_mask"])
    monitor = CombinedCriterion(arch=m["arch"], k_max=m["k_max"], device=dev, observation_mask=tm, reduction="none")
    corrupter = Corrupter(nb_observation=m["N"], arch=m["arch"], k_max=m["k_max"], device=dev)
    assert np.array_equal(corrupter.binary_masks.numpy(), g["binary_masks"])
    corrupter.mask_to_use = torch.tensor(g["mask_to_use"])
    corrupter.mask_to_use_i32 = corrupter.mask_to_use.to(torch.int32).contiguous().to(dev)
    data = t.data

    class Norm:
        scale = torch.tensor(g["norm_scale"]); min = torch.tensor(g["norm_min"])
    per_k = [int(v) for v in g["nb_corruption_per_k"]]
    nb_run, nb_pred = sum(per_k), len(m["arch"])
    nt, nv = math.ceil(m["nb_train"] / m["batch"]), math.ceil((m["N"] - m["nb_train"]) / m["batch"])
    calls = g.calls()
    n_onehot = m["arch"][0]["size"]
    book = {k: [] for k in ("ftl", "ptl", "fvl", "pvl", "ftl_per_k", "ptl_per_k", "fvl_per_k", "pvl_per_k")}
    losses, gnorms, grad0 = [], [], []
    c = 0

    def sweep(n_batches, n_rows, train):
        nonlocal c
        for run in range(nb_run):
            for _ in range(n_batches):
                idx, r_ = calls[c]; c += 1
                assert r_ == run
                rows = torch.tensor(np.asarray(idx), dtype=torch.int32, device=dev)
                if train:
                    t.train_batch(rows, run=run)
                    y = t.last_output()
                    if monitored:
                        _, _, gsq, loss = t.engine.read_scalars()
                        losses.append(loss); gnorms.append(math.sqrt(gsq))
                        if not grad0:
                            for l in range(t.engine.L):
                                grad0.append((t.engine.weight_grad(l).cpu().numpy().copy(), t.engine.bias_grad(l).cpu().numpy().copy()))
                else:
                    y = t.eval_batch(rows, run=run, want_y=True)
                if monitored:
                    long_rows = rows.long()
                    monitor.accumulate(data[long_rows], y, corrupter.mask_ids(long_rows, run), corrupter, normalizer=Norm,
                                       first_scaled_column=n_onehot)
        if not monitored:
            return None
        f, p, f_k, p_k = monitor.accumulated()
        for i in range(len(per_k)):
            f_k[i, :] /= n_rows * sum(per_k[:i + 1])
            p_k[i, :] /= n_rows * sum(per_k[:i + 1]) / nb_pred
        f /= sum(per_k) * n_rows
        p /= sum(per_k) * n_rows / nb_pred
        f_k[:, 1:] = np.sqrt(f_k[:, 1:]); p_k[:, 1:] = np.sqrt(p_k[:, 1:])
        return np.sqrt(f), np.sqrt(p), f_k, p_k

    for _ in range(m["epochs"]):
        r = sweep(nt, m["nb_train"], True)
        if monitored:
            for k, v in zip(("ftl", "ptl", "ftl_per_k", "ptl_per_k"), r):
                book[k].append(v)
        r = sweep(nv, m["N"] - m["nb_train"], False)
        if monitored:
            for k, v in zip(("fvl", "pvl", "fvl_per_k", "pvl_per_k"), r):
                book[k].append(v)
    assert c == len(calls)
    return book, losses, gnorms, grad0


def test_abalone_reference_run_through_the_fused_step_and_graph_replay():
    g = Golden("abalone_k2")
    t = _abalone_trainer(g)
    assert t.engine.step_path(64) == "layers"
    book, losses, gnorms, grad0 = _abalone_run(g, t, True)
    assert len(losses) == 180
    print("MEASURE abalone fused: step loss worst %.3f  grad norm worst %.3f" % (max_err(losses, g["step_loss"]), max_err(gnorms, g["step_grad_norm"])))
    assert close(losses, g["step_loss"]), max_err(losses, g["step_loss"])
    assert close(gnorms, g["step_grad_norm"]), max_err(gnorms, g["step_grad_norm"])
    for l, (gw, gb) in enumerate(g.list("grad0")):
        assert close(grad0[l][0], gw), ("grad0 W", l, max_err(grad0[l][0], gw))
        assert close(grad0[l][1], gb), ("grad0 b", l, max_err(grad0[l][1], gb))
    eng = t.engine
    for name, flat in (("adam_m", eng.adam_m), ("adam_v", eng.adam_v)):
        for l, (gw, gb) in enumerate(g.list(name)):
            assert close(eng._view(flat, l, False).cpu().numpy(), gw), (name, "W", l)
            assert close(eng._view(flat, l, True).cpu().numpy(), gb), (name, "b", l)
    for l, (gw, gb) in enumerate(g.params("final")):
        assert close(eng.weight(l).cpu().numpy(), gw), ("final W", l, max_err(eng.weight(l).cpu().numpy(), gw))
        assert close(eng.bias(l).cpu().numpy(), gb), ("final b", l)
    for k in ("ftl", "ptl", "fvl", "pvl"):
        assert close(book[k], g["book_" + k]), (k, book[k], g["book_" + k])
    for k in ("ftl_per_k", "ptl_per_k", "fvl_per_k", "pvl_per_k"):
        assert close(np.stack(book[k]), g["book_" + k]), k
    # graph replay: the same 180 steps (the ragged 18-row batches re-capture), the same state
    tg = _abalone_trainer(g, use_graph=True)
    _abalone_run(g, tg, False)
    from codae import hip
    a, b = t.state_digest(), tg.state_digest()
    differ = sorted(k for k in a if a[k] != b[k])
    # scalars[CODAE_S_ADAM_STEP] is the replay's own device-side step counter: codae_train_step_graph writes it before every launch
    # and codae_train_step never does, under any criterion.  Everything else - parameters, moments, and every other scalar, the
    # epoch sums, the last loss and the gradient norm's accumulators among them - has the plain run's bits.
    assert set(differ) <= {"scalars", "all"}, "graph replay differs from the plain run in %s" % differ
    sa, sb = t.engine.scalars.cpu(), tg.engine.scalars.cpu()
    assert float(sa[hip.S_ADAM_STEP]) == 0.0 and float(sb[hip.S_ADAM_STEP]) == 180.0
    sb[hip.S_ADAM_STEP] = sa[hip.S_ADAM_STEP]
    assert torch.equal(_bits(sa), _bits(sb)), "graph replay's scalars differ from the plain run's"
    assert tg.engine.graph_captures() >= 2


# ---- 3. bf16 ------------------------------------------------------------------------------------------------------------------------

def _problem_b_stack(B=70, hidden=24, seed=5):
    rng = np.random.default_rng(seed)
    N = 2 * B
    data, _ = rows_for(ARCH_B, N, seed)
    sched = [(56, hidden, True), (hidden, 56, False)]
    params = O.init_params(sched, rng)
    bm, nmr, _ = O.corrupter_tables(ARCH_B, 1)
    mtu = np.stack([rng.permutation(len(bm)) for _ in range(N)]).astype(np.int32)
    idx = rng.permutation(N)[:B].astype(np.int32)
    _, fmask = O.get_masks(bm, nmr, mtu, 1, idx, 0)
    return dict(data=data, sched=sched, params=params, bm=bm, mtu=mtu, idx=idx, fmask=fmask, B=B)


def _rel_l2(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def test_bf16_first_step_matches_the_bf16_oracle():
    from codae.train import HipEmbeddingTrainer
    p = _problem_b_stack()
    t = HipEmbeddingTrainer(p["sched"], torch.tensor(p["data"]), torch.tensor(p["bm"]).to(torch.uint8), torch.tensor(p["mtu"]), 1e-3, 1e-4,
                            clip=1.0, max_batch=p["B"], precision="bf16", device=DEV, criterion=_vl(ARCH_B, WEIGHT_B))
    t.load_params(p["params"])
    eng = t.engine
    batch = t._batch(torch.tensor(p["idx"], device=DEV), 0)
    eng.step_forward_loss(batch, eng.hyper(1e-3, 1e-4, 1.0, global_rows=p["B"]))
    eng.step_backward(p["B"], 0, eng.L)
    torch.cuda.synchronize()
    x = p["data"][p["idx"]]
    relu = [r for _, _, r in p["sched"]]
    y, acts = O.forward(p["params"], relu, O.corrupt(x, p["fmask"]), keep=True, quant=O.bf16_round)
    want_loss = float(O.combined_mean(ARCH_B, WEIGHT_B, x, y))
    grads = O.backward(p["params"], relu, acts, O.combined_mean_grad_y(ARCH_B, WEIGHT_B, x, y), quant=O.bf16_round)
    loss = eng.read_scalars()[3]
    print("MEASURE variable loss bf16: loss %.7g oracle %.7g" % (loss, want_loss))
    assert abs(loss - want_loss) <= 1e-3 * want_loss
    for l, (gw, gb) in enumerate(grads):
        ew, eb = _rel_l2(eng.weight_grad(l).cpu().numpy(), gw), _rel_l2(eng.bias_grad(l).cpu().numpy(), gb)
        print("MEASURE variable loss bf16: layer %d dW rel L2 %.2e db rel L2 %.2e" % (l, ew, eb))
        assert ew <= 2e-3 and eb <= 2e-3, (l, ew, eb)
    assert close(eng.output_view(p["B"]).cpu().numpy(), y, rtol=1e-2, atol=1e-3)      # (bf16 operands; the bit-exact check is below)


# ---- 4. composition -----------------------------------------------------------------------------------------------------------------

EPS = 1e-5
LR, WD = 1e-3, 1e-4


def _dy_of(vl, x):
    """The criterion of the host restatements: VariableLoss.loss under float64 autograd."""
    def dy_of(y):
        ty = torch.tensor(np.asarray(y, dtype=np.float64), requires_grad=True)
        loss = vl.loss(torch.tensor(x.astype(np.float64)), ty)
        loss.backward()
        return ty.grad.numpy(), float(loss.detach())
    return dy_of


def _compose_problem():
    g = Golden("abalone_k2")
    m = g.meta
    p = dict(g=g, arch=m["arch"], weight=m["weight"], params=g.params("init"), acts=["relu" if r else None for r in g.relu_flags()],
             data=g["data"], idx=np.asarray(g.calls()[0][0]).astype(np.int32))
    _, p["fmask"] = O.get_masks(g["binary_masks"], g["nb_missing_per_run"], g["mask_to_use"], m["k_max"], p["idx"], 0)
    return p


def _compose_trainer(p, **kw):
    from codae.train import HipEmbeddingTrainer
    g = p["g"]
    sched = [(w.shape[1], w.shape[0], r) for (w, _), r in zip(p["params"], g.relu_flags())]
    kw.setdefault("criterion", _vl(p["arch"], p["weight"]))
    t = HipEmbeddingTrainer(sched, torch.tensor(p["data"]), torch.tensor(g["binary_masks"]).to(torch.uint8),
                            torch.tensor(g["mask_to_use"]).to(torch.int32), LR, WD, clip=1.0, max_batch=64, precision="f32", device=DEV, **kw)
    t.load_params(p["params"])
    return t


def _check_step(t, ref, p, c, factors=None, update=True):
    """tests/test_gpu_norm.py's check of one fp32 step: the loss, the norm, every gradient tensor, the parameters after the update"""
    eng = t.engine
    vl = eng.variable_loss
    x = p["data"][p["idx"]]
    ro = ref.step(c, _dy_of(vl, x), factors)
    t.train_batch(torch.tensor(p["idx"], device=DEV), run=0)
    _, _, gsq, loss = eng.read_scalars()
    print("MEASURE composition: loss", loss, ro["loss"], "gnorm", math.sqrt(gsq), ro["grad_norm"])
    assert close(loss, ro["loss"]), (loss, ro["loss"])
    assert close(math.sqrt(gsq), ro["grad_norm"]), (math.sqrt(gsq), ro["grad_norm"])
    for l, (gw, gb) in enumerate(ref.last_grads):
        ew, eb = max_err(eng.weight_grad(l).cpu().numpy(), gw), max_err(eng.bias_grad(l).cpu().numpy(), gb)
        assert ew <= 1.0 and eb <= 1.0, ("gradient", l, ew, eb)
    if update:
        for l, (w_, b_) in enumerate(ref.params):
            assert close(eng.weight(l).cpu().numpy(), w_), ("W", l)
            assert close(eng.bias(l).cpu().numpy(), b_), ("b", l)


def _ref(p, norms=None, tied=False):
    import norm_ref as NR
    L = len(p["params"])
    return NR.StepRef(p["params"], p["acts"], [0] * L, norms or [0] * L, "layer", EPS, LR, WD, tied=tied)


def test_composes_with_masking_noise():
    import noise_ref as NZ
    from codae.tool import InputNoise
    p = _compose_problem()
    t = _compose_trainer(p, input_noise=InputNoise("masking", p=0.25, seed=11))
    c = NZ.corrupt(p["data"][p["idx"]], p["idx"], 1, "masking", seed=11, p=0.25, keep=p["fmask"])
    assert (c != p["data"][p["idx"]] * p["fmask"]).sum() > 20
    _check_step(t, _ref(p), p, c)


def test_composes_with_hidden_dropout():
    from codae.tool import HiddenDropout
    p = _compose_problem()
    drop = HiddenDropout([0.0, 0.5, 0.0, 0.25, 0.0], seed=77)
    t = _compose_trainer(p, hidden_dropout=drop)
    factors = [drop.factor(p["idx"], l, 11, 1, n_layers=6) if pl > 0 else None for l, pl in enumerate([0.0, 0.5, 0.0, 0.25, 0.0])]
    x = p["data"][p["idx"]]
    _check_step(t, _ref(p), p, x * p["fmask"], factors)


def test_composes_with_layer_norm():
    from codae.tool import Norm
    p = _compose_problem()
    t = _compose_trainer(p, norm=Norm("layer", layers="hidden", eps=EPS))
    assert t.engine.norm_layers == [0, 1, 2, 3, 4]
    x = p["data"][p["idx"]]
    _check_step(t, _ref(p, norms=[1, 1, 1, 1, 1, 0]), p, x * p["fmask"])


def test_composes_with_tied_weights():
    p = _compose_problem()
    t = _compose_trainer(p, tied_weights=True)
    ref = _ref(p, tied=True)
    x = p["data"][p["idx"]]
    # (load_params mirrored the decoder matrices; the reference mirrors its own copy the same way)
    _check_step(t, ref, p, x * p["fmask"])


def test_composes_with_lamb():
    import trust_ref as TR
    from codae.tool import Optimizer
    from test_gpu_optimizer_kinds import read_state
    from test_gpu_trust import check_engine
    p = _compose_problem()
    tool = Optimizer("lamb")
    t = _compose_trainer(p, optimizer=tool)
    eng = t.engine
    before = read_state(eng)
    hp = eng.hyper(LR, WD, clip=1.0, global_rows=64, step=1)
    x = p["data"][p["idx"]]
    # the gradients of the step against the host restatement, the update as the float64 kind fed those gradients
    _check_step(t, _ref(p), p, x * p["fmask"], update=False)
    before["g"] = eng.grads.cpu().numpy().copy()
    ratios = check_engine(eng, before, hp, TR.trust_of(tool), "variable loss lamb")
    assert np.isfinite(ratios).all() and (ratios > 0).all()


def test_save_load_resume_is_bit_for_bit(tmp_path):
    from codae.tool import HiddenDropout, InputNoise
    p = _compose_problem()
    calls = p["g"].calls()
    mk = lambda: _compose_trainer(p, input_noise=InputNoise("masking", p=0.1, seed=3), hidden_dropout=HiddenDropout(0.25, seed=5))
    step = lambda t, s: t.train_batch(torch.tensor(np.asarray(calls[s][0]).astype(np.int32), device=DEV), run=calls[s][1])
    whole = mk()
    for s in range(3):
        step(whole, s)
    first = mk()
    step(first, 0)
    path = str(tmp_path / "ck.codae")
    first.save(path)
    second = mk()
    meta = second.load(path)
    assert meta["options"]["variable_loss"]["n_var"] == 9 and meta["options"]["variable_loss"]["io"] == 11
    for s in (1, 2):
        step(second, s)
    a, b = whole.state_digest(), second.state_digest()
    assert a == b, sorted(k for k in a if a[k] != b[k])
    assert torch.equal(_bits(whole.last_output()), _bits(second.last_output()))


def test_graph_replay_takes_the_criterion_on_its_own_only():
    """use_graph=True with any option of the step beside the criterion: the step is refused, naming the option, nothing is
    captured and nothing moves; on plain steps the same trainer settings run (the composition tests above)."""
    from codae.hip import HipError
    from codae.tool import HiddenDropout, InputNoise, Norm, Optimizer, Residual, SparseCode, WeightAverage
    p = _compose_problem()
    rows = torch.tensor(p["idx"], device=DEV)
    for kw, word in ((dict(input_noise=InputNoise("masking", p=0.25, seed=11)), "input noise"),
                     (dict(hidden_dropout=HiddenDropout(0.25, seed=5)), "hidden dropout"),
                     (dict(optimizer=Optimizer("adamw")), "optimizer"), (dict(optimizer=Optimizer("lamb")), "optimizer"),
                     (dict(residual=Residual([1])), "residual"), (dict(norm=Norm("layer", layers="hidden", eps=EPS)), "normalisation"),
                     (dict(sparse_code=SparseCode(4)), "sparse code"), (dict(tied_weights=True), "tied weights"),
                     (dict(weight_average=WeightAverage("ema", decay=0.9)), "weight average")):
        t = _compose_trainer(p, use_graph=True, **kw)
        before = t.state_digest()
        with pytest.raises(HipError, match=word):
            t.train_batch(rows, run=0)
        assert t.engine.graph_captures() == 0 and t.engine.step_count == 0 and t.state_digest() == before, word
    # the criterion alone replays (and Optimizer() is no setting)
    t = _compose_trainer(p, use_graph=True, optimizer=Optimizer())
    t.train_batch(rows, run=0)
    assert t.engine.graph_captures() == 1 and t.engine.step_count == 1


def test_output_view_of_a_bf16_stack_whose_widths_are_no_multiples_of_64():
    """Plain mean squared error, bf16, 56 -> 24 -> 56: the work space pads every activation row to 64 columns, and output_view /
    last_output must find y behind them - bit for bit what the same forward hands to the caller."""
    from codae.hip import HipError
    from codae.train import HipEmbeddingTrainer
    p = _problem_b_stack()
    t = HipEmbeddingTrainer(p["sched"], torch.tensor(p["data"]), torch.tensor(p["bm"]).to(torch.uint8), torch.tensor(p["mtu"]), 1e-3, 1e-4,
                            clip=1.0, max_batch=p["B"], precision="bf16", device=DEV)
    t.load_params(p["params"])
    rows = torch.tensor(p["idx"], device=DEV)
    want = t.eval_batch(rows, run=0, want_y=True).clone()
    assert float(want.abs().max()) > 0
    t.engine.acts.zero_()
    t.eval_batch(rows, run=0)                       # (y stays in the work space)
    assert torch.equal(_bits(t.engine.output_view(p["B"]).contiguous()), _bits(want))
    # the plain bf16 training step never stores y, and says so; with the criterion on it does
    assert not t.engine.step_stores_output(p["B"])
    t.train_batch(rows, run=0)
    with pytest.raises(HipError, match="did not store"):
        t.last_output()
    t.set_criterion(_vl(ARCH_B, WEIGHT_B))
    assert t.engine.step_stores_output(p["B"])
    t.train_batch(rows, run=0)
    x = p["data"][p["idx"]]
    y = t.last_output().cpu().numpy()
    assert y.shape == x.shape and close(t.engine.read_scalars()[3], O.combined_mean(ARCH_B, WEIGHT_B, x, y))


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------

def test_what_assumes_equal_width_slots_is_refused_and_the_trainer_stays_usable():
    from codae.hip import HipError
    from codae.tool import InputNoise, LossEmphasis, ReconstructionLoss, SlotContrast, SlotPresence
    from codae.train import HipEmbeddingTrainer
    p = _compose_problem()
    t = _compose_trainer(p, n_slots=11)
    twin = _compose_trainer(p, n_slots=11)
    pres = np.ones((len(p["data"]), 11), dtype=np.uint8); pres[3, 2] = 0
    for what, word in ((lambda: t.set_loss_emphasis(LossEmphasis(3.0, 1.0)), "loss emphasis"),
                       (lambda: t.set_criterion(ReconstructionLoss("l1")), "reconstruction loss"),
                       (lambda: t.set_contrast(SlotContrast(negatives=8)), "slot contrast"),
                       (lambda: t.set_presence(SlotPresence(pres)), "slot-presence"),
                       (lambda: t.set_input_noise(InputNoise("swap", p=0.3, seed=1)), "swap noise")):
        with pytest.raises(HipError, match=word):
            what()
    with pytest.raises(HipError, match="data parallel"):
        _compose_trainer(p, distributed=True)
    for name in ("complete", "retrieval_metrics", "score_outfits", "complete_items", "compatibility_metrics", "encode_items", "code_index"):
        with pytest.raises(HipError, match="embedding-slot feature"):
            getattr(t, name)(*([None] * {"complete": 3, "complete_items": 3}.get(name, 1)))
    # ... and the other way round: the criterion is refused while such an option is on
    for kw, word in ((dict(loss_emphasis=LossEmphasis(3.0, 1.0)), "loss emphasis"), (dict(presence=SlotPresence(pres)), "slot-presence"),
                     (dict(contrast=SlotContrast(negatives=8)), "slot contrast"),
                     (dict(input_noise=InputNoise("swap", p=0.3, seed=1)), "swap noise")):
        other = _compose_trainer(p, n_slots=11, criterion=None, **kw)
        with pytest.raises(HipError, match=word):
            other.set_criterion(_vl(p["arch"], p["weight"]))
    other = _compose_trainer(p, n_slots=11, criterion=ReconstructionLoss("l1"))
    with pytest.raises(HipError, match="reconstruction loss"):
        other.set_criterion(_vl(p["arch"], p["weight"]))
    with pytest.raises(HipError, match="cover 56 columns"):
        t.set_criterion(_vl(ARCH_B, WEIGHT_B))
    # last_output before any step
    with pytest.raises(HipError, match="no train_batch"):
        t.last_output()
    # the refusals changed nothing: the trainer steps as its untouched twin, bit for bit
    rows = torch.tensor(p["idx"], device=DEV)
    t.train_batch(rows, run=0); twin.train_batch(rows, run=0)
    assert t.state_digest() == twin.state_digest()
    assert t.last_output().shape == (64, 11)
    # the plain bf16 step keeps its reconstruction to itself
    g = Golden("embedding_square")
    m = g.meta
    sched = [(w.shape[1], w.shape[0], r) for (w, _), r in zip(g.params("init"), g.relu_flags())]
    plain = HipEmbeddingTrainer(sched, torch.tensor(g["data"]), torch.tensor(g["binary_masks"]).to(torch.uint8),
                                torch.tensor(g["mask_to_use"]).to(torch.int32), 1e-3, 1e-4, max_batch=m["batch"], precision="bf16", device=DEV)
    plain.load_params(g.params("init"))
    idx, run = g.calls()[0]
    plain.train_batch(torch.tensor(np.asarray(idx).astype(np.int32), device=DEV), run=run)
    with pytest.raises(HipError, match="did not store"):
        plain.last_output()
