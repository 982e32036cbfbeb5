"""Tied encoder / decoder weights on a real MI355X (include/codae_hip.h, "Tied weights").

  A. the two kernels alone, exact: codae_tie_fold against g_l + g_l'.T formed by torch in fp32, codae_tie_mirror against the
     transposes and torch's .bfloat16(), a poison pattern everywhere else.
  B. the fused step: the gradient a tied step consumes is TiedWeights.fold of what the untied step of the same state leaves, bit
     for bit; the invariants of the tie after five steps in every step form; the update against the float64 optimizers of
     tests/optim_ref.py fed the folded gradients; the fp32 and bf16 engines against the tied torch model of tests/tied_ref.py.
  C. off is off, the refusals, init / load, and the training script.

Shapes (the smallest at which every path is taken): the 6-layer 192 / 128 / 64 taper at batch 72; 3 slots x 24 (io 72), code 40,
batch 48 - partial tiles everywhere; 10 x 192 square at batch 64 - the persistent chain kernel.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import optim_ref as OR
import tied_ref as TR

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, WD = 1e-3, 1e-4

# (slots, slot width, code, layers per side, batch)
SHAPES = {"taper": (3, 64, 64, 2, 72), "partial": (3, 24, 40, 2, 48), "chain": (3, 64, 192, 4, 64)}


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous().view(torch.int16)


class Problem:
    def __init__(self, name):
        from oracle import dae_oracle as O
        S, E, z, nl, B = SHAPES[name]
        self.S, self.E, self.B, self.io = S, E, B, S * E
        self.sched = O.layer_schedule(self.io, z, nl, nl, False, "embedding")
        rng = np.random.default_rng(sorted(SHAPES).index(name) + 40)
        self.data = rng.random((B + 40, self.io), dtype=np.float32)
        self.bm, _, _ = O.corrupter_tables([{"size": E, "position": s * E} for s in range(S)], 1)
        self.mtu = rng.integers(0, S, (B + 40, 1)).astype(np.int32)
        self.rows = rng.permutation(B + 40)[:B].astype(np.int32)
        self.mid = self.mtu[self.rows, 0]
        self.fmask = self.bm[self.mid]
        self.params = TR.tied_init(self.sched, 7 + sorted(SHAPES).index(name))
        self.order = [rng.permutation(B + 40)[:B].astype(np.int32) for _ in range(5)]

    def engine(self, prec, tied, optimizer=None):
        from codae.hip.engine import DaeEngine
        eng = DaeEngine(self.sched, self.B, prec, DEV)
        assert (eng.w_off, eng.b_off, eng.n_param) == TR.flat_layout(self.sched)
        if optimizer is not None:
            eng.set_optimizer(optimizer)
        if tied:
            eng.set_tied_weights(True)
        eng.load_params(self.params)
        return eng

    def batch(self, eng):
        dev = lambda a, dt: torch.tensor(a, dtype=dt, device=DEV)
        return eng.make_batch(dev(self.data, torch.float32), dev(self.rows, torch.int32), dev(self.mid, torch.int32),
                              dev(self.bm, torch.uint8))

    def trainer(self, prec="bf16", clip=1.0, **kw):
        from codae.train import HipEmbeddingTrainer
        tr = HipEmbeddingTrainer(self.sched, torch.tensor(self.data), torch.tensor(self.bm).to(torch.uint8), torch.tensor(self.mtu), LR, WD,
                                 clip, max_batch=self.B, precision=prec, device=DEV, **kw)
        tr.load_params(self.params)
        return tr


@functools.lru_cache(maxsize=None)
def problem(name):
    """Built once per shape and left unchanged."""
    return Problem(name)


def pair_views(eng, flat, l, m):
    """(encoder range as [out][in], decoder range as [in][out]) of a flat tensor in the parameter layout."""
    k, n, _ = eng.schedule[l]
    return flat[eng.w_off[l]:eng.w_off[l] + n * k].view(n, k), flat[eng.w_off[m]:eng.w_off[m] + n * k].view(k, n)


def assert_tied_state(eng, what):
    """Every decoder matrix and both its shadows are the mirror of the encoder's, bit for bit."""
    from codae.tool import TiedWeights
    torch.cuda.synchronize()
    p = eng.params
    for l, m in TiedWeights.pairs(eng.schedule):
        enc, dec = pair_views(eng, p, l, m)
        assert torch.equal(bits(dec), bits(enc.t().contiguous())), "%s: W_%d is not W_%d transposed" % (what, m, l)
        if eng.shadow is not None:
            s_enc, s_dec = pair_views(eng, eng.shadow[:eng.n_param], l, m)
            assert torch.equal(bits(s_dec), bits(dec.bfloat16())), "%s: shadow of layer %d" % (what, m)
            assert torch.equal(bits(s_dec), bits(s_enc.t().contiguous())), "%s: shadow of layer %d against layer %d's" % (what, m, l)
            k, n, _ = eng.schedule[l]
            t_dec = eng.shadow_t[eng.w_off[m]:eng.w_off[m] + n * k].view(n, k)        # (W_m)^T, laid out as W_l
            assert torch.equal(bits(t_dec), bits(s_enc)), "%s: transposed shadow of layer %d" % (what, m)
    if eng.shadow is not None:
        assert torch.equal(bits(eng.shadow[:eng.n_param]), bits(p.bfloat16())), "%s: the shadow is not params.bfloat16()" % what


# ---- A. the kernels ----------------------------------------------------------------------------------------------------------
KERNEL_CASES = {
    "four": ([(136, 192), (72, 136), (40, 72), (8, 16)], 0),
    "many": ([(64, 64)] * 64, 0),
    "mixed": ([(40, 72), (136, 8)], 24 * 24),             # a non-square pair list around a middle matrix no pair names
    "ragged": ([(7, 5), (33, 65)], 9),                    # no multiple of 4 anywhere: the element-wise instantiations (fp32 only)
}


def kernel_layout(shapes, middle):
    """[(enc_off, dec_off, rows, cols)], n: encoders, the middle range, decoders in mirror order, each padded to 64, 64 in front."""
    pad = lambda n: (n + 63) // 64 * 64
    off, enc = 64, []
    for r, c in shapes:
        enc.append(off)
        off += pad(r * c)
    off += pad(middle)
    dec = [0] * len(shapes)
    for i in reversed(range(len(shapes))):
        dec[i] = off
        off += pad(shapes[i][0] * shapes[i][1])
    return [(e, d, r, c) for e, d, (r, c) in zip(enc, dec, shapes)], off + 64


@pytest.mark.parametrize("case", sorted(KERNEL_CASES))
def test_tie_fold_kernel_is_exact_and_touches_nothing_else(case):
    from codae.hip.engine import tie_fold
    shapes, middle = KERNEL_CASES[case]
    pairs, n = kernel_layout(shapes, middle)
    gen = torch.Generator().manual_seed(len(shapes) + middle)
    g0 = (torch.randn(n, generator=gen) * 10.0 ** torch.randint(-6, 3, (n,), generator=gen).float()).to(DEV)   # (padding and middle too: the poison)
    g0[pairs[0][0]] = -0.0
    g0[pairs[0][1]] = -0.0                                # (-0) + (-0) = -0 in the encoder; the decoder becomes +0
    want = g0.clone()
    for e, d, r, c in pairs:
        want[e:e + r * c].view(r, c).copy_(g0[e:e + r * c].view(r, c) + g0[d:d + r * c].view(c, r).t())
        want[d:d + r * c] = 0.0
    got = g0.clone()
    tie_fold(got, pairs)
    torch.cuda.synchronize()
    assert torch.equal(bits(got), bits(want)), case
    for e, d, r, c in pairs:
        assert not bool(torch.signbit(got[d:d + r * c]).any()), "decoder range is not +0"
    assert bool(torch.signbit(got[pairs[0][0]]))
    touched = torch.zeros(n, dtype=torch.bool, device=DEV)
    for e, d, r, c in pairs:
        touched[e:e + r * c] = True
        touched[d:d + r * c] = True
    assert torch.equal(bits(got[~touched]), bits(g0[~touched])) and int((~touched).sum()) >= 128 + middle


@pytest.mark.parametrize("with_shadows", (True, False), ids=("shadows", "fp32-only"))
@pytest.mark.parametrize("case", sorted(KERNEL_CASES))
def test_tie_mirror_kernel_is_exact_and_touches_nothing_else(case, with_shadows):
    from codae.hip import HipError
    from codae.hip.engine import tie_mirror
    shapes, middle = KERNEL_CASES[case]
    pairs, n = kernel_layout(shapes, middle)
    gen = torch.Generator().manual_seed(17 + len(shapes))
    p0 = (torch.randn(n, generator=gen) * 10.0 ** torch.randint(-6, 3, (n,), generator=gen).float()).to(DEV)
    poison = lambda: torch.randint(-30000, 30000, (n,), generator=gen, dtype=torch.int16).to(DEV).view(torch.bfloat16)
    s0, t0 = poison(), poison()
    p, s, t = p0.clone(), s0.clone(), t0.clone()
    if with_shadows and case == "ragged":
        with pytest.raises(HipError, match="multiples of 8"):
            tie_mirror(p, pairs, s, t)
        torch.cuda.synchronize()
        assert torch.equal(bits(p), bits(p0)) and torch.equal(bits(s), bits(s0))         # refused before any launch
        return
    tie_mirror(p, pairs, s if with_shadows else None, t if with_shadows else None)
    torch.cuda.synchronize()
    want = p0.clone()
    dec_mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    for e, d, r, c in pairs:
        want[d:d + r * c].view(c, r).copy_(p0[e:e + r * c].view(r, c).t())
        dec_mask[d:d + r * c] = True
    assert torch.equal(bits(p), bits(want)), case                       # the fp32 mirror; everything else as it was
    if not with_shadows:
        assert torch.equal(bits(s), bits(s0)) and torch.equal(bits(t), bits(t0))
        return
    for e, d, r, c in pairs:
        sd = s[d:d + r * c]
        assert torch.equal(bits(sd), bits(p[d:d + r * c].bfloat16())), "shadow"            # the rounding of params.bfloat16()
        assert torch.equal(bits(t[d:d + r * c].view(r, c)), bits(sd.view(c, r).t().contiguous())), "transposed shadow"
        assert torch.equal(bits(t[d:d + r * c]), bits(p0[e:e + r * c].bfloat16()))
    assert torch.equal(bits(s[~dec_mask]), bits(s0[~dec_mask])) and torch.equal(bits(t[~dec_mask]), bits(t0[~dec_mask]))


def test_tie_kernels_refuse_bad_pair_lists():
    from codae.hip import HipError
    from codae.hip.engine import tie_fold, tie_mirror
    g = torch.zeros(1024, device=DEV)
    for bad in ([(0, 32, 8, 8)], [(0, 512, 8, 8), (520, 256, 8, 8)], [(0, 64, 0, 8)], [(-64, 64, 8, 8)]):
        with pytest.raises(HipError):
            tie_fold(g, bad)
        with pytest.raises(HipError):
            tie_mirror(g, bad)


# ---- B. the fused step -------------------------------------------------------------------------------------------------------
def step_once(p, prec, tied, clip=1.0):
    eng = p.engine(prec, tied)
    batch = p.batch(eng)
    eng.train_step(batch, eng.hyper(LR, WD, clip=clip, global_rows=p.B))
    torch.cuda.synchronize()
    return eng


@pytest.mark.parametrize("name,prec,chain", [("taper", "bf16", None), ("taper", "f32", None), ("partial", "bf16", None),
                                             ("partial", "f32", None), ("chain", "bf16", True), ("chain", "bf16", False),
                                             ("chain", "f32", None)])
def test_tied_step_consumes_the_fold_of_the_untied_gradients(monkeypatch, name, prec, chain):
    """An untied and a tied engine from the same tied state, forward + backward on the same batch: the same GEMMs, plus one add.
    chain: the persistent chain kernel against the per-layer launches (CODAE_NO_CHAIN, as test_chain_step_equals_per_layer_step)."""
    from codae.tool import TiedWeights
    if chain is False:
        monkeypatch.setenv("CODAE_NO_CHAIN", "1")
    else:
        monkeypatch.delenv("CODAE_NO_CHAIN", raising=False)
    p = problem(name)
    untied, tied = step_once(p, prec, False), step_once(p, prec, True)
    if chain is not None:
        assert untied.step_path(p.B) == ("chain" if chain else "layers")
    assert tied.step_path(p.B) == untied.step_path(p.B)                  # tying never changes the path
    want = TiedWeights.fold(untied.grads, p.sched, untied.w_off)
    assert float(untied.grads.abs().max()) > 0
    for l, m in TiedWeights.pairs(p.sched):
        assert float(pair_views(untied, untied.grads, l, m)[1].abs().max()) > 0      # there was something to fold
    assert torch.equal(bits(tied.grads), bits(want)), (name, prec, chain)
    assert_tied_state(tied, "%s %s after one step" % (name, prec))
    # the two engines' losses are the same number: the forward is untouched
    assert tied.read_scalars()[3] == untied.read_scalars()[3]


def _dist_env(monkeypatch, port):
    monkeypatch.setenv("CODAE_DP_FORCE_ALLREDUCE", "1")
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1"); monkeypatch.setenv("MASTER_PORT", str(port))
    monkeypatch.setenv("RANK", "0"); monkeypatch.setenv("WORLD_SIZE", "1")


def _five_steps(p, prec, poison, **kw):
    """Five steps of a tied trainer; the decoder ranges of both moments hold `poison` beforehand.  Returns the engine's state."""
    from codae.tool import TiedWeights
    tr = p.trainer(prec, tied_weights=True, **kw)
    eng = tr.engine
    for _, m in TiedWeights.pairs(p.sched):
        k, n, _r = p.sched[m]
        eng.adam_m[eng.w_off[m]:eng.w_off[m] + n * k] = poison
        eng.adam_v[eng.w_off[m]:eng.w_off[m] + n * k] = poison
    for idx in p.order:
        tr.train_batch(torch.tensor(idx, dtype=torch.int32, device=DEV), run=0)
    what = "%s %s" % (prec, kw)
    assert_tied_state(eng, what)
    for _, m in TiedWeights.pairs(p.sched):
        k, n, _r = p.sched[m]
        for name, t in (("adam_m", eng.adam_m), ("adam_v", eng.adam_v)):
            assert bool((t[eng.w_off[m]:eng.w_off[m] + n * k] == poison).all()), "%s: %s of decoder layer %d was written" % (what, name, m)
    if kw.get("use_graph"):
        assert eng.graph_captures() == 1, what
    out = [eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone(), eng.read_scalars()]
    if eng.shadow is not None:
        out += [eng.shadow.clone(), eng.shadow_t.clone()]
    return out


def _same(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        if torch.is_tensor(x):
            assert torch.equal(bits(x), bits(y)), (what, i)
        else:
            assert x == y, (what, x, y)


@pytest.mark.parametrize("name,prec", [("taper", "bf16"), ("partial", "bf16"), ("chain", "bf16"), ("partial", "f32")])
def test_tie_holds_after_five_steps_in_every_step_form(monkeypatch, name, prec):
    """plain, graph replay, one-rank torch.distributed and one-rank native data parallel: the tie, the untouched decoder moments,
    one capture, and identical bits (on the per-layer launches, which every form can take; then plain against graph replay on
    whichever path the shape takes by itself)."""
    import torch.distributed as dist
    from codae.train import init_rccl_process_group
    p = problem(name)
    _dist_env(monkeypatch, 29551)
    monkeypatch.setenv("CODAE_NO_CHAIN", "1")
    init_rccl_process_group(torch.device(DEV))
    try:
        legs = [dict(), dict(use_graph=True), dict(distributed=True), dict(distributed=True, native_dp=True)]
        outs = [_five_steps(p, prec, 3.25, **kw) for kw in legs]
        for kw, o in zip(legs[1:], outs[1:]):
            _same(outs[0], o, (name, prec, kw))
    finally:
        dist.destroy_process_group()
    monkeypatch.delenv("CODAE_NO_CHAIN")
    if prec == "bf16":
        a, b = _five_steps(p, prec, 3.25), _five_steps(p, prec, 3.25, use_graph=True)
        _same(a, b, (name, prec, "own path"))
        if name == "chain":
            assert p.trainer(prec, tied_weights=True).engine.step_path(p.B) == "chain"


def _opt_cases():
    from codae.tool import LRSchedule, Optimizer
    return {"adam": None,
            "adamw-cosine": Optimizer("adamw", schedule=LRSchedule("cosine", warmup=2, total=50, min_factor=0.1)),
            "sgd-nesterov": Optimizer("sgd", momentum=0.9, nesterov=True)}


@pytest.mark.parametrize("branch", ("on", "off"))
@pytest.mark.parametrize("kind", ("adam", "adamw-cosine", "sgd-nesterov"))
@pytest.mark.parametrize("name,prec", [("taper", "bf16"), ("partial", "bf16"), ("chain", "bf16"), ("partial", "f32")])
def test_tied_update_is_the_optimizer_of_its_own_inputs(name, prec, kind, branch):
    """The second step of a tied engine: the free parameters and their moments against the float64 update of tests/optim_ref.py
    (adam_ref's bounds underneath) fed the folded gradients the step consumed and the state cloned before it; the norm the step
    reports is that of the folded vector (1e-6 of the float64 sum); clip triggering and not."""
    from codae.tool import TiedWeights
    p = problem(name)
    tool = _opt_cases()[kind]
    o = OR.opt() if tool is None else OR.opt_of(tool)
    eng = p.engine(prec, True, optimizer=tool)
    batch = p.batch(eng)
    eng.train_step(batch, eng.hyper(LR, WD, clip=1.0, global_rows=p.B))
    norm1 = eng.read_scalars()[2] ** 0.5
    clip = norm1 * (0.25 if branch == "on" else 64.0)      # (the second step's norm is within a few percent of the first's)
    before = {k: t.clone().cpu().numpy() for k, t in (("p", eng.params), ("m", eng.adam_m), ("v", eng.adam_v))}
    hp = eng.hyper(LR, WD, clip=clip, global_rows=p.B)
    assert hp.step == 2
    eng.train_step(batch, hp)
    torch.cuda.synchronize()
    g = eng.grads.cpu().numpy()
    got = {"p": eng.params.cpu().numpy(), "m": eng.adam_m.cpu().numpy(), "v": eng.adam_v.cpu().numpy(), "vmax": None}
    gsq = eng.read_scalars()[2]
    want_sq = float((g.astype(np.float64) ** 2).sum())
    print("MEASURE tied %s %s %s clip %s: reported sum g^2 %.17g float64 %.17g rel %.3g" % (name, prec, kind, branch, gsq, want_sq,
                                                                                            abs(gsq - want_sq) / want_sq))
    assert abs(gsq - want_sq) <= 1e-6 * want_sq
    for l, m in TiedWeights.pairs(p.sched):
        k, n, _ = p.sched[m]
        assert not g[eng.w_off[m]:eng.w_off[m] + n * k].any()                              # the folded vector
    coef = OR.clip_coef32(gsq, clip)
    assert (coef < 1) == (branch == "on"), coef
    live = TR.free_mask(p.sched)
    h = OR.hyper_of_struct(hp)
    args = (before["p"][live], g[live], before["m"][live], before["v"][live] if o.kind != "sgd" else None, None, h, o, coef)
    want, tol = OR.step64(*args), OR.bounds(*args)
    ratios = OR.worst_ratios({k: (None if got[k] is None else got[k][live]) for k in OR.KEYS}, want, tol)
    print("MEASURE tied %s %s %s clip %s: worst |error| / bound %s" % (name, prec, kind, branch, ratios))
    assert all(r <= 1.0 for r in ratios.values()), ratios
    # everything that is not free: moments untouched, the decoder matrices the mirror of the new encoder, padding zero
    for k in ("m", "v"):
        assert np.array_equal(got[k][~live], before[k][~live]), k
    assert_tied_state(eng, "%s %s %s" % (name, prec, kind))
    if o.kind == "sgd":
        assert np.array_equal(got["v"], before["v"])


def _rel_l2(got, want):
    return float(np.linalg.norm(got.astype(np.float64) - want) / np.linalg.norm(want))


def _free_tensors(sched, flat):
    """{name: array} of the free tensors of a flat vector."""
    w_off, b_off, _ = TR.flat_layout(sched)
    out = {}
    for l, s in enumerate(sched):
        if l < TR.n_free(len(sched)):
            out["W%d" % l] = flat[w_off[l]:w_off[l] + s[0] * s[1]]
        out["b%d" % l] = flat[b_off[l]:b_off[l] + s[1]]
    return out


def test_fp32_engine_follows_the_torch_tied_model():
    """Three steps at the taper shape against TiedModel in float64 under clip_grad_norm_ + torch.optim.Adam: loss, gradient norm,
    the folded first-step gradients and the final parameters within BASELINE's rtol 1e-3 / atol 1e-5."""
    p = problem("taper")
    model = TR.TiedModel(p.sched, p.params)
    opt = torch.optim.Adam(model.parameters(), lr=LR, weight_decay=WD)
    eng = p.engine("f32", True)
    batch = p.batch(eng)
    x, fm = torch.tensor(p.data[p.rows], dtype=torch.float64), torch.tensor(p.fmask, dtype=torch.float64)
    for step in range(3):
        opt.zero_grad()
        loss = model.loss(x, fm)
        loss.backward()
        g_ref = model.flat_grads().numpy()
        norm = float(torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0))
        opt.step()
        eng.train_step(batch, eng.hyper(LR, WD, clip=1.0, global_rows=p.B))
        torch.cuda.synchronize()
        _, _, gsq, got_loss = eng.read_scalars()
        print("MEASURE tied fp32 step %d: loss %.9g (torch %.9g) norm %.9g (torch %.9g)" % (step, got_loss, float(loss), gsq ** 0.5, norm))
        assert np.allclose(got_loss, float(loss.detach()), rtol=1e-3, atol=1e-5)
        assert np.allclose(gsq ** 0.5, norm, rtol=1e-3, atol=1e-5)
        if step == 0:
            assert np.allclose(eng.grads.cpu().numpy(), g_ref, rtol=1e-3, atol=1e-5)
    assert np.allclose(eng.params.cpu().numpy(), model.flat_params().numpy(), rtol=1e-3, atol=1e-5)
    assert_tied_state(eng, "fp32 against torch")


# (worst relative L2 error of a free tensor's folded first-step gradient, relative error of the loss) of the bf16 engine against the
# bf16-rounded float64 run of tests/tied_ref.py, measured on an MI355X, per shape (the worst tensor: b0, b5, b0); each shape
# asserts twice its own measured values
BF16_MEASURED = {"chain": (1.352e-4, 1.936e-7), "partial": (9.475e-8, 1.328e-8), "taper": (3.433e-5, 1.879e-9)}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_bf16_engine_follows_the_bf16_rounded_tied_model(name):
    p = problem(name)
    model = TR.TiedModel(p.sched, p.params, bf16=True)
    x, fm = torch.tensor(p.data[p.rows], dtype=torch.float64), torch.tensor(p.fmask, dtype=torch.float64)
    loss = model.loss(x, fm)
    loss.backward()
    want = _free_tensors(p.sched, model.flat_grads().numpy())
    eng = step_once(p, "bf16", True)
    got = _free_tensors(p.sched, eng.grads.cpu().numpy())
    errs = {k: _rel_l2(got[k], want[k]) for k in want}
    loss_err = abs(eng.read_scalars()[3] - float(loss.detach())) / float(loss.detach())
    worst = max(errs, key=errs.get)
    print("MEASURE tied bf16 %s: worst relative L2 of a folded gradient tensor %.4g (%s), loss relative error %.4g" % (
        name, errs[worst], worst, loss_err))
    grad_measured, loss_measured = BF16_MEASURED[name]
    assert errs[worst] <= 2 * grad_measured, (worst, errs[worst])
    assert loss_err <= 2 * loss_measured, loss_err


# ---- C. off, refusals, init / load, the script -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("partial", "chain"))
def test_off_is_off(name):
    """tied_weights=False / None against no argument: identical bits after three steps (an untied random state), plain and chain paths."""
    from oracle import dae_oracle as O
    p = problem(name)
    params = O.init_params(p.sched, np.random.default_rng(5))
    outs = []
    for kw in (dict(), dict(tied_weights=None), dict(tied_weights=False)):
        tr = p.trainer("bf16", **kw)
        tr.load_params(params)
        if name == "chain":
            assert tr.engine.step_path(p.B) == "chain"
        for idx in p.order[:3]:
            tr.train_batch(torch.tensor(idx, dtype=torch.int32, device=DEV), run=0)
        eng = tr.engine
        assert not eng.tied_weights
        outs.append([eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone(), eng.grads.clone(), eng.shadow.clone(), eng.shadow_t.clone(),
                     eng.read_scalars()])
    _same(outs[0], outs[1], "None")
    _same(outs[0], outs[2], "False")
    w = [outs[0][0][tr.engine.w_off[l]] for l in range(len(p.sched))]
    assert len(set(float(v) for v in w)) > 1                              # (and the state is not tied by accident)


def test_refusals_name_the_pair_and_leave_the_engine_usable():
    from codae.hip import HipError
    from codae.hip.engine import DaeEngine
    from codae.train import HipEmbeddingTrainer
    from oracle import dae_oracle as O
    p = problem("partial")
    sched = [(72, 72, True), (72, 40, False), (40, 72, False)]            # layers 0 and 2: 72 -> 72 against 40 -> 72
    eng = DaeEngine(sched, p.B, "bf16", DEV)
    with pytest.raises(HipError, match=r"tied weights: layers 0 and 2 are not mirror images \(72 -> 72 against 40 -> 72\)"):
        eng.set_tied_weights(True)
    assert not eng.tied_weights
    eng.load_params(O.init_params(sched, np.random.default_rng(1)))
    eng.train_step(p.batch(eng), eng.hyper(LR, WD, clip=1.0, global_rows=p.B))
    torch.cuda.synchronize()
    assert np.isfinite(eng.read_scalars()[3]) and eng.read_scalars()[3] > 0
    with pytest.raises(HipError, match="are not mirror images"):
        HipEmbeddingTrainer(sched, torch.tensor(p.data), torch.tensor(p.bm).to(torch.uint8), torch.tensor(p.mtu), LR, WD, 1.0,
                            max_batch=p.B, precision="bf16", device=DEV, tied_weights=True)
    # the sharded update: refused by the trainer, and by the library's span update itself
    with pytest.raises(HipError, match=r"tied weights: the sharded update is not supported: the tied layers 0 and 5"):
        p.trainer("bf16", tied_weights=True, distributed=True, sharded_update=True)
    eng = p.engine("bf16", True)
    batch = p.batch(eng)
    hp = eng.hyper(LR, WD, clip=1.0, global_rows=p.B)
    eng.step_forward_loss(batch, hp)
    eng.step_backward(p.B, 0, eng.L)
    acc = eng.new_accumulator()
    eng.span_sumsq(0, eng.n_param, acc)
    with pytest.raises(HipError, match=r"tied weights: the sharded update is not supported: the tied layers 0 and 5"):
        eng.step_update_span(hp, 0, eng.n_param, acc)
    eng.step_update(hp)                                                   # usable afterwards: the phased step ends as the fused one
    fused = step_once(p, "bf16", True)
    assert torch.equal(bits(eng.params), bits(fused.params))
    assert_tied_state(eng, "after a refused span update")


def test_init_and_load_keep_the_encoder_and_mirror_the_decoder():
    from oracle import dae_oracle as O
    p = problem("partial")
    a, b = p.trainer("bf16"), p.trainer("bf16", tied_weights=True)
    a.init_params(seed=123); b.init_params(seed=123)
    free = torch.from_numpy(TR.free_mask(p.sched)).to(DEV)
    assert torch.equal(bits(a.engine.params[free]), bits(b.engine.params[free]))          # the untied init's bits
    assert_tied_state(b.engine, "init_params")
    loose = O.init_params(p.sched, np.random.default_rng(2))             # a decoder of its own: overwritten
    b.load_params(loose)
    assert_tied_state(b.engine, "load_params")
    for l in range(TR.n_free(len(p.sched))):
        assert np.array_equal(b.engine.weight(l).cpu().numpy(), loose[l][0])
    assert not np.array_equal(b.engine.weight(len(p.sched) - 1).cpu().numpy(), loose[-1][0])
    ws = [w for w, _ in b.params()]
    assert torch.equal(ws[-1], ws[0].t())
    y = b.eval_batch(torch.tensor(p.rows, dtype=torch.int32, device=DEV), run=0, want_y=True)         # the forward reads the mirrors
    ref = O.forward([(w.cpu().numpy(), bb.cpu().numpy()) for w, bb in b.params()], [r for _, _, r in p.sched],
                    O.corrupt(p.data[p.rows], p.bm[p.mtu[p.rows, 0]]), quant=O.bf16_round)
    assert np.allclose(y.cpu().numpy(), ref, rtol=2e-2, atol=2e-2)
    # f32 engine: the same through the fp32 image alone
    c = p.trainer("f32", tied_weights=True)
    c.load_params(loose)
    assert_tied_state(c.engine, "load_params f32")


def test_embedding_script_with_tied_weights(tmp_path):
    import yaml
    E, z = 64, 64
    rng = np.random.default_rng(1)
    cats = ["top", "bottom", "shoe"]
    centers = rng.standard_normal((5, 3 * E)).astype(np.float32)
    emb = {}
    for i in range(200):
        v = centers[i % 5] + 0.1 * rng.standard_normal(3 * E).astype(np.float32)
        emb["o%04d" % i] = {c: v[s * E:(s + 1) * E].tolist() for s, c in enumerate(cats)}
    (tmp_path / "emb.json").write_text(json.dumps(emb))
    cfg = {"MODEL": {"Z_SIZE": z, "BATCH_SIZE": 64, "NB_INPUT_LAYER": 2, "NB_OUTPUT_LAYER": 2, "STEEP_LAYER_SIZE": False,
                     "EPOCH": 1, "LEARNING_RATE": 1e-3, "WEIGHT_DECAY": 1e-4, "NB_CORRUPTED": 1, "TRUNK_GRAD": True},
           "DATASET": {"NAME": "EMBEDDING", "USED_CATEGORY": cats, "EMBEDDING_SIZE": E, "SHUFFLE": True, "SPLIT": [0.7, 0.3]},
           "SEED": 27493045, "HIP": {"TIED_WEIGHTS": True}}
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    os.makedirs(tmp_path / "log")
    script = os.path.join(ROOT, "mui-deepautoencoder_amd", "script", "train_dae_on_embedding.py")
    # the script run as a program (runpy, its own argv) in a child process; the probe keeps the trainer it builds and, after main()
    # returns, compares every decoder matrix with its encoder matrix transposed
    probe = (
        "import runpy, sys, torch\n"
        "import codae.train as T\n"
        "made = []\n"
        "class Spy(T.HipEmbeddingTrainer):\n"
        "    def __init__(self, *a, **kw):\n"
        "        super().__init__(*a, **kw)\n"
        "        made.append(self)\n"
        "T.HipEmbeddingTrainer = Spy\n"
        "sys.argv = [%r, '--embedding_path', 'emb.json', '--output_path', 'out', '--config', 'cfg.yaml', '--precision', 'bf16']\n"
        "runpy.run_path(sys.argv[0], run_name='__main__')\n"
        "tr = made[-1]\n"
        "ws = [w for w, _ in tr.params()]\n"
        "L = len(ws)\n"
        "print('PROBE tied', tr.engine.tied_weights, all(torch.equal(ws[L - 1 - l], ws[l].t()) for l in range(L // 2)),\n"
        "      bool((ws[0] != 0).any()), tr.engine.step_count)\n" % script)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "mui-deepautoencoder_amd"), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", probe], cwd=str(tmp_path), capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = r.stdout + r.stderr
    widths = [(192, 192), (192, 128), (128, 64), (64, 128), (128, 192), (192, 192)]
    n_free = sum(k * n for k, n in widths[:3]) + sum(n for _, n in widths)
    n_all = sum(k * n + n for k, n in widths)
    assert "TIED WEIGHTS: %d free parameters of %d" % (n_free, n_all) in out, out[-3000:]
    assert "PROBE tied True True True 3" in out, out[-3000:]             # 140 training rows in batches of 64: three steps
    assert "TRAINING HAS ENDED." in out
    book = json.load(open(tmp_path / "out" / os.listdir(tmp_path / "out")[0] / "book.json"))
    assert len(book["ftl"]) == 1 and all(np.isfinite(book[k]).all() for k in book)
