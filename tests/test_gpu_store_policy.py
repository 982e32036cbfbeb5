"""Output store policy of the pipelined bf16 GEMM epilogues (CODAE_STORE_POLICY).

A cache policy cannot change a value: every check here is EQUALITY - torch.equal of whole buffers, poisoned pads included -
between the write-through policy (`wt`: sc1 stores; the sc0 sc1 flavour measured the same and is not built) and `plain`.  No
tolerance anywhere.

Kernel level, through the stand-alone C-ABI GEMMs (as tests/test_gpu_kernels.py): output 520 x 392 - three tiles each way with
ragged last ones, N % 8 == 0 - and K in {64, 128, 320}: one K-tile, two, and an odd count (where the prologue's dummy loads
matter); the tile is forced so that these small shapes take the pipelined kernels: `x` (library tile id 6, 256 x 192) for every
form, `m` (id 7, 128 x 192) for the forward form, the only one that tile is built for.
The stand-alone entries reach the forward (ReLU), the data gradient (activation mask + column sums) and the k-strided fp32
output.  The 1-bit mask out / in, the fused loss and the weight gradient's sum g^2 exist only inside an engine step: small
engines of width 64 / 128 / 320 (the same three K-tile counts) at 520 rows run one forced-tile step and every engine buffer -
saved activations with their mask bits, activation gradients (the fused-loss dy among them), weight and bias gradients, the
partial column sums, the scalars - is compared whole.

Hand-over (what a write-through store changes is WHERE the next reader finds the line): several optimizer steps of a forced-tile
3-layer 192-wide stack at B = 96 and of the smallest default-path shape (io 1536, 5 layers, B 64), policy on against off:
parameters, both moments, loss and gradient norm after every step, read once from a second torch stream behind an event and
once from the host."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
M, N = 520, 392
KS = [64, 128, 320]
POLICIES = ["wt"]
POISON = 12352.0          # (exact in bf16 and fp32; no GEMM here produces it: |values| stay far below)


@pytest.fixture(scope="module")
def hip():
    from codae import hip as H
    H.lib()
    return H


def _ints(shape, g, lo=-3, hi=4):
    return torch.randint(lo, hi, shape, generator=g).float()


class _Env:
    """CODAE_* variables for one library call sequence; the library reads them at codae_reload_env / codae_create."""

    def __init__(self, monkeypatch, hip):
        self.mp, self.hip = monkeypatch, hip
        self.names = set()

    def set(self, **kw):
        for k, v in kw.items():
            self.names.add(k)
            if v is None:
                self.mp.delenv(k, raising=False)
            else:
                self.mp.setenv(k, v)
        self.hip.check(self.hip.lib().codae_reload_env())

    def clear(self):
        for k in self.names:
            self.mp.delenv(k, raising=False)
        self.hip.check(self.hip.lib().codae_reload_env())


@pytest.fixture
def env(monkeypatch, hip):
    e = _Env(monkeypatch, hip)
    yield e
    e.clear()


def _poisoned(rows, cols, dtype, pad_rows=8):
    """[rows + pad_rows][cols] full of the poison value: the GEMM writes the first `rows` rows"""
    return torch.full((rows + pad_rows, cols), POISON, device=DEV, dtype=dtype)


def _assert_same(got, ref, rows, what):
    for name in ref:
        assert torch.equal(got[name], ref[name]), "%s: %s differs from the plain-policy run" % (what, name)
    for name, t in got.items():
        if t.dim() == 2 and t.shape[0] > rows.get(name, t.shape[0]):
            pad = t[rows[name]:]
            assert bool((pad == torch.tensor(POISON, dtype=t.dtype, device=t.device)).all()), "%s: rows past the end of %s were written" % (what, name)


def _forward(hip, K, y_f32):
    g = torch.Generator(device="cpu").manual_seed(K + 7 * y_f32)
    x, W, b = _ints((M, K), g).to(DEV).bfloat16(), _ints((N, K), g).to(DEV).bfloat16(), _ints((N,), g).to(DEV)
    y = _poisoned(M, N, torch.float32 if y_f32 else torch.bfloat16)
    hip.check(hip.lib().codae_linear_bf16(hip.ptr(x), hip.ptr(W), hip.ptr(b), hip.ptr(y), y_f32, M, N, K, 1, hip.current_stream()))
    torch.cuda.synchronize()
    return {"y": y}


def _dgrad(hip, K):
    # dx [M][N] = (dy [M][K] . W [K][N]) * [h > 0], column sums -> db; the reduction extent is K
    g = torch.Generator(device="cpu").manual_seed(11 * K)
    dy, W, h = _ints((M, K), g, -2, 3).to(DEV).bfloat16(), _ints((K, N), g, -2, 3).to(DEV).bfloat16(), _ints((M, N), g, -1, 2).to(DEV).bfloat16()
    dx = _poisoned(M, N, torch.bfloat16)
    db = torch.full((N,), POISON, device=DEV)
    ws = torch.full(((M + 63) // 64 * N,), POISON, device=DEV)
    hip.check(hip.lib().codae_dgrad_bf16(hip.ptr(dy), hip.ptr(W), hip.ptr(h), hip.ptr(dx), hip.ptr(db), hip.ptr(ws), M, K, N, hip.current_stream()))
    torch.cuda.synchronize()
    return {"dx": dx, "db": db, "colsum_part": ws}


def _wgrad(hip, K, split):
    # dW [M][N] = dy [K][M]^T x [K][N]: both operands k-strided, fp32 out; with the slab workspace the K split writes fp32 slabs
    g = torch.Generator(device="cpu").manual_seed(13 * K + split)
    dy, x = _ints((K, M), g, -2, 3).to(DEV).bfloat16(), _ints((K, N), g, -2, 3).to(DEV).bfloat16()
    dW = _poisoned(M, N, torch.float32)
    slabs = torch.full((8 * M * N,), POISON, device=DEV) if split else None
    hip.check(hip.lib().codae_wgrad_bf16(hip.ptr(dy), hip.ptr(x), hip.ptr(dW), hip.ptr(slabs) if split else None,
                                         slabs.numel() * 4 if split else 0, K, M, N, hip.current_stream()))
    torch.cuda.synchronize()
    out = {"dW": dW}
    if split:
        out["slabs"] = slabs
    return out


FORMS = {
    "forward-relu": (lambda hip, K: _forward(hip, K, 0), ("x", "m")),
    "forward-fp32-out": (lambda hip, K: _forward(hip, K, 1), ("x",)),
    "dgrad-mask-colsums": (_dgrad, ("x",)),
    "kstrided-fp32-out": (lambda hip, K: _wgrad(hip, K, False), ("x",)),
    "kstrided-fp32-slabs": (lambda hip, K: _wgrad(hip, K, True), ("x",)),
}


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("form,tile", [(f, t) for f, (_, tiles) in FORMS.items() for t in tiles])
def test_gemm_outputs_do_not_depend_on_the_store_policy(hip, env, form, tile, K):
    run = FORMS[form][0]
    env.set(CODAE_GEMM_TILE=tile, CODAE_STORE_POLICY="plain")
    ref = run(hip, K)
    rows = {"y": M, "dx": M, "dW": M}
    # (the slab workspace stays untouched where the library does not split K: one or two K-tiles)
    assert all(bool((t[:rows[n]] != POISON).any()) for n, t in ref.items() if n in rows), "the plain run wrote nothing"
    for pol in POLICIES:
        env.set(CODAE_STORE_POLICY=pol)
        _assert_same(run(hip, K), ref, rows, "%s, tile %s, K %d, policy %s" % (form, tile, K, pol))


def _problem(S, E, B, n_layers, seed):
    """n_layers square Linear layers of width S * E (ReLU after all but the last), dataset, slot masks, 4 index batches"""
    from oracle import dae_oracle as O
    io = S * E
    rng = np.random.default_rng(seed)
    n = B + 64
    data = rng.random((n, io), dtype=np.float32)
    sched = [(io, io, l + 1 < n_layers) for l in range(n_layers)]
    params = O.init_params(sched, rng)
    bm, _, _ = O.corrupter_tables([{"size": E, "position": s * E} for s in range(S)], 1)
    mtu = rng.integers(0, S, (n, 1)).astype(np.int32)
    idx = [torch.tensor(rng.permutation(n)[:B], dtype=torch.int32, device=DEV) for _ in range(4)]
    return sched, params, torch.tensor(data), torch.tensor(bm).to(torch.uint8), torch.tensor(mtu), idx


def _trainer(problem, B, clip=1.0):
    from codae.train import HipEmbeddingTrainer
    sched, params, data, bm, mtu, _ = problem
    tr = HipEmbeddingTrainer(sched, data, bm, mtu, 1e-3, 1e-4, clip, max_batch=B, precision="bf16", device=DEV)
    tr.load_params(params)
    return tr


# every launch of the step on the forced pipelined tile, on one stream: per-layer unsplit weight gradients (their epilogue adds
# sum g^2), 1-bit masks, fused loss
FORCED = dict(CODAE_GEMM_TILE="x", CODAE_NO_CHAIN="1", CODAE_NO_DEFER_WGRAD="1", CODAE_SINGLE_STREAM="1", CODAE_WGRAD_SPLITK="1")


@pytest.mark.parametrize("S,E", [(2, 32), (2, 64), (5, 64)], ids=["K64", "K128", "K320"])
def test_engine_only_epilogue_forms_do_not_depend_on_the_store_policy(hip, env, S, E):
    """mask bits out / in, fused loss, sum g^2 from the fp32 epilogue: one forced-tile step at 520 rows, every engine buffer"""
    B = M
    problem = _problem(S, E, B, 3, 100 + E * S)
    outs = {}
    for pol in ["plain"] + POLICIES:
        env.set(CODAE_STORE_POLICY=pol, **FORCED)
        tr = _trainer(problem, B)
        assert tr.engine.step_path(B) == "layers"
        tr.train_batch(problem[5][0], run=0)
        eng = tr.engine
        gsq = eng.read_scalars()[2]
        outs[pol] = {"acts": eng.acts.clone(), "dacts": eng.dacts.clone(), "grads": eng.grads.clone(), "bias_parts": eng.bias_parts.clone(),
                     "scalars": eng.scalars.clone(), "params": eng.params.clone(), "shadow": eng.shadow.clone(), "shadow_t": eng.shadow_t.clone()}
        del tr
    assert float(outs["plain"]["grads"].abs().max()) > 0 and gsq > 0
    for pol in POLICIES:
        for name, ref in outs["plain"].items():
            assert torch.equal(outs[pol][name], ref), "policy %s: %s differs from the plain-policy step" % (pol, name)


def _run_steps(problem, B, steps, side):
    """[(params, m, v, scalars)] after every step: read by a second stream behind an event (`side`) or straight from the host"""
    tr = _trainer(problem, B)
    eng = tr.engine
    out = []
    for s in range(steps):
        tr.train_batch(problem[5][s], run=0)
        if side is not None:
            eng.join()
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                side.wait_event(ev)
                snap = (eng._params.clone(), eng.adam_m.clone(), eng.adam_v.clone(), eng.scalars.clone())
            torch.cuda.current_stream().wait_stream(side)
            loss_norm = None
        else:
            loss_norm = tr.last_loss_and_grad_norm()
            snap = (eng.params.cpu(), eng.adam_m.cpu(), eng.adam_v.cpu(), eng.scalars.cpu())
        out.append((snap, loss_norm))
    torch.cuda.synchronize()
    del tr
    return out


@pytest.mark.parametrize("reader", ["second-stream", "host"])
@pytest.mark.parametrize("stack", ["forced-3x192-B96", "default-io1536-L5-B64"])
def test_steps_hand_over_the_same_bits_under_every_store_policy(hip, env, stack, reader):
    if stack == "forced-3x192-B96":
        S, E, B, n_layers, forced = 3, 64, 96, 3, FORCED          # 3 layers, 192 wide
    else:
        S, E, B, n_layers, forced = 3, 512, 64, 5, {}             # the engine's own kernel choice
    problem = _problem(S, E, B, n_layers, 7)
    side = torch.cuda.Stream(device=DEV) if reader == "second-stream" else None
    env.set(CODAE_STORE_POLICY="plain", **forced)
    ref = _run_steps(problem, B, 4, side)
    assert not torch.equal(ref[0][0][0], ref[3][0][0]), "the parameters never moved"
    for pol in POLICIES + [None]:                  # None: the engine's own choice by output size
        env.set(CODAE_STORE_POLICY=pol, **forced)
        got = _run_steps(problem, B, 4, side)
        for s, ((snap, ln), (rsnap, rln)) in enumerate(zip(got, ref)):
            for name, a, b in zip(("parameters", "adam m", "adam v", "scalars"), snap, rsnap):
                assert torch.equal(a, b), "policy %s, step %d: %s differ from the plain-policy run" % (pol, s, name)
            assert ln == rln, "policy %s, step %d: loss / gradient norm %r against %r" % (pol, s, ln, rln)
