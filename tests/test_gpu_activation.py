"""The `activation` argument on a real MI355X: every supported kind through the model classes (forward, input and parameter
gradients) against a float64 CPU copy of the same Sequential, the generic-activation kernels one by one through the
codae_*_act_* entries (every epilogue variant the env toggles select), the fused trainer step against a float64 torch loop,
and what must NOT change for ReLU (bits, 1-bit masks, the persistent chain)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
nn = torch.nn

KINDS = [nn.ReLU, nn.LeakyReLU, lambda inplace: nn.LeakyReLU(0.1, inplace), nn.ReLU6, nn.ELU, nn.CELU,
         lambda inplace: nn.CELU(0.7, inplace), nn.SELU, nn.Softplus, lambda inplace: nn.Softplus(2.0, 5.0), nn.Hardsigmoid]
KIND_IDS = ["relu", "leaky1", "leaky0.1", "relu6", "elu", "celu", "celu0.7", "selu", "softplus", "softplus2", "hardsigmoid"]


def dev():
    return torch.device("cuda:0")


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def cpu_copy(model):
    """float64 CPU Sequential with the model's weights and freshly built activation modules (not in place: autograd
    takes their derivative from the input, an independent check of the engine's derivative-from-output)."""
    mods = []
    for seq in (model.input_layer, model.output_layer):
        for m in seq:
            if isinstance(m, nn.Linear):
                lin = nn.Linear(m.in_features, m.out_features).double()
                with torch.no_grad():
                    lin.weight.copy_(m.weight.detach().cpu().double())
                    lin.bias.copy_(m.bias.detach().cpu().double())
                mods.append(lin)
            else:
                a = type(m).__new__(type(m))
                a.__dict__.update(m.__dict__)
                if hasattr(a, "inplace"):
                    a.inplace = False
                mods.append(a)
    return nn.Sequential(*mods)


def run_model(model, x_np):
    x = torch.tensor(x_np, device=dev(), requires_grad=True)
    y = model(x)
    g = torch.tensor(np.random.default_rng(5).normal(size=y.shape).astype(np.float32), device=dev())
    (y * g).sum().backward()
    torch.cuda.synchronize()
    grads = [p.grad.detach().cpu().numpy() for p in model.parameters()]
    return y.detach().cpu().numpy(), x.grad.cpu().numpy(), grads, g.cpu().numpy()


def run_ref(ref, x_np, g_np):
    x = torch.tensor(x_np, dtype=torch.float64, requires_grad=True)
    y = ref(x)
    (y * torch.tensor(g_np, dtype=torch.float64)).sum().backward()
    return y.detach().numpy(), x.grad.numpy(), [p.grad.numpy() for p in ref.parameters()]


def build(cls, E, steep, factory, seed=0):
    from codae.model import EmbeddingDenoisingAutoencoder, MixedVariableDenoisingAutoencoder
    torch.manual_seed(seed)
    io = 3 * E
    if cls == "embedding":
        return EmbeddingDenoisingAutoencoder(io, E, E, 2, 2, steep, activation=factory)
    return MixedVariableDenoisingAutoencoder([], io, E, dev(), 2, 2, steep, activation=factory)


@pytest.mark.parametrize("kind", range(len(KINDS)), ids=KIND_IDS)
@pytest.mark.parametrize("cls", ["embedding", "mixed"])
@pytest.mark.parametrize("E,steep", [(48, False), (64, False), (64, True)])
def test_model_forward_backward_fp32_matches_float64(kind, cls, E, steep):
    if cls == "embedding" and steep:
        pytest.skip("EmbeddingDenoisingAutoencoder cannot be built with steep_layer_size=True (upstream quirk)")
    model = build(cls, E, steep, KINDS[kind]).to(dev())
    model.precision = "f32"
    x = np.random.default_rng(1).random((200, 3 * E)).astype(np.float32) * 2 - 0.5
    y, dx, grads, g = run_model(model, x)
    ry, rdx, rgrads = run_ref(cpu_copy(model), x, g)
    assert np.allclose(y, ry, rtol=1e-3, atol=1e-5), np.abs(y - ry).max()
    assert rel_l2(dx, rdx) < 1e-4
    for a, b in zip(grads, rgrads):
        assert rel_l2(a, b) < 1e-4
    # encode / decode sub-chains carry the activation too
    z = model.encode(torch.tensor(x, device=dev())).detach().cpu().numpy()
    ref = cpu_copy(model)
    n_enc = len(model.input_layer)
    rz = ref[:n_enc](torch.tensor(x, dtype=torch.float64)).detach().numpy()
    assert np.allclose(z, rz, rtol=1e-3, atol=1e-5)
    d = model.decode(torch.tensor(z, device=dev())).detach().cpu().numpy()
    rd = ref[n_enc:](torch.tensor(z, dtype=torch.float64)).detach().numpy()
    assert np.allclose(d, rd, rtol=1e-3, atol=1e-5)


def bf16_restatement(model, x, g):
    """float64 forward / backward of the model rounded to bf16 where the bf16 engine rounds: input, weights, every stored
    layer output (the code layer's too: codae_forward keeps it in act[l+1] like any hidden output; only the last layer's y
    goes out in fp32), the incoming and every stored activation gradient (the GEMM result, then - for a kind other than
    ReLU - its product with the derivative taken from the stored activation).  Bias gradients: the top layer's sums the
    caller's fp32 dy (colsum_parts_f32 in codae_backward), every other layer's the STORED bf16 activation gradient (the
    data-gradient epilogues sum what they write).  Returns y, dx, [dW0, db0, dW1, ...]."""
    from codae.model.activation import as_engine_act
    bf = lambda a: torch.tensor(a).to(torch.bfloat16).double().numpy()     # noqa: E731
    layers = []
    for seq in (model.input_layer, model.output_layer):
        mods = list(seq)
        for i, m in enumerate(mods):
            if isinstance(m, nn.Linear):
                nxt = mods[i + 1] if i + 1 < len(mods) and not isinstance(mods[i + 1], nn.Linear) else None
                layers.append((bf(m.weight.detach().cpu().numpy()), m.bias.detach().cpu().double().numpy(),
                               None if nxt is None else as_engine_act(nxt)))
    hs = [bf(x)]
    for l, (W, b, act) in enumerate(layers):
        v = hs[-1] @ W.T + b
        v = v if act is None else np_act(act[0], act[1:], v)
        hs.append(v if l == len(layers) - 1 else bf(v))
    y = hs[-1]
    da = bf(g)
    grads = []
    for l in range(len(layers) - 1, -1, -1):
        W, b, _ = layers[l]
        grads[:0] = [da.T @ hs[l], (g.astype(np.float64) if l == len(layers) - 1 else da).sum(0)]
        if l == 0:
            dx = da @ W
        else:
            act = layers[l - 1][2]
            t = bf(da @ W)
            if act is not None:
                t = t * np_dact(act[0], act[1:], hs[l])
                if act[0] != 1:                    # (ReLU masks exactly; any other kind rounds the product again)
                    t = bf(t)
            da = t
    return y, dx, grads


@pytest.mark.parametrize("kind", range(len(KINDS)), ids=KIND_IDS)
@pytest.mark.parametrize("cls", ["embedding", "mixed"])
@pytest.mark.parametrize("E", [48, 64])
def test_model_forward_backward_bf16(kind, cls, E):
    model = build(cls, E, False, KINDS[kind]).to(dev())
    model.precision = "bf16"
    x = np.random.default_rng(2).random((200, 3 * E)).astype(np.float32) * 2 - 0.5
    y, dx, grads, g = run_model(model, x)
    assert model._engine.precision == 1
    ry, rdx, rgrads = bf16_restatement(model, x, g)
    assert rel_l2(y, ry) < 1e-2
    errs = [rel_l2(dx, rdx)] + [rel_l2(a, b) for a, b in zip(grads, rgrads)]
    print("MEASURE drop-in bf16 %s %s %d: y %.3g, max grad rel L2 %.3g (index %d)"
          % (KIND_IDS[kind], cls, E, rel_l2(y, ry), max(errs), int(np.argmax(errs))))
    assert max(errs) < DROPIN_BF16_REL_L2, errs


# Measured on the MI355X over every kind, both classes and E = 48 / 64: at most 9.5e-4 (ReLU 1.3e-4).  The old restatement
# left the code layer's output unrounded and summed the top bias gradient from the rounded dy, which put it 4-5.7 % off
# for ReLU; the bound is about twice the measured deviation.
DROPIN_BF16_REL_L2 = 2e-3


def _encode_decode(model, x_np, g_np):
    """decode(encode(x)) with a backward: two autograd nodes, the input gradient handed from one to the other."""
    x = torch.tensor(x_np, device=dev(), requires_grad=True)
    y = model.decode(model.encode(x))
    (y * torch.tensor(g_np, device=dev())).sum().backward()
    torch.cuda.synchronize()
    grads = [p.grad.detach().cpu().numpy() for p in model.parameters()]
    for p in model.parameters():
        p.grad = None
    return y.detach().cpu().numpy(), x.grad.cpu().numpy(), grads


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("cls", ["embedding", "mixed"])
def test_encode_then_decode_backward_equals_forward_backward(precision, cls):
    """decode(encode(x)).backward - codae_backward on the two sub-ranges, decode's with an fp32 input gradient that becomes
    encode's dy - against model(x).backward on a ragged batch (333 rows).  Both run the same GEMMs; the code layer's bias
    gradient is summed from the fp32 dy on the split path and from the stored activation gradient on the whole chain
    (in bf16: rounded), and the code layer's output leaves the encode GEMM in fp32 before decode stores it.  Every other
    tensor within 1e-6 of the whole chain's; and against float64 (f32, 1e-4) or the bf16 restatement (bf16)."""
    model = build(cls, 64, False, nn.ReLU).to(dev())
    model.precision = precision
    x = np.random.default_rng(3).random((333, 192)).astype(np.float32) * 2 - 0.5
    y, dx, grads, g = run_model(model, x)
    for p in model.parameters():
        p.grad = None
    y2, dx2, grads2 = _encode_decode(model, x, g)
    assert model._engine.precision == (1 if precision == "bf16" else 0)
    errs = [rel_l2(y2, y), rel_l2(dx2, dx)] + [rel_l2(a, b) for a, b in zip(grads2, grads)]
    code_db = 2 + 2 * (model._n_enc - 1) + 1            # (errs index of the code layer's bias gradient)
    print("MEASURE encode-decode %s %s vs whole chain: max %.3g (index %d), code-layer bias %.3g"
          % (precision, cls, max(errs), int(np.argmax(errs)), errs[code_db]))
    # everything else measured bit-identical in both precisions; the code layer's bias gradient in bf16 2.4e-3 (the
    # rounding of the stored activation gradient it sums on the whole chain)
    assert max(e for i, e in enumerate(errs) if i != code_db) <= 1e-6, errs
    assert errs[code_db] <= (1e-6 if precision == "f32" else 5e-3), errs
    if precision == "f32":
        ry, rdx, rgrads = run_ref(cpu_copy(model), x, g)
        assert rel_l2(y2, ry) < 1e-4 and rel_l2(dx2, rdx) < 1e-4
    else:
        ry, rdx, rgrads = bf16_restatement(model, x, g)
        assert rel_l2(y2, ry) < 1e-2 and rel_l2(dx2, rdx) < DROPIN_BF16_REL_L2
    for i, (a, b) in enumerate(zip(grads2, rgrads)):
        # (the restatement sums the code layer's bias gradient as the whole chain does: the bf16 split path is 2.4e-3 off)
        bound = 1e-4 if precision == "f32" else (5e-3 if i == code_db - 2 else DROPIN_BF16_REL_L2)
        assert rel_l2(a, b) < bound, i


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_backward_after_a_second_forward_is_refused(precision):
    """The engine keeps one set of saved activations: a backward through a forward whose activations a later forward
    overwrote raises HipError (_ChainFunction's stamps) instead of returning the later batch's gradients; the later
    forward's own backward still runs, and a sub-range forward (encode) invalidates a whole-chain forward too."""
    from codae.hip import HipError
    model = build("embedding", 64, False, nn.ReLU).to(dev())
    model.precision = precision
    rng = np.random.default_rng(4)
    x1, x2 = (torch.tensor(rng.random((100, 192), dtype=np.float32), device=dev()) for _ in range(2))
    y1 = model(x1)
    y2 = model(x2)
    with pytest.raises(HipError, match="overwritten"):
        y1.sum().backward()
    y2.sum().backward()
    assert all(p.grad is not None and float(p.grad.abs().sum()) > 0 for p in model.parameters())
    y3 = model(x1)
    model.encode(x2)
    with pytest.raises(HipError, match="overwritten"):
        y3.sum().backward()


def test_explicit_relu_is_bitwise_the_default_and_keeps_masks_and_chain():
    from codae.hip.engine import DaeEngine
    from codae import hip
    outs = []
    for factory in (None, nn.ReLU):
        kw = {} if factory is None else {"activation": factory}
        from codae.model import EmbeddingDenoisingAutoencoder
        torch.manual_seed(3)
        m = EmbeddingDenoisingAutoencoder(192, 64, 64, 2, 2, False, **kw).to(dev())
        m.precision = "bf16"
        x = torch.rand(256, 192, device=dev())
        y = m(x)
        y.sum().backward()
        outs.append((y.detach().cpu(), [p.grad.cpu() for p in m.parameters()]))
    assert torch.equal(outs[0][0], outs[1][0])
    assert all(torch.equal(a, b) for a, b in zip(outs[0][1], outs[1][1]))
    sched = [(384, 128, True), (128, 128, True), (128, 384, False)]
    per_layer = [(hip.ACT_RELU, 0, 0, 0), (hip.ACT_RELU, 0, 0, 0), (hip.ACT_NONE, 0, 0, 0)]
    a = DaeEngine(sched, 1024, "bf16", dev())
    b = DaeEngine(sched, 1024, "bf16", dev(), activation=per_layer)
    assert a.step_path(1024) == b.step_path(1024) == "chain"
    # same workspace (the 1-bit masks are still allocated for the ReLU layers)
    assert a.acts.numel() == b.acts.numel()


def _trainer(act, precision, use_graph=False, io=192, B=256, seed=0):
    from codae.model.schedule import linear_stack
    from codae.train import HipEmbeddingTrainer
    enc, dec = linear_stack(io, 64, 2, 2, False, False)
    rng = np.random.default_rng(seed)
    data = torch.tensor(rng.random((4 * B, io), dtype=np.float32))
    tr = HipEmbeddingTrainer(enc + dec, data, None, None, 1e-3, 1e-4, 1.0, max_batch=B, precision=precision,
                             device="cuda:0", use_graph=use_graph, activation=act)
    tr.init_params(seed=7)
    return tr, data, enc + dec


@pytest.mark.parametrize("act", [nn.ELU, nn.SELU], ids=["elu", "selu"])
def test_fused_trainer_fp32_matches_float64_torch_loop(act):
    tr, data, sched = _trainer(act, "f32")
    mods = []
    for l, (k, n, r) in enumerate(sched):
        lin = nn.Linear(k, n).double()
        with torch.no_grad():
            lin.weight.copy_(tr.engine.weight(l).cpu().double())
            lin.bias.copy_(tr.engine.bias(l).cpu().double())
        mods.append(lin)
        if r:
            mods.append(act(True))
    ref = nn.Sequential(*mods)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3, weight_decay=1e-4)
    rng = np.random.default_rng(11)
    for _ in range(5):
        idx = rng.permutation(len(data))[:256]
        tr.train_batch(torch.tensor(idx, dtype=torch.int32, device=dev()), run=None)
        xb = data[idx].double()
        opt.zero_grad()
        loss = ((ref(xb) - xb) ** 2).mean()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(ref.parameters(), 1.0)
        opt.step()
    torch.cuda.synchronize()
    assert abs(tr.engine.read_scalars()[3] - float(loss.detach())) <= 1e-3 * float(loss.detach())
    for l, lin in enumerate(m for m in ref if isinstance(m, nn.Linear)):
        w = tr.engine.weight(l).cpu().double().numpy()
        assert np.allclose(w, lin.weight.detach().numpy(), rtol=1e-3, atol=1e-5), np.abs(w - lin.weight.detach().numpy()).max()


def test_fused_trainer_bf16_deterministic_and_graph_equals_eager():
    results = []
    for use_graph in (False, False, True):
        tr, data, _ = _trainer(nn.ELU, "bf16", use_graph=use_graph)
        rng = np.random.default_rng(12)
        for _ in range(3):
            idx = rng.permutation(len(data))[:256]
            tr.train_batch(torch.tensor(idx, dtype=torch.int32, device=dev()), run=None)
        torch.cuda.synchronize()
        results.append(tr.engine.params.detach().cpu().clone())
    assert torch.equal(results[0], results[1])
    assert torch.equal(results[0], results[2])


def test_narrow_elu_stack_takes_the_per_layer_path_and_is_correct():
    from codae.hip.engine import DaeEngine
    sched = [(384, 128, True), (128, 128, True), (128, 384, False)]
    eng = DaeEngine(sched, 1024, "bf16", dev(), activation=nn.ELU)
    assert eng.step_path(1024) == "layers"
    tr, data, sched2 = _trainer(nn.ELU, "bf16", io=384, B=1024)
    assert tr.engine.step_path(1024) == "layers"
    w0 = [tr.engine.weight(l).cpu().double() for l in range(tr.engine.L)]
    b0 = [tr.engine.bias(l).cpu().double() for l in range(tr.engine.L)]
    x = data[:1024].to(dev())
    y = tr.engine.forward(x, 0, tr.engine.L)
    torch.cuda.synchronize()
    h = data[:1024].double()
    for l, (k, n, r) in enumerate(sched2):
        h = h @ w0[l].T + b0[l]
        if r:
            h = torch.nn.functional.elu(h)
    assert rel_l2(y.cpu().numpy(), h.numpy()) < 2e-2


def test_create_rejects_bad_kind_or_parameter():
    from codae import hip
    from codae.hip.engine import DaeEngine
    sched = [(64, 64, True), (64, 64, False)]
    for act in [(9, 0, 0, 0), (hip.ACT_LEAKY, -0.5, 0, 0), (hip.ACT_ELU, 1.0, 0.0, 1.0), (hip.ACT_ELU, 1.0, 1.0, -1.0),
                (hip.ACT_SOFTPLUS, 0.0, 20.0, 0.0)]:
        with pytest.raises(hip.HipError, match="codae_create") as e:
            DaeEngine(sched, 64, "f32", dev(), activation=act)
        assert "error -1" in str(e.value)               # CODAE_E_INVALID
    with pytest.raises(hip.HipError, match="last layer"):
        DaeEngine(sched, 64, "f32", dev(), activation=[(0, 0, 0, 0), (hip.ACT_ELU, 1, 1, 1)])


# ---- the kernels one by one through codae_*_act_* -----------------------------------------------------------------
def np_act(kind, p, v):
    from codae import hip
    v = v.astype(np.float64)
    if kind == hip.ACT_RELU:
        return np.maximum(v, 0)
    if kind == hip.ACT_LEAKY:
        return np.where(v > 0, v, p[0] * v)
    if kind == hip.ACT_RELU6:
        return np.clip(v, 0, 6)
    if kind == hip.ACT_ELU:
        return np.where(v > 0, p[0] * v, p[0] * p[1] * np.expm1(v * p[2]))
    if kind == hip.ACT_SOFTPLUS:
        return np.where(v * p[0] > p[1], v, np.log1p(np.exp(np.minimum(v * p[0], 80))) / p[0])
    if kind == hip.ACT_HARDSIGMOID:
        return np.clip(v / 6 + 0.5, 0, 1)
    return v


def np_dact(kind, p, y):
    from codae import hip
    y = y.astype(np.float64)
    if kind == hip.ACT_RELU:
        return (y > 0).astype(np.float64)
    if kind == hip.ACT_LEAKY:
        return np.where(y > 0, 1.0, p[0])
    if kind == hip.ACT_RELU6:
        return ((y > 0) & (y < 6)).astype(np.float64)
    if kind == hip.ACT_ELU:
        return np.where(y > 0, p[0], p[2] * (y + p[0] * p[1]))
    if kind == hip.ACT_SOFTPLUS:
        return np.where(y * p[0] > p[1], 1.0, -np.expm1(-y * p[0]))
    if kind == hip.ACT_HARDSIGMOID:
        return np.where((y > 0) & (y < 1), 1 / 6, 0.0)
    return np.ones_like(y)


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


ACT_PARAMS = None


def act_params():
    from codae import hip
    from codae.model.activation import SELU_ALPHA, SELU_SCALE
    return [(hip.ACT_RELU, 0, 0, 0), (hip.ACT_LEAKY, 0.1, 0, 0), (hip.ACT_RELU6, 0, 0, 0), (hip.ACT_ELU, 1.0, 1.0, 1.0),
            (hip.ACT_ELU, SELU_SCALE, SELU_ALPHA, 1.0), (hip.ACT_ELU, 1.0, 0.7, 1 / 0.7), (hip.ACT_SOFTPLUS, 2.0, 5.0, 0),
            (hip.ACT_HARDSIGMOID, 0, 0, 0)]


@pytest.fixture
def env_toggle():
    from codae import hip
    saved = {}

    def set_(name, value):
        saved.setdefault(name, os.environ.get(name))
        if value is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = value
        hip.lib().codae_reload_env()
    yield set_
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    hip.lib().codae_reload_env()


@pytest.mark.parametrize("f32_gemm", [None, "native"])
@pytest.mark.parametrize("M,N,K", [(37, 11, 11), (200, 136, 128), (256, 256, 256)])
def test_act_entries_fp32(M, N, K, f32_gemm, env_toggle):
    from codae import hip
    env_toggle("CODAE_F32_GEMM", f32_gemm)
    lib = hip.lib()
    rng = np.random.default_rng(M + N + K)
    x = rng.normal(size=(M, K)).astype(np.float32)
    W = (rng.normal(size=(N, K)) / np.sqrt(K)).astype(np.float32) * 2
    b = rng.normal(size=N).astype(np.float32)
    dy = rng.normal(size=(M, N)).astype(np.float32)
    Wd = (rng.normal(size=(N, K)) / np.sqrt(N)).astype(np.float32)
    for kind, p0, p1, p2 in act_params():
        xt, Wt, bt = (torch.tensor(a, device=dev()) for a in (x, W, b))
        y = torch.empty(M, N, device=dev())
        hip.check(lib.codae_linear_act_f32(P(xt), P(Wt), P(bt), P(y), M, N, K, kind, p0, p1, p2, hip.current_stream()))
        ref = np_act(kind, (p0, p1, p2), x.astype(np.float64) @ W.T.astype(np.float64) + b)
        torch.cuda.synchronize()
        assert np.allclose(y.cpu().numpy(), ref, rtol=1e-3, atol=1e-5), (kind, np.abs(y.cpu().numpy() - ref).max())
        # data gradient of the layer below: dx = (dy . W) * act'(h), h = a saved activation [M][K]
        h = np_act(kind, (p0, p1, p2), rng.normal(size=(M, K)) * 3).astype(np.float32)
        dyt, Wdt, ht = (torch.tensor(a, device=dev()) for a in (dy, Wd, h))
        dx = torch.empty(M, K, device=dev())
        hip.check(lib.codae_dgrad_act_f32(P(dyt), P(Wdt), P(ht), P(dx), M, N, K, kind, p0, p1, p2, hip.current_stream()))
        rdx = (dy.astype(np.float64) @ Wd.astype(np.float64)) * np_dact(kind, (p0, p1, p2), h)
        torch.cuda.synchronize()
        assert np.allclose(dx.cpu().numpy(), rdx, rtol=1e-3, atol=1e-5), (kind, np.abs(dx.cpu().numpy() - rdx).max())


def bf16(a):
    return torch.tensor(a).to(torch.bfloat16)


@pytest.mark.parametrize("toggle", [("CODAE_GEMM_TILE", "0"), ("CODAE_GEMM_TILE", "3"), ("CODAE_GEMM_TILE", "6"),
                                    ("CODAE_SMALL_TILE_MAX", "0"), ("CODAE_NO_DEEP_SMALL", "1"), (None, None)])
@pytest.mark.parametrize("M,N,K", [(200, 128, 192), (256, 256, 256), (1000, 384, 384)])
def test_act_entries_bf16(M, N, K, toggle, env_toggle):
    from codae import hip
    if toggle[0]:
        env_toggle(toggle[0], toggle[1])
    lib = hip.lib()
    rng = np.random.default_rng(M * 7 + N + K)
    x = bf16(rng.normal(size=(M, K)).astype(np.float32))
    W = bf16((rng.normal(size=(N, K)) / np.sqrt(K) * 2).astype(np.float32))
    b = torch.tensor(rng.normal(size=N).astype(np.float32))
    dy = bf16(rng.normal(size=(M, N)).astype(np.float32))
    for kind, p0, p1, p2 in act_params():
        for y_f32 in (0, 1):
            xt, Wt, bt = x.to(dev()), W.to(dev()), b.to(dev())
            y = torch.empty(M, N, device=dev(), dtype=torch.float32 if y_f32 else torch.bfloat16)
            hip.check(lib.codae_linear_act_bf16(P(xt), P(Wt), P(bt), P(y), y_f32, M, N, K, kind, p0, p1, p2,
                                                hip.current_stream()))
            ref = np_act(kind, (p0, p1, p2), x.double().numpy() @ W.double().numpy().T + b.double().numpy())
            torch.cuda.synchronize()
            got = y.double().cpu().numpy()
            assert np.allclose(got, ref, rtol=1e-2, atol=1e-2), (kind, y_f32, np.abs(got - ref).max())
        # data gradient through W itself (k-strided B), with the bias gradient of the layer below
        h = bf16(np_act(kind, (p0, p1, p2), rng.normal(size=(M, K)) * 3).astype(np.float32))
        dyt, Wt, ht = dy.to(dev()), W.to(dev()), h.to(dev())
        dx = torch.empty(M, K, device=dev(), dtype=torch.bfloat16)
        db = torch.empty(K, device=dev())
        ws = torch.empty(((M + 63) // 64) * K, device=dev())
        hip.check(lib.codae_dgrad_act_bf16(P(dyt), P(Wt), P(ht), P(dx), P(db), P(ws), M, N, K, kind, p0, p1, p2,
                                           hip.current_stream()))
        rdx = (dy.double().numpy() @ W.double().numpy()) * np_dact(kind, (p0, p1, p2), h.double().numpy())
        torch.cuda.synchronize()
        got = dx.double().cpu().numpy()
        assert np.allclose(got, rdx, rtol=2e-2, atol=2e-2), (kind, np.abs(got - rdx).max())
        assert np.allclose(db.cpu().numpy(), got.sum(0), rtol=1e-3, atol=1e-2)


@pytest.mark.parametrize("kind", [nn.ELU, lambda inplace: nn.LeakyReLU(0.1, inplace), nn.Softplus],
                         ids=["elu", "leaky", "softplus"])
def test_split_k_slab_reduce_epilogue(kind):
    """fp32 engine at io 384, batch 128: the forward / data-gradient GEMMs are split over K into slabs and finished by
    reduce_slabs_epi (gemm_f32_small), whose epilogue applies the activation."""
    from codae.model import EmbeddingDenoisingAutoencoder
    torch.manual_seed(4)
    m = EmbeddingDenoisingAutoencoder(384, 384, 128, 2, 2, False, activation=kind).to(dev())
    m.precision = "f32"
    x = np.random.default_rng(9).random((128, 384)).astype(np.float32)
    y, dx, grads, g = run_model(m, x)
    ry, rdx, rgrads = run_ref(cpu_copy(m), x, g)
    assert np.allclose(y, ry, rtol=1e-3, atol=1e-5)
    assert rel_l2(dx, rdx) < 1e-4
    for a, b in zip(grads, rgrads):
        assert rel_l2(a, b) < 1e-4
