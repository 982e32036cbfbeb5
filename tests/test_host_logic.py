"""CPU-only tests of the host side: the C-ABI library loads and exports every symbol the header
declares (no compute call is made), and the Python mirror of the reference interface
(codae.model / codae.tool / codae.dataset) agrees with the golden fixtures and the oracle."""
import json
import os
import random
import re

import numpy as np
import pytest
import torch

from golden_util import Golden, close
from oracle import dae_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from codae import hip
    header = open(os.path.join(ROOT, "include", "codae_hip.h")).read()
    declared = set(re.findall(r"\b(codae_[a-z0-9_]+)\s*\(", header))
    declared -= {"codae_engine"}
    lib = hip.lib()
    missing = [n for n in sorted(declared) if not hasattr(lib, n)]
    assert not missing, missing
    assert declared == set(hip.PROTOTYPES), declared ^ set(hip.PROTOTYPES)
    assert lib.codae_abi_version() == hip.ABI_VERSION == int(re.search(r"#define CODAE_ABI_VERSION (\d+)", header).group(1))


def _header_enum(header, prefix):
    """{name: value} of the `PREFIX_NAME = value` enumerators of include/codae_hip.h."""
    return {k: int(v) for k, v in re.findall(r"\b(%s[A-Z0-9_]+)\s*=\s*(-?\d+)" % prefix, header)}


def test_binding_constants_match_the_header():
    """the Python side once hard-coded S_COUNT = 72 against the header's 80 (Adam step slot past the
    tensor): every CODAE_S_* / CODAE_K_* / CODAE_PREC_* the binding names must equal the header's value."""
    from codae import hip
    header = open(os.path.join(ROOT, "include", "codae_hip.h")).read()
    S = _header_enum(header, "CODAE_S_")
    for name in ("SQ_FULL", "SQ_PARTIAL", "GRAD_SQ", "LAST_LOSS", "STEP_SQ", "CLIP_COEF", "GRAD_SQ_SLOTS", "N_SLOTS",
                 "ADAM_STEP", "COUNT"):
        assert getattr(hip, "S_" + name) == S["CODAE_S_" + name], name
    assert hip.S_ADAM_STEP < hip.S_COUNT and hip.S_GRAD_SQ_SLOTS + hip.S_N_SLOTS <= hip.S_ADAM_STEP
    K = _header_enum(header, "CODAE_K_")
    assert K["CODAE_K_COUNT"] == len(hip.KERNEL_CLASSES)
    for i, name in enumerate(hip.KERNEL_CLASSES):
        assert K["CODAE_K_" + name.upper()] == i, name
    P = _header_enum(header, "CODAE_PREC_")
    assert (hip.PREC_F32, hip.PREC_BF16) == (P["CODAE_PREC_F32"], P["CODAE_PREC_BF16"])


def test_struct_sizes_are_checked_at_load(monkeypatch):
    """codae_struct_sizes(): the ctypes layouts must equal the library's sizeof()s, and a binding with a short
    struct (INTEGRATION.md once showed a 9-field codae_buffers) must be refused before any call."""
    import ctypes as C
    from codae import hip
    lib = hip.lib()
    got = (C.c_int32 * 7)()
    assert lib.codae_struct_sizes(got, 7) == 0
    assert list(got) == hip.struct_sizes_expected()
    assert lib.codae_struct_sizes(got, 3) != 0          # too little room: an error, not an overrun

    class ShortBuffers(C.Structure):
        _fields_ = hip.Buffers._fields_[:9]
    monkeypatch.setattr(hip, "Buffers", ShortBuffers)
    with pytest.raises(hip.HipError, match="codae_buffers"):
        hip.check_struct_sizes(lib)


def test_integration_doc_shows_the_current_binding():
    """INTEGRATION.md's ctypes snippet is generated from the binding's own field lists."""
    from codae import hip
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for cls in (hip.Buffers, hip.Batch, hip.Hyper):
        for name, _ in cls._fields_:
            assert '"%s"' % name in doc, (cls.__name__, name)
    header = open(os.path.join(ROOT, "include", "codae_hip.h")).read()
    for fn in set(re.findall(r"\b(codae_[a-z0-9_]+)\s*\(", header)) - {"codae_engine"}:
        assert fn in doc, fn


def test_missing_library_fails_loudly(monkeypatch):
    from codae import hip
    monkeypatch.setattr(hip, "_lib", None)
    monkeypatch.setattr(hip, "LIB_PATH", "/nonexistent/libcodae_hip.so")
    with pytest.raises(hip.HipError, match="no CPU fallback"):
        hip.lib()


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "mui-deepautoencoder_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(d, f)).read()
                assert "oracle" not in src.replace("the oracle", "").replace("oracle-", "") or f == "never", (d, f)


@pytest.mark.parametrize("name", ["embedding_square", "embedding_taper"])
def test_embedding_model_surface_and_seeded_init(name):
    from codae.model import EmbeddingDenoisingAutoencoder
    g = Golden(name)
    m = g.meta
    torch.manual_seed(m["seed"])
    model = EmbeddingDenoisingAutoencoder(m["S"] * m["E"], m["z"], m["E"], m["nb_input_layer"], m["nb_output_layer"], False)
    sd = model.state_dict()
    assert list(sd.keys()) == g.names
    for n, t in sd.items():          # same torch seed -> the reference's exact Xavier draws
        assert np.array_equal(t.numpy(), g["init__" + n.replace(".", "__")]), n
    assert [n for n, _ in model.named_parameters()] == g.names
    assert model.nb_category == m["S"] and isinstance(model.nb_category, float)
    assert (model.io_size, model.z_size, model.embedding_size, model.mode) == (m["S"] * m["E"], m["z"], m["E"], 0)
    assert "Linear(in_features=48, out_features=48, bias=True)" in repr(model) and "ReLU(inplace=True)" in repr(model)
    from codae.hip import HipError
    with pytest.raises(HipError, match="HIP device"):
        model(torch.zeros(2, m["S"] * m["E"]))
    with pytest.raises(HipError):
        model.corrupt(torch.zeros(2, 4), torch.ones(2, 4))


def test_model_constructor_errors_and_mixed_surface():
    from codae.model import EmbeddingDenoisingAutoencoder, MixedVariableDenoisingAutoencoder
    with pytest.raises(Exception, match="multiple of embedding_size"):
        EmbeddingDenoisingAutoencoder(50, 10, 16)
    with pytest.raises(UnboundLocalError):
        EmbeddingDenoisingAutoencoder(48, 48, 16, 2, 2, True)      # upstream quirk (embedding_...py:126)
    g = Golden("abalone_k2")
    torch.manual_seed(g.meta["seed"])
    mm = MixedVariableDenoisingAutoencoder(g.meta["arch"], 11, 11, torch.device("cpu"), 2, 2, True)
    for n, t in mm.state_dict().items():
        assert np.array_equal(t.numpy(), g["init__" + n.replace(".", "__")]), n
    assert mm.arch == g.meta["arch"] and mm.device == torch.device("cpu")
    with pytest.raises(Exception, match="invalid corruption type"):
        mm.corrupt(torch.zeros(1, 11), torch.ones(1, 11), corruption_type="gaussian")
    from codae.model.schedule import linear_stack
    for args in [(1536, 1536, 4, 4, False), (1536, 128, 2, 2, False), (48, 16, 4, 4, False), (11, 11, 2, 2, True), (11, 4, 3, 2, False)]:
        for mixed in (False, True):
            try:
                ref = O.layer_schedule(*args, "mixed" if mixed else "embedding")
            except UnboundLocalError:
                with pytest.raises(UnboundLocalError):
                    linear_stack(*args, mixed)
                continue
            enc, dec = linear_stack(*args, mixed)
            assert enc + dec == ref


@pytest.mark.parametrize("name", ["embedding_square", "abalone_k2"])
def test_corrupter_matches_reference_tables(name):
    from codae.tool import Corrupter
    g = Golden(name)
    m = g.meta
    arch = ([{"size": m["E"], "position": s * m["E"]} for s in range(m["S"])] if m["kind"] == "embedding" else m["arch"])
    random.seed(m["seed"])
    if m["kind"] == "embedding":         # the script draws N samples first (embedding.py:131-132)
        c = list(range(m["S"]))
        for _ in range(m["N"]):
            random.sample(c, len(c))
    cor = Corrupter(nb_observation=m["N"], arch=arch, k_max=m["k_max"], device=torch.device("cpu"))
    assert np.array_equal(cor.binary_masks.numpy(), g["binary_masks"])
    assert np.array_equal(cor.mask_to_use.numpy(), g["mask_to_use"])
    assert cor.nb_missing_per_run == list(g["nb_missing_per_run"])
    assert cor.nb_run == g["binary_masks"].shape[0] and cor.io_size == g["binary_masks"].shape[1]
    idx, run = g.calls()[0]
    masks, fmask = cor.get_masks(tuple(int(i) for i in idx), run)
    rm, rf = O.get_masks(g["binary_masks"], g["nb_missing_per_run"], g["mask_to_use"], m["k_max"], idx, run)
    assert len(masks) == m["k_max"]
    for a, b in zip(masks, rm):
        assert np.array_equal(a.numpy(), b)
    assert np.array_equal(fmask.numpy(), rf)
    with pytest.raises(Exception, match="Invalid k_max"):
        Corrupter(10, arch, len(arch), torch.device("cpu"))


def test_concatenated_embedding_dataset_and_loader(tmp_path):
    from codae.dataset import ConcatenatedEmbeddingDataset
    from codae.tool import collate_embedding, load_dataset_of_embeddings
    g = Golden("embedding_square")
    m = g.meta
    per_cat = g["data_per_category"]
    emb = {"o%03d" % i: {c: per_cat[s][i].tolist() for s, c in enumerate(m["categories"])} for i in range(m["N"])}
    emb["lacking"] = {m["categories"][1]: [0.0] * m["E"]}
    ds = ConcatenatedEmbeddingDataset(emb, m["categories"])
    assert ds.nb_observation == m["N"] == len(ds) and ds.nb_predictor == m["S"] * m["E"] and ds.nb_used_category == m["S"]
    assert np.allclose(ds.data.numpy(), g["data"], rtol=1e-6, atol=0) and abs(ds.scale - m["scale"]) < 1e-6 * m["scale"]
    assert np.array_equal(ds.data_per_category[2].numpy(), per_cat[2])
    assert [a["position"] for a in ds.arch] == [0, m["E"], 2 * m["E"]] and ds.arch[0]["type"] == "regression"
    row, idx = ds[5]
    assert idx == 5 and torch.equal(row, ds.data[5])
    batch, ids = collate_embedding([ds[1], ds[3]])
    assert batch.shape == (2, m["S"] * m["E"]) and ids == (1, 3)
    path = tmp_path / "emb.json"
    path.write_text(json.dumps(emb))
    cfg = {"DATASET": {"USED_CATEGORY": m["categories"]}}
    a = load_dataset_of_embeddings(str(path), cfg, cache_dir=str(tmp_path / "tmp") + "/")
    b = load_dataset_of_embeddings(str(path), cfg, cache_dir=str(tmp_path / "tmp") + "/")   # from the .npz cache
    assert torch.equal(a.data, ds.data) and torch.equal(b.data, ds.data) and b.index == ds.index


def test_mixed_variable_dataset_matches_oracle():
    import pandas as pd
    from codae.dataset import MixedVariableDataset
    rng = np.random.default_rng(2)
    df = pd.DataFrame({"sex": rng.choice(list("MFI"), 40), "a": rng.random(40), "rings": rng.integers(1, 20, 40)})
    ds = MixedVariableDataset(df)
    ref = O.mixed_variable_dataset([df[c].tolist() for c in df.columns], list(df.columns), [False, True, True])
    assert np.array_equal(ds.data.numpy(), ref["data"]) and np.array_equal(ds.type_mask.numpy(), ref["type_mask"])
    assert [(a["size"], a["type"], a["position"]) for a in ds.arch] == [(a["size"], a["type"], a["position"]) for a in ref["arch"]]
    assert ds.nb_predictor == 3 and ds.io_size == 5 and ds.nb_observation == 40


def test_criteria_match_oracle():
    from codae.tool import CombinedCriterion, Normalizer, RankingLoss, get_mask_transformation, get_rmse
    g = Golden("abalone_k2")
    m = g.meta
    arch = m["arch"]
    rng = np.random.default_rng(5)
    idx, run = g.calls()[7]
    B = len(idx)
    x = g["data"][idx]
    y = rng.standard_normal((B, 11)).astype(np.float32)
    T = get_mask_transformation(g["type_mask"], [0] * len(arch))
    assert np.array_equal(T.numpy(), O.mask_transformation(g["type_mask"], len(arch)))
    yt = torch.tensor(y, requires_grad=True)
    crit = CombinedCriterion(arch, 2, torch.device("cpu"), torch.tensor(g["type_mask"]), weight=m["weight"], reduction="mean")
    loss = crit(x=torch.tensor(x), y=yt)
    loss.backward()
    assert close(float(loss), O.combined_mean(arch, m["weight"], x, y))
    assert close(yt.grad.numpy(), O.combined_mean_grad_y(arch, m["weight"], x, y), atol=1e-7)
    mon = CombinedCriterion(arch, 2, torch.device("cpu"), torch.tensor(g["type_mask"]), reduction="none")
    full = mon(torch.tensor(x), torch.tensor(y), as_numpy=True)
    assert close(full, O.combined_full(arch, x, y))
    masks, fmask = O.get_masks(g["binary_masks"], g["nb_missing_per_run"], g["mask_to_use"], 2, idx, run)
    tm = [torch.tensor(a) for a in masks]
    assert close(mon.get_per_k(full, tm), O.get_per_k(full, masks, O.mask_transformation(g["type_mask"], len(arch))))
    assert close(mon.get_partial(full, torch.tensor(fmask)), O.get_partial(full, fmask, O.mask_transformation(g["type_mask"], len(arch))))

    class Scaler:
        data_min_, data_max_, data_range_ = g["norm_min"], g["norm_min"] + g["norm_scale"], g["norm_scale"]
    nz = Normalizer(Scaler(), torch.device("cpu"))
    assert close(nz.undo(torch.tensor(x[:, 3:])).numpy(), O.normalizer_undo(x[:, 3:], g["norm_scale"], g["norm_min"]))
    assert close(nz.do(nz.undo(torch.tensor(x[:, 3:]))).numpy(), x[:, 3:], atol=1e-6)
    assert abs(get_rmse(np.ones(4), np.zeros(4)) - 1) < 1e-12

    ge = Golden("embedding_square")

    class DS:
        nb_predictor, nb_used_category, embedding_size = 48, 3, 16
        data_per_category = {c: torch.tensor(ge["data_per_category"][c]) for c in range(3)}
    val = list(ge["validation_indices"])
    rl = RankingLoss(DS(), val, device=torch.device("cpu"))
    idx, run = ge.calls()[6]
    _, fm = O.get_masks(ge["binary_masks"], ge["nb_missing_per_run"], ge["mask_to_use"], 1, idx, run)
    pred = rng.standard_normal((len(idx), 48)).astype(np.float32)
    got = rl.get(torch.tensor(pred), torch.tensor(fm), tuple(int(i) for i in idx))
    assert abs(got - O.ranking_loss(pred, fm, idx, list(ge["data_per_category"]), 16, val)) < 1e-9


def test_epoch_sampler_matches_torch_dataloader_order():
    """SubsetEpochSampler must visit the batches DataLoader(SubsetRandomSampler) would
    (script/train_dae_on_embedding.py:118-128 of the reference), seed for seed."""
    from torch.utils.data import DataLoader
    from torch.utils.data.sampler import SubsetRandomSampler
    from codae.tool import collate_embedding
    from codae.train import SubsetEpochSampler

    class DS(torch.utils.data.Dataset):
        def __len__(self): return 100
        def __getitem__(self, i): return torch.tensor([float(i)]), i
    subset = [int(v) for v in np.random.default_rng(0).permutation(100)[:70]]
    torch.manual_seed(11)
    loader = DataLoader(DS(), batch_size=16, collate_fn=collate_embedding, sampler=SubsetRandomSampler(subset))
    ref = [list(ids) for _ in range(2) for _, ids in loader]
    torch.manual_seed(11)
    mine = SubsetEpochSampler(subset, 16)
    got = [b.tolist() for _ in range(2) for b in mine]
    assert got == ref and len(mine) == 5
    # the one-copy-per-epoch form the scripts iterate (views of the whole epoch order): same draws, same batches
    torch.manual_seed(11)
    moved = [b.tolist() for _ in range(2) for b in mine.device_batches("cpu")]
    assert moved == ref
    assert next(iter(mine.device_batches("cpu"))).dtype == torch.int32
    assert next(iter(mine.device_batches("cpu", dtype=torch.long))).dtype == torch.long


def test_host_threads_follow_the_cpu_quota_and_are_never_raised(tmp_path, monkeypatch):
    """fit_host_threads caps torch's intra-op pool at min(affinity, cgroup quota) and never widens it (why it exists: a
    256-thread pool under a 16-cpu CFS quota gets the whole container throttled, GPU enqueue thread included)."""
    import builtins
    from codae import train as T
    share = T.host_cpu_share()
    assert 1 <= share <= len(os.sched_getaffinity(0))
    before = torch.get_num_threads()
    try:
        assert T.fit_host_threads() == share and torch.get_num_threads() == min(before, share)
        torch.set_num_threads(1)
        T.fit_host_threads()
        assert torch.get_num_threads() == 1
        # a cgroup-v2 quota of 2.5 cpus counts as 2; "max" leaves the affinity mask
        real_open = builtins.open
        for text, want in (("250000 100000\n", min(2, len(os.sched_getaffinity(0)))), ("max 100000\n", len(os.sched_getaffinity(0)))):
            f = tmp_path / "cpu.max"
            f.write_text(text)
            monkeypatch.setattr(builtins, "open", lambda p, *a, **k: real_open(str(f) if p == "/sys/fs/cgroup/cpu.max" else p, *a, **k))
            assert T.host_cpu_share() == want
            monkeypatch.setattr(builtins, "open", real_open)
    finally:
        torch.set_num_threads(before)


def _load_check_isa():
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_isa", os.path.join(ROOT, "tools", "check_isa.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_isa_guard_passes_on_the_built_library():
    """tools/check_isa.py (run by build()): every bf16 GEMM kernel of the code object that ships keeps its asm-issued
    transposed LDS reads behind an s_waitcnt, has no vmcnt(0) in a pipelined K loop and no scratch."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_isa.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failing" in r.stdout and "k-strided pipelined instantiations" in r.stdout
    assert "packed-fp32 ops scanned" in r.stdout                      # rule 4 ran over every function of the code object


def test_isa_guard_detects_the_hazards_it_exists_for():
    """The checker itself, on hand-written instruction streams: (a) an MFMA that consumes a transposed read before the
    covering lgkmcnt wait, (b) a VALU write to a register whose transposed read is still in flight (what round 1's
    code object did with the dead last-tile reads), (c) vmcnt(0) inside a pipelined K loop; and a clean loop passes."""
    C = _load_check_isa()
    name = "gemm_bf16_pipe_kernel<256, 192, 4, 2, 6, 1, 1, 1, 0, 0>"

    def kernel(body):
        ins = [(0x100, "s_nop", "0")]
        a = 0x104
        for op, args in body:
            ins.append((a, op, args)); a += 4
        ins.append((a, "s_cbranch_scc1", "65000 <k+0x4>"))
        return ins

    clean = [("ds_read_b64_tr_b16", "v[10:11], v5"), ("ds_read_b64_tr_b16", "v[12:13], v5 offset:768"),
             ("s_waitcnt", "vmcnt(6)"), ("s_waitcnt", "lgkmcnt(0)"), ("s_barrier", ""),
             ("v_mfma_f32_16x16x32_bf16", "v[0:3], v[10:13], v[20:23], v[0:3]")]
    assert C.check_kernel("k", name, kernel(clean)) == []
    early = [clean[0], clean[1], clean[5], clean[3]]
    assert any("touches" in e for e in C.check_kernel("k", name, kernel(early)))
    one_left = [clean[0], clean[1], ("s_waitcnt", "lgkmcnt(1)"), clean[5]]       # the younger read is still in flight
    assert any("touches" in e for e in C.check_kernel("k", name, kernel(one_left)))
    waw = [clean[0], ("v_add_u32_e32", "v10, 32, v7"), clean[3], clean[5]]
    assert any("v_add_u32_e32" in e for e in C.check_kernel("k", name, kernel(waw)))
    drained = clean[:2] + [("s_waitcnt", "vmcnt(0)")] + clean[3:]
    assert any("vmcnt(0)" in e for e in C.check_kernel("k", name, kernel(drained)))


def test_isa_guard_flags_packed_fp32_ops_that_route_a_hi_half_into_the_lo_result():
    """Rule 4: on this MI355X pool v_pk_{fma,add,mul}_f32 with op_sel set on src1 / src2 returns the lo
    result of lanes 48-63 with the re-routed half read as zero while MFMAs are in flight (tools/abl/pk_fma_opsel_repro.hip).
    The exact instruction the compiler formed in the failing build must be flagged; the forms measured exact must not."""
    C = _load_check_isa()
    bad = [(0x10, "v_pk_fma_f32", "v[18:19], v[18:19], v[18:19], v[62:63] op_sel:[0,0,1] op_sel_hi:[1,1,0]"),        # round 2's build
           (0x18, "v_pk_fma_f32", "v[4:5], v[8:9], v[10:11], v[8:9] op_sel:[0,1,0] op_sel_hi:[1,0,1]"),
           (0x20, "v_pk_add_f32", "v[2:3], v[38:39], v[38:39] op_sel:[0,1] op_sel_hi:[1,0]"),
           (0x28, "v_pk_mul_f32", "v[2:3], v[6:7], v[8:9] op_sel:[0,1] op_sel_hi:[1,0]"),
           (0x30, "v_pk_fma_f32", "v[2:3], v[6:7], v[6:7], v[8:9] op_sel:[0,0,1] op_sel_hi:[1,1,1] neg_lo:[0,0,1]")]
    errs = C.packed_opsel_errors(bad)
    assert len(errs) == len(bad), errs
    assert "src2" in errs[0] and "src1" in errs[1] and "src1" in errs[2]
    fine = [(0x10, "v_pk_fma_f32", "v[18:19], v[32:33], v[32:33], v[18:19]"),
            (0x18, "v_pk_add_f32", "v[18:19], v[64:65], v[18:19] op_sel:[1,0] op_sel_hi:[0,1]"),                     # src0 swapped: exact
            (0x20, "v_pk_mul_f32", "v[34:35], s[22:23], v[30:31] op_sel_hi:[0,1]"),                                  # broadcast of a lo half
            (0x28, "v_pk_fma_f32", "v[50:51], s[22:23], v[30:31], 0 op_sel_hi:[0,1,0]"),
            (0x30, "v_pk_add_f32", "v[18:19], v[30:31], v[18:19] neg_lo:[0,1] neg_hi:[0,1]"),
            (0x38, "v_pk_mul_f32", "v[30:31], v[18:19], -2.0 op_sel_hi:[1,0]"),
            (0x40, "v_pk_fma_f32", "v[2:3], v[6:7], v[6:7], v[8:9] op_sel_hi:[1,1,0]"),                               # both results take src2.lo: exact
            (0x48, "v_fma_f32", "v2, v6, v6, v8")]
    assert C.packed_opsel_errors(fine) == []


def test_shard_batch_skips_batches_smaller_than_the_world():
    """a ragged last batch with fewer rows than ranks used to leave the high ranks with an empty shard (their
    launch fails, the others hang in the all-reduce).  shard_batch gives every rank the same verdict."""
    from codae.train import shard_batch, seed_all_ranks
    b = torch.arange(10)
    assert torch.equal(shard_batch(b, 0, 1), b)
    parts = [shard_batch(b, r, 4) for r in range(4)]
    assert sorted(torch.cat(parts).tolist()) == list(range(10)) and all(len(p) >= 2 for p in parts)
    assert all(shard_batch(torch.arange(3), r, 4) is None for r in range(4))
    assert all(shard_batch(torch.arange(1), r, 2) is None for r in range(2))
    assert [len(shard_batch(torch.arange(4), r, 4)) for r in range(4)] == [1, 1, 1, 1]
    # same seed on every rank -> same mask tables and sampler order
    from codae.tool import Corrupter
    arch = [{"size": 4, "position": 4 * s} for s in range(3)]
    tabs = []
    for _ in range(2):
        seed_all_ranks(1234)
        c = Corrupter(nb_observation=20, arch=arch, k_max=1, device=torch.device("cpu"))
        tabs.append((c.mask_to_use.clone(), torch.randperm(7)))
    assert torch.equal(tabs[0][0], tabs[1][0]) and torch.equal(tabs[0][1], tabs[1][1])


def test_three_bf16_planes_carry_an_fp32_value_and_six_products_carry_its_product():
    """The arithmetic of gemm_f32x3.hip restated in numpy (no GPU): a0 = bf16(a), a1 = bf16(a - a0), a2 = bf16(a - a0 - a1) with
    round-to-nearest-even; the differences are exact in fp32; the planes leave out less than 2^-24 |a|; of the nine plane
    products the six the kernel keeps reproduce a * b to 1.5 * 2^-23 relative, each of them exactly representable in fp32
    (8 x 8 significant bits).  Integers below 2^24 split exactly."""
    def bf16(x):                     # round-to-nearest-even to 8 significant bits, kept as float32
        u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
        u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
        return u.astype(np.uint32).view(np.float32)

    def planes(x):
        x = np.asarray(x, dtype=np.float32)
        p0 = bf16(x)
        r1 = (x - p0).astype(np.float32)
        assert np.array_equal(r1.astype(np.float64), x.astype(np.float64) - p0.astype(np.float64))        # exact in fp32
        p1 = bf16(r1)
        r2 = (r1 - p1).astype(np.float32)
        assert np.array_equal(r2.astype(np.float64), r1.astype(np.float64) - p1.astype(np.float64))
        return p0, p1, bf16(r2)
    rng = np.random.default_rng(0)
    a = (rng.standard_normal(200000) * np.exp(rng.uniform(-20, 20, 200000))).astype(np.float32)
    b = (rng.standard_normal(200000) * np.exp(rng.uniform(-20, 20, 200000))).astype(np.float32)
    pa, pb = planes(a), planes(b)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    assert np.all(np.abs(a64 - sum(p.astype(np.float64) for p in pa)) <= 2.0 ** -24 * np.abs(a64))
    assert np.all(np.abs(pa[1]) <= 2.0 ** -8 * np.abs(a) * 1.01) and np.all(np.abs(pa[2]) <= 2.0 ** -16 * np.abs(a) * 1.01)
    kept = [(0, 2), (1, 1), (2, 0), (0, 1), (1, 0), (0, 0)]                    # (plane of a, plane of b): i + j <= 2
    total = np.zeros_like(a64)
    for i, j in kept:
        prod64 = pa[i].astype(np.float64) * pb[j].astype(np.float64)
        assert np.array_equal((pa[i] * pb[j]).astype(np.float64), prod64)       # each kept product is exact in fp32
        total += prod64
    assert np.all(np.abs(total - a64 * b64) <= 1.5 * 2.0 ** -23 * np.abs(a64 * b64))
    ints = rng.integers(-(2 ** 24) + 1, 2 ** 24, 100000).astype(np.float32)
    assert np.array_equal(sum(p.astype(np.float64) for p in planes(ints)), ints.astype(np.float64))


def test_bench_dump_outputs_and_rollback_on_host_tensors(tmp_path):
    """bench.py's --dump-outputs writer and the roll-back of the extra warm-up steps, on a stand-in for the engine that keeps
    the same state tensors on the host: the C3 shapes stay under 64 MB, the weight sample is the same every time, and a
    restore puts every carried-over tensor and the step count back."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    io, L = 1536, 10

    class Eng:
        def __init__(self, seed):
            g = torch.Generator().manual_seed(seed)
            n = L * (io * io + io)
            self.L, self.step_count = L, 0
            self.params, self.grads = torch.rand(n, generator=g), torch.rand(n, generator=g)
            self.adam_m, self.adam_v = torch.rand(n, generator=g), torch.rand(n, generator=g)
            self.shadow = self.params[:L * io * io].to(torch.bfloat16)
            self.shadow_t = self.shadow.clone()
            self.scalars = torch.rand(80, generator=g, dtype=torch.float64)

        def weight(self, l): return self.params[l * io * io:(l + 1) * io * io].view(io, io)
        def bias(self, l): return self.params[L * io * io + l * io:L * io * io + (l + 1) * io]
        def read_scalars(self): return float(self.scalars[0]), float(self.scalars[1]), float(self.scalars[2]), float(self.scalars[3])

    class Tr:
        def __init__(self, seed): self.engine = Eng(seed)
        def last_loss_and_grad_norm(self): return float(self.engine.scalars[3]), float(self.engine.scalars[2]) ** 0.5

    tr = Tr(0)
    names = bench.dump_outputs(tr, str(tmp_path / "a"))
    bench.dump_outputs(Tr(0), str(tmp_path / "b"))
    assert names == sorted(["loss", "grad_norm", "metric_sums", "weights_sample", "biases"])
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy"))
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n
        total += a.nbytes
    assert total <= 64 << 20
    w = np.load(tmp_path / "a" / "weights_sample.npy")
    assert w.shape == (L, bench.DUMP_WEIGHT_FLOATS // L)
    assert np.isin(w[3], tr.engine.weight(3).numpy()).all()
    assert np.array_equal(np.load(tmp_path / "a" / "biases.npy"), np.stack([tr.engine.bias(l).numpy() for l in range(L)]))
    assert np.load(tmp_path / "a" / "loss.npy")[0] == tr.last_loss_and_grad_norm()[0]

    # the roll-back list covers every device buffer the library is handed (codae.hip.Buffers: it allocates none of its own)
    # except the per-step workspaces, and names the tensor the engine itself binds to that field
    from codae.hip import Buffers
    from codae.hip.engine import DaeEngine
    import inspect
    fields = [f for f, _ in Buffers._fields_]
    assert set(bench.STATE_BUFFERS).isdisjoint(bench.WORKSPACE_BUFFERS)
    assert set(bench.STATE_BUFFERS) | set(bench.WORKSPACE_BUFFERS) == set(fields)
    bound = re.search(r"self\.bufs = Buffers\((.*?)\)\n", inspect.getsource(DaeEngine.__init__), re.S).group(1)
    attrs = re.findall(r"ptr\(self\.(\w+)\)", bound)
    assert len(attrs) == len(fields)
    for field, attr in zip(fields, attrs):
        if field in bench.STATE_BUFFERS:
            assert attr in (bench.STATE_BUFFERS[field], "_" + bench.STATE_BUFFERS[field]), (field, attr)

    snap = bench.snapshot_state(tr)
    before = [t.clone() for t in bench._state_tensors(tr.engine)]
    for t in bench._state_tensors(tr.engine):
        t.add_(1)
    tr.engine.step_count = 77
    bench.restore_state(tr, snap)
    assert tr.engine.step_count == 0
    assert all(torch.equal(a, b) for a, b in zip(before, bench._state_tensors(tr.engine)))
