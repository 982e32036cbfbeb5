"""One gather kernel serves every width: for the same data, masks, presence table, seed and step, the 8-wide (bf16), the 4-wide and
the scalar launch of codae_corrupt_batch / codae_corrupt_batch_present give the same bits, for every noise kind (none included), with
and without a presence table, and leave the pad columns of the output alone.

The launcher chooses the width from its arguments' alignment, so the cases force it:
  x8      everything aligned, bf16 output
  x4      the mask table starts 4 bytes past an 8-byte boundary (bf16); fp32 output, everything aligned
  scalar  `data` starts one float past a 16-byte boundary; or an odd output stride
B in {1, 5, 257} (one thread group, a ragged one, more than one block's worth of 8-wide groups at io 72), io in {8, 24, 72} with
4-, 6- and 12-column slots: an 8-wide group spans two slots at io 8, 4- and 8-wide groups straddle slot borders at io 24 and 72.

Everything is torch.equal on the raw bits, Gaussian included: run against the library of the commit before the kernels were
unified, this file passed as it stands - noise_apply1 and noise_apply4 round alike there too, so no kind needs a tolerance.

The last test runs one batch past the first trip of the capped grid (B 2800, io 1536) against tests/noise_ref.py."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"

KINDS = [("none", None), ("gaussian", dict(sigma=0.3)), ("masking", dict(p=0.25)), ("salt_pepper", dict(p=0.1, lo=-0.75, hi=1.5))]
SLOTS = {8: 2, 24: 4, 72: 6}
BATCHES = (1, 5, 257)
N = 300
STEP = 7
SEED = 0x0123456789ABCDEF
POISON = 7.0
PAD = 8

_PROBLEMS = {}


def _offset_copy(t, lead, align):
    """the values of t in fresh device memory that starts `lead` bytes past a multiple of `align`"""
    flat = t.contiguous().view(-1)
    n_lead = lead // flat.element_size()
    buf = torch.empty(flat.numel() + n_lead, dtype=flat.dtype, device=DEV)
    assert buf.data_ptr() % align == 0
    out = buf[n_lead:]
    out.copy_(flat)
    assert out.data_ptr() % align == lead
    return out.view(t.shape)


def _problem(io):
    """N dataset rows (NaN-free, with zeros and negative values), one mask per slot, a presence table with about 30 % absent, a
    permuted row_idx with one dataset row twice; built once per width and never modified."""
    if io not in _PROBLEMS:
        S = SLOTS[io]
        E = io // S
        rng = np.random.default_rng(4000 + io)
        data = rng.standard_normal((N, io)).astype(np.float32)
        data[rng.random((N, io)) < 0.05] = 0.0
        table = np.ones((S, io), dtype=np.uint8)
        for m in range(S):
            table[m, m * E:(m + 1) * E] = 0
        present = (rng.random((N, S)) >= 0.3).astype(np.uint8)
        rows = rng.permutation(N)[:max(BATCHES)].astype(np.int32)
        rows[3] = rows[2]
        mask_id = rng.integers(0, S, max(BATCHES)).astype(np.int32)
        d = dict(data=torch.tensor(data, device=DEV), table=torch.tensor(table, device=DEV), present=torch.tensor(present, device=DEV),
                 rows=torch.tensor(rows, device=DEV), mask_id=torch.tensor(mask_id, device=DEV))
        d["data_off"] = _offset_copy(d["data"], 4, 16)
        d["table_off"] = _offset_copy(d["table"], 4, 8)
        assert d["data"].data_ptr() % 16 == 0 and d["table"].data_ptr() % 8 == 0
        _PROBLEMS[io] = d
    return _PROBLEMS[io]


def _gather(d, io, B, noise, pres, bf16, data="data", table="table", ld=None):
    from codae import hip
    lib = hip.lib()
    ld = io + PAD if ld is None else ld
    out = torch.full((B, ld), POISON, dtype=torch.bfloat16 if bf16 else torch.float32, device=DEV)
    batch = hip.Batch(hip.ptr(d[data]), hip.ptr(d["rows"]), hip.ptr(d["mask_id"]), hip.ptr(d[table]), B, io, None, 0, 0)
    st = None if noise is None else C.byref(noise)
    if pres:
        rc = lib.codae_corrupt_batch_present(C.byref(batch), st, STEP, None, hip.ptr(out), int(bf16), ld, hip.ptr(d["present"]), SLOTS[io],
                                             hip.current_stream())
    else:
        rc = lib.codae_corrupt_batch(C.byref(batch), st, STEP, None, hip.ptr(out), int(bf16), ld, hip.current_stream())
    assert rc == 0, lib.codae_last_error()
    return out


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("pres", [False, True], ids=["all-present", "presence"])
@pytest.mark.parametrize("kind,kw", KINDS, ids=[k for k, _ in KINDS])
def test_every_width_gives_the_same_bits(kind, kw, pres):
    from codae.tool import InputNoise
    noise = None if kw is None else InputNoise(kind, seed=SEED, **kw).as_struct()
    for io in SLOTS:
        d = _problem(io)
        for B in BATCHES:
            where = "io %d B %d" % (io, B)
            x8 = _gather(d, io, B, noise, pres, True)
            others = {"x4 bf16": _gather(d, io, B, noise, pres, True, table="table_off"),
                      "scalar bf16 (data offset)": _gather(d, io, B, noise, pres, True, data="data_off"),
                      "scalar bf16 (odd stride)": _gather(d, io, B, noise, pres, True, ld=io + PAD + 1)}
            x4 = _gather(d, io, B, noise, pres, False)
            x1 = _gather(d, io, B, noise, pres, False, data="data_off")
            torch.cuda.synchronize()
            for name, got in others.items():
                assert torch.equal(_bits(got[:, :io]), _bits(x8[:, :io])), (where, name)
                assert (got[:, io:].float() == POISON).all(), (where, name)
            assert torch.equal(_bits(x1[:, :io]), _bits(x4[:, :io])), (where, "scalar fp32")
            assert torch.equal(_bits(x4[:, :io].to(torch.bfloat16)), _bits(x8[:, :io])), (where, "fp32 rounded against bf16")
            for name, got in (("x8", x8), ("x4 fp32", x4), ("scalar fp32", x1)):
                assert (got[:, io:].float() == POISON).all(), (where, name)
            # the launches did something: the blanked slot is 0, and what is left is not the poison
            keep = d["table"][d["mask_id"][:B].long()] != 0
            assert (x4[:, :io][~keep] == 0).all() and not (x4[:, :io] == POISON).any(), where
            if pres:
                pm = d["present"][d["rows"][:B].long()].repeat_interleave(io // SLOTS[io], dim=1) != 0
                assert (_bits(x8[:, :io])[~pm] == 0).all() and (_bits(x4[:, :io])[~pm] == 0).all(), where


# ---- past the first trip of the capped grid ---------------------------------------------------------------------------------------------
BIG_B, BIG_IO, BIG_SLOTS = 2800, 1536, 6      # 2800 x 192 8-wide groups (bf16 out) and 2800 x 384 4-wide ones (fp32) against 2048 x 256 a trip
_BIG = {}


def big_groups(bf16):
    """work items of the aligned launch: 8-column groups for a bf16 output, 4-column groups for an fp32 one"""
    return BIG_B * (BIG_IO // (8 if bf16 else 4))


def _big_problem():
    """the file's N dataset rows at io 1536 in 6 slots; 2800 batch rows drawn from them (every row about nine times), one mask each"""
    if not _BIG:
        E = BIG_IO // BIG_SLOTS
        rng = np.random.default_rng(4000 + BIG_IO)
        data = rng.standard_normal((N, BIG_IO)).astype(np.float32)
        data[rng.random((N, BIG_IO)) < 0.05] = 0.0
        table = np.ones((BIG_SLOTS, BIG_IO), dtype=np.uint8)
        for m in range(BIG_SLOTS):
            table[m, m * E:(m + 1) * E] = 0
        rows = rng.integers(0, N, BIG_B).astype(np.int32)
        mask_id = rng.integers(0, BIG_SLOTS, BIG_B).astype(np.int32)
        _BIG.update(np=dict(data=data, table=table, rows=rows, mask_id=mask_id), data=torch.tensor(data, device=DEV),
                    table=torch.tensor(table, device=DEV), rows=torch.tensor(rows, device=DEV), mask_id=torch.tensor(mask_id, device=DEV))
    return _BIG


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "f32"])
@pytest.mark.parametrize("kind,kw", KINDS, ids=[k for k, _ in KINDS])
def test_a_batch_past_the_first_grid_trip_matches_the_definition(kind, kw, bf16):
    """B 2800 x io 1536: the 8-wide launch makes one trip and 2.5 % of a second, the 4-wide one two trips and 5 % of a third.
    Every kind is checked over the WHOLE matrix against tests/noise_ref.py (its Philox is whole-array numpy: under half a second
    a kind at this size, so no kind runs on a row subset) at the tolerances of tests/test_gpu_noise.py - bit for bit, Gaussian
    within its derived bound; `none` is the plain masked gather, bit for bit.  The pad columns keep their poison."""
    from codae.tool import InputNoise
    from test_gpu_noise import _check_against_reference
    d = _big_problem()
    h = d["np"]
    noise = None if kw is None else InputNoise(kind, seed=SEED, **kw).as_struct()
    got = _gather(d, BIG_IO, BIG_B, noise, False, bf16)
    torch.cuda.synchronize()
    assert (got[:, BIG_IO:].float() == POISON).all()
    x, keep = h["data"][h["rows"]], h["table"][h["mask_id"]]
    if kw is None:
        want = torch.tensor(np.where(keep != 0, x, np.float32(0))).to(got.dtype)                 # (a blanked element is +0, not x * 0)
        assert torch.equal(_bits(got[:, :BIG_IO]).cpu(), _bits(want))
    else:
        _check_against_reference(got[:, :BIG_IO], x, h["rows"], keep, STEP, kind, kw, bf16, seed=SEED)
