"""codae_corrupt_batch_image - the training step's gather from the resident bf16 image of the dataset - against the gather it
replaces: codae_corrupt_batch_present(..., out_bf16 = 1) on the fp32 rows the image was cast from, bit for bit.

The two differ in order (round then clear, against clear then round) and in how they clear (an AND on packed halves, against a
select on fp32 values), so what can go wrong is a value whose cleared form is not +0 (NaN, -0, Inf), a rounding that differs
(ties, denormals, NaN payloads: codae_cast_f32_to_bf16 must round as the gather's pack does), a group that is only partly
masked or straddles two slots, the shortcut for a wholly blanked group, and the addressing (repeated rows, a padded output row,
both mask sources).  Shapes: one group per row (io 8), three (24: slots of 8 and, with four slots, of 6 - a group then
straddles two), the benchmark's row (1536); one row, a few, and more rows than one block's threads hold groups of.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
SENTINEL = 0x7b7b       # what both outputs hold before the launch: pad columns must keep it

# slots per row of the slot-aligned mask table and the presence tables
SLOTS = {8: (2,), 24: (3, 4), 1536: (3,)}


@pytest.fixture(scope="module")
def hip():
    from codae import hip as H
    H.lib()
    return H


# fp32 bit patterns (kept as integers: a signalling NaN must reach the device as it is written here)
SPECIALS = np.array([
    0x00000000, 0x80000000,                 # +-0
    0x00000001, 0x807fffff, 0x00008000,     # denormals (the last one a tie between 0 and the smallest bf16 denormal)
    0x7f800000, 0xff800000,                 # +-Inf
    0x7fc00000, 0xffc12345, 0x7f800001, 0x7f80ffff, 0xff808000,      # quiet / signalling NaNs, payload in the low half only
    0x3f808000, 0x3f818000, 0xbf808000,     # ties: to even down, to even up, negative
    0x3f807fff, 0x3f808001,                 # just below / above a tie
    0x7f7fffff, 0x7f7f8000,                 # rounds up to Inf
], dtype=np.uint32)


def _data(N, io, seed):
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((N, io)).astype(np.float32)
    flat = d.reshape(-1).view(np.uint32)
    for i, s in enumerate(SPECIALS):        # every special lands in masked and in kept groups over the table / id combinations
        flat[i::len(SPECIALS) + 4] = s
    return d


def _tables(io, rng):
    S = SLOTS[io][0]
    E = io // S
    aligned = np.ones((S, io), np.uint8)
    for s in range(S):
        aligned[s, s * E:(s + 1) * E] = 0
    ragged = rng.choice(np.array([0, 0, 1, 2, 255], np.uint8), size=(5, io))     # any non-zero byte keeps
    ragged[0, :8] = (0, 0, 0, 0, 0, 0, 0, 1)                                      # a group with a single kept element
    return {"aligned": aligned, "ragged": ragged, "zeros": np.zeros((2, io), np.uint8), "ones": np.ones((2, io), np.uint8), "none": None}


def _presence(N, S, rng):
    t = (rng.random((N, S)) < 0.7).astype(np.uint8)
    t[0] = 1
    t[N - 1] = 0
    return t


@pytest.fixture(scope="module")
def problems(hip):
    """per io: dataset, its image (codae_cast_f32_to_bf16), mask tables, presence tables - made once, never modified"""
    out = {}
    for io in (8, 24, 1536):
        N = 150
        rng = np.random.default_rng(io)
        data = torch.tensor(_data(N, io, io), device=DEV)
        image = torch.full((N, io), float("nan"), dtype=torch.bfloat16, device=DEV)
        hip.check(hip.lib().codae_cast_f32_to_bf16(hip.ptr(data), hip.ptr(image), N * io, hip.current_stream()))
        tables = {k: (None if v is None else torch.tensor(v, device=DEV)) for k, v in _tables(io, rng).items()}
        pres = {S: torch.tensor(_presence(N, S, rng), device=DEV) for S in SLOTS[io]}
        mtu = {k: torch.tensor(rng.integers(0, t.shape[0], (N, 3)).astype(np.int32), device=DEV) for k, t in tables.items() if t is not None}
        out[io] = dict(N=N, data=data, image=image, tables=tables, pres=pres, mtu=mtu, rng=rng)
    torch.cuda.synchronize()
    return out


def _run_pair(hip, p, io, B, out_ld, rows, table_name, source, S):
    """-> (reference bits, image-path bits) as int16 [B][out_ld]"""
    lib = hip.lib()
    table = p["tables"][table_name]
    row_idx = mask_id = mask_to_use = None
    nb_run = run = 0
    if rows == "repeats":
        r = p["rng"].integers(0, p["N"], B).astype(np.int32)
        if B >= 2:
            r[B - 1] = r[0]
        row_idx = torch.tensor(r, device=DEV)
    if table is not None:
        if source == "mask_id":
            mask_id = torch.tensor(p["rng"].integers(0, table.shape[0], B).astype(np.int32), device=DEV)
        else:
            mask_to_use, nb_run, run = p["mtu"][table_name], 3, 1
    present = None if S == 0 else p["pres"][S]
    batch = hip.Batch(hip.ptr(p["data"]), hip.ptr(row_idx), hip.ptr(mask_id), hip.ptr(table), B, io, hip.ptr(mask_to_use), nb_run, run)
    ref = torch.full((B, out_ld), SENTINEL, dtype=torch.int16, device=DEV)
    got = torch.full((B, out_ld), SENTINEL, dtype=torch.int16, device=DEV)
    hip.check(lib.codae_corrupt_batch_present(C.byref(batch), None, 0, None, hip.ptr(ref), 1, out_ld, hip.ptr(present), S, hip.current_stream()))
    hip.check(lib.codae_corrupt_batch_image(C.byref(batch), hip.ptr(p["image"]), hip.ptr(present), S, hip.ptr(got), out_ld, hip.current_stream()))
    torch.cuda.synchronize()
    return ref.cpu().numpy(), got.cpu().numpy(), (row_idx, mask_id)


@pytest.mark.parametrize("B", [1, 5, 130])
@pytest.mark.parametrize("io", [8, 24, 1536])
def test_image_gather_gives_the_bits_of_the_fp32_gather(hip, problems, io, B):
    p = problems[io]
    n = 0
    for pad, rows, table_name, source, S in itertools.product((0, 8), ("repeats", "null"), ("aligned", "ragged", "zeros", "ones", "none"),
                                                              ("mask_id", "mask_to_use"), (0,) + SLOTS[io]):
        if table_name == "none" and source == "mask_to_use":
            continue                                          # (no mask: one source is enough)
        ref, got, _ = _run_pair(hip, p, io, B, io + pad, rows, table_name, source, S)
        what = (pad, rows, table_name, source, S)
        assert np.array_equal(ref, got), (what, np.argwhere(ref != got)[:4])
        assert (got[:, io:] == SENTINEL).all(), what          # pad columns are not written
        if table_name == "zeros":
            assert (got[:, :io] == 0).all(), what             # a masked NaN, Inf or -0 is +0
        n += 1
    assert n == 2 * 2 * (4 * 2 + 1) * (1 + len(SLOTS[io]))


@pytest.mark.parametrize("io", [8, 24, 1536])
def test_the_cast_rounds_as_the_gather_packs(hip, problems, io):
    """no mask, no presence, every dataset row: the image itself against the fp32 gather's output, NaNs, ties and denormals included"""
    p = problems[io]
    ref, got, _ = _run_pair(hip, p, io, p["N"], io, "null", "none", "mask_id", 0)
    image = p["image"].view(torch.int16).cpu().numpy()
    assert np.array_equal(ref, image) and np.array_equal(got, image)
    f = p["data"].cpu().numpy().reshape(-1).view(np.uint32)
    for s in SPECIALS:                                          # the fixture really holds every special value
        assert (f == s).any(), hex(int(s))


def test_a_blanked_slot_is_zero_whatever_the_image_holds_there(hip, problems):
    """slot-aligned masks at io 1536 (the shortcut that stores zeros without loading): the masked slot is +0 bits, the other two are the
    image's rows"""
    io, B = 1536, 130
    p = problems[io]
    _, got, (row_idx, mask_id) = _run_pair(hip, p, io, B, io, "repeats", "aligned", "mask_id", 0)
    image = p["image"].view(torch.int16).cpu().numpy()
    r, m = row_idx.cpu().numpy(), mask_id.cpu().numpy()
    E = io // 3
    for b in range(B):
        for s in range(3):
            want = 0 if m[b] == s else image[r[b], s * E:(s + 1) * E]
            assert np.array_equal(got[b, s * E:(s + 1) * E], np.broadcast_to(want, (E,))), (b, s)


def test_misaligned_arguments_are_refused(hip, problems):
    p = problems[24]
    lib = hip.lib()
    out = torch.zeros((4, 40), dtype=torch.int16, device=DEV)
    batch = hip.Batch(hip.ptr(p["data"]), None, None, None, 4, 24, None, 0, 0)
    assert lib.codae_corrupt_batch_image(C.byref(batch), hip.ptr(p["image"]), None, 0, hip.ptr(out), 28, hip.current_stream()) != 0     # out_ld % 8
    assert lib.codae_corrupt_batch_image(C.byref(batch), None, None, 0, hip.ptr(out), 24, hip.current_stream()) != 0                      # no image
    odd = hip.Batch(hip.ptr(p["data"]), None, None, None, 4, 12, None, 0, 0)
    assert lib.codae_corrupt_batch_image(C.byref(odd), hip.ptr(p["image"]), None, 0, hip.ptr(out), 16, hip.current_stream()) != 0        # io % 8
    torch.cuda.synchronize()
    assert int(out.abs().max()) == 0                          # nothing was launched
