"""Table-addressed kernels past 2^31 elements and 4 GiB offsets, on a real MI355X (shapes: tests/far_offsets.py; the evidence that a
32-bit slip would show: tests/test_far_offset_shapes_host.py; layout and reasons: DESIGN.md, "Far offsets").

Every big table is a view into one arena of NaN fill (every aligned 16-bit word 0x7fc0) that starts 8 GiB above the arena's base,
so the address a truncated offset reaches lies inside the arena and holds NaN or another row: a failed assertion, never an illegal
access.  Only the probe rows - the rows on either side of element offsets 2^31 and 2^32 and byte offset 2^32, and the last row -
are written, on the device; the host never holds a big table.

The reference is the SAME entry point on a compact table: the probe rows read back out of the far table into a fresh allocation of a
few dozen rows, the row indices remapped.  The far call must give the bits of the near call.  Where a Philox key is tied to the row
id the near call keeps the key and moves only the address (noise_rows = the true far rows on a batch gathered beforehand); where an
entry point cannot separate the two (the loss sweeps under replacing noise, swap noise with a far pool) the far call is held to the
host statement and the tolerance of that entry point's own test, fed the true row ids."""
import ctypes as C

import numpy as np
import pytest

import far_offsets as F

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
FILL16S = np.uint16(F.FILL16).view(np.int16).item()
STEP = 7
SEED = 0x0123456789ABCDEF
B = F.B
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "u8": torch.uint8}
ES = {"f32": 4, "bf16": 2, "u8": 1}


@pytest.fixture(scope="module")
def hip():
    from codae import hip as H
    H.lib()
    return H


def _bits(t):
    t = t.contiguous()
    return t.view({torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype, t.dtype))


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _filled(shape, dtype):
    """a small device tensor holding the arena's fill"""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    return torch.full(((n + 1) // 2,), FILL16S, dtype=torch.int16, device=DEV).view(torch.uint8)[:n].view(dtype).view(shape)


def _is_fill(t):
    """every element of t still holds the fill.  Bytes: 0xc0 at even addresses and 0x7f at odd ones (the arena and every fresh
    allocation start on an even address)"""
    if t.element_size() == 1:
        odd = torch.full(t.shape, t.data_ptr() % 2, dtype=torch.int64, device=DEV)
        for dim, n in enumerate(t.shape):
            shape = [n if i == dim else 1 for i in range(t.dim())]
            odd = odd + torch.arange(n, device=DEV).view(shape) * (t.stride(dim) % 2)
        want = torch.where(odd % 2 == 1, 0x7F, 0xC0).to(torch.uint8)
        return bool((t == want).all())
    raw = t.contiguous().view(torch.uint8)
    assert raw.numel() % 2 == 0
    return bool((raw.view(torch.int16) == FILL16S).all())


class Arena:
    """One uint8 device tensor of fill.  flat() hands out a view that starts `head` bytes above its base; touch() records every
    range written through such a view, and wipe() refills them, so that the next table finds nothing but fill."""

    def __init__(self, n_bytes, head):
        self.raw = torch.empty(n_bytes, dtype=torch.uint8, device=DEV)
        self.raw.view(torch.int16).fill_(FILL16S)
        self.head = head
        self.dirty = []            # (byte offset, bytes)
        self.key, self.value = None, None

    def flat(self, dtype, n_elems):
        es = torch.empty((), dtype=dtype).element_size()
        assert self.head + n_elems * es <= self.raw.numel()
        return self.raw[self.head:self.head + n_elems * es].view(dtype)

    def wipe(self):
        for off, n in self.dirty:
            lo, hi = off - off % 2, off + n + (off + n) % 2
            self.raw[lo:hi].view(torch.int16).fill_(FILL16S)
        self.dirty = []
        self.key = self.value = None

    def touch(self, t):
        """t: a view into the arena that is about to be, or may have been, written"""
        es = t.element_size()
        off = t.data_ptr() - self.raw.data_ptr()
        if t.dim() == 2 and t.stride(0) != t.shape[1]:
            for r in range(t.shape[0]):
                self.dirty.append((off + r * t.stride(0) * es, t.shape[1] * es))
        else:
            assert t.is_contiguous()
            self.dirty.append((off, t.numel() * es))

    def claim(self, key, build):
        """the arena holds one problem at a time; the same key again gets the same object"""
        if self.key != key:
            self.wipe()
            self.value = build()
            self.key = key
        return self.value


class Arenas:
    """the big arena, and the image arena while somebody needs it (the inventory readers give its 8 GiB back for their row-keyed
    tables; it comes back filled on the next use)"""

    def __init__(self):
        self.big = Arena(F.ARENA_BYTES, F.HEADROOM)
        self._img = None

    @property
    def img(self):
        if self._img is None:
            self._img = Arena(F.IMAGE_ARENA_BYTES, F.IMAGE_HEADROOM)
        return self._img

    def release_image(self):
        if self._img is not None:
            self._img.raw = self._img.value = None
            self._img = None
            torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def arenas():
    need = F.ARENA_BYTES + F.IMAGE_ARENA_BYTES
    free, _ = torch.cuda.mem_get_info()
    if free < need + 4 * F.GIB:
        pytest.skip("the far-offset arenas need %d bytes plus 4 GiB of room (%d); the device has %d free" % (need, need + 4 * F.GIB, free))
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    a = Arenas()
    a.img
    torch.cuda.synchronize()
    yield a
    peak = torch.cuda.max_memory_allocated()
    print("far offsets: peak device memory %.2f GiB of the %d GiB cap" % (peak / F.GIB, F.CAP_BYTES // F.GIB))
    a.release_image()
    a.big.raw = a.big.value = None
    del a.big
    torch.cuda.empty_cache()
    assert peak <= F.CAP_BYTES, peak


class FarTable:
    """[n][io] of `kind` elements in an arena; rows: the distinct probe rows (plus `extra` rows beside them), ascending; near: those
    rows read back into a compact table; idx(far rows) -> near rows."""

    def __init__(self, arena, io, kind, n=None, extra=0, seed=0, fill_rows=True):
        self.io, self.kind, self.dtype, self.es = io, kind, DT[kind], ES[kind]
        self.n = F.n_obs(io, self.es) if n is None else n
        self.arena, self._near = arena, None
        self.flat = arena.flat(self.dtype, self.n * io + F.GUARD)
        self.t = self.flat[:self.n * io].view(self.n, io)
        probes = F.distinct_rows(io, self.es, self.n)
        rows = set(probes)
        for r in probes:                                   # `extra` rows beside every probe row, inside the table
            for k in range(1, extra + 1):
                if 0 <= r - 2 - k:
                    rows.add(r - 2 - k)
        self.rows = sorted(rows)
        self.probes = probes
        self.pos = {r: i for i, r in enumerate(self.rows)}
        if fill_rows:
            rng = np.random.default_rng(1000 + io + 7 * self.es + seed)
            v = rng.standard_normal((len(self.rows), io)).astype(np.float32)
            v[rng.random(v.shape) < 0.05] = 0.0
            vals = torch.tensor(v, device=DEV).to(self.dtype) if kind != "u8" else torch.tensor(rng.integers(0, 3, v.shape).astype(np.uint8), device=DEV)
            self.write(self.rows, vals)

    def write(self, rows, vals):
        """vals [len(rows)][io] -> the far rows; runs of consecutive rows in one copy"""
        i = 0
        while i < len(rows):
            j = i
            while j + 1 < len(rows) and rows[j + 1] == rows[j] + 1:
                j += 1
            dst = self.t[rows[i]:rows[j] + 1]
            self.arena.touch(dst)
            dst.copy_(vals[i:j + 1])
            i = j + 1
        self._near = None

    @property
    def near(self):
        """the written rows read back out of the far table, at the start of a fresh small allocation"""
        if self._near is None:
            self._near = torch.stack([self.t[r] for r in self.rows]).clone()
        return self._near

    def idx(self, far_rows):
        return [self.pos[int(r)] for r in far_rows]

    def batch(self, seed=1):
        """(far row_idx int32 [B], near row_idx int32 [B], the far rows as a list)"""
        rows = F.batch_rows(self.io, self.es, seed, self.n)
        return _i32(rows), _i32(self.idx(rows)), rows

    def guard_ok(self):
        return _is_fill(self.flat[self.n * self.io:])


def _i32(v):
    return torch.tensor(np.asarray(v, dtype=np.int64).astype(np.int32), device=DEV)


def _dataset(arenas, io, extra=0):
    return arenas.big.claim(("f32", io, extra), lambda: FarTable(arenas.big, io, "f32", extra=extra))


def _masks(io, S):
    """one mask per slot and the batch's mask ids"""
    E = io // S
    table = np.ones((S, io), dtype=np.uint8)
    for s in range(S):
        table[s, s * E:(s + 1) * E] = 0
    mask_id = np.random.default_rng(io).integers(0, S, B).astype(np.int32)
    return torch.tensor(table, device=DEV), torch.tensor(mask_id, device=DEV)


def _noise(kind):
    from codae.tool import InputNoise
    kw = {"gaussian": dict(sigma=0.3), "masking": dict(p=0.25), "salt_pepper": dict(p=0.1, lo=-0.75, hi=1.5)}
    return None if kind == "none" else InputNoise(kind, seed=SEED, **kw[kind])


def _presence(n, S, rows, seed=0):
    """present [n][S] uint8 on the device: ones, with about a third of the slots of the given rows absent (never a whole row)"""
    t = torch.ones((n, S), dtype=torch.uint8, device=DEV)
    rng = np.random.default_rng(50 + seed)
    sub = (rng.random((len(rows), S)) >= 0.35).astype(np.uint8)
    sub[np.arange(len(rows)), rng.integers(0, S, len(rows))] = 1
    assert (sub == 0).any()
    t[torch.tensor(np.asarray(rows, dtype=np.int64), device=DEV)] = torch.tensor(sub, device=DEV)
    return t, sub


def _out(io, bf16, rows=B):
    """an output of `rows` rows with a guard band of F.GUARD fill elements behind every row"""
    return _filled((rows, io + F.GUARD), torch.bfloat16 if bf16 else torch.float32)


def _guards_ok(out, io):
    return _is_fill(out[:, io:])


# ---- dataset readers --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("io", F.WIDTHS)
def test_cast_over_the_whole_far_table(hip, arenas, io):
    """codae_cast_f32_to_bf16 over all 2^31 + 2^20 elements, into the image arena: the probe rows have the bits of the cast of the
    compact table, a row of fill is the cast of fill, and the 64 elements behind the image's last row keep the fill."""
    d = _dataset(arenas, io)
    arenas.img.wipe()
    n = d.n * io
    image = arenas.img.flat(torch.bfloat16, n + F.GUARD)
    arenas.img.dirty.append((arenas.img.head, n * 2))
    hip.check(hip.lib().codae_cast_f32_to_bf16(hip.ptr(d.t), hip.ptr(image), n, hip.current_stream()))
    near = torch.cat([d.near, _filled((1, io), torch.float32)])
    want = _filled(near.shape, torch.bfloat16)
    hip.check(hip.lib().codae_cast_f32_to_bf16(hip.ptr(near), hip.ptr(want), near.numel(), hip.current_stream()))
    torch.cuda.synchronize()
    img = image[:n].view(d.n, io)
    got = torch.stack([img[r] for r in d.rows])
    assert _same(got, want[:-1]) and not torch.isnan(got.float()).any()
    for r in (0, 12345, d.rows[0] - 1, d.rows[-1] - 1):
        assert r not in d.pos and _same(img[r], want[-1]) and torch.isnan(img[r].float()).all(), r
    assert _is_fill(image[n:])
    assert d.guard_ok()
    arenas.img.wipe()
    torch.cuda.synchronize()


def _gather(hip, data, row_idx, mask_id, table, io, out, noise=None, noise_rows=None, present=None, S=0, mask_to_use=None, run=0):
    lib = hip.lib()
    batch = hip.Batch(hip.ptr(data), hip.ptr(row_idx), hip.ptr(mask_id), hip.ptr(table), B, io, hip.ptr(mask_to_use),
                      0 if mask_to_use is None else int(mask_to_use.shape[1]), run)
    st = None if noise is None else noise.as_struct()
    bf16 = int(out.dtype == torch.bfloat16)
    args = (C.byref(batch), None if st is None else C.byref(st), STEP, hip.ptr(noise_rows), hip.ptr(out), bf16, out.stride(0))
    if present is None:
        hip.check(lib.codae_corrupt_batch(*args, hip.current_stream()))
    else:
        hip.check(lib.codae_corrupt_batch_present(*args, hip.ptr(present), S, hip.current_stream()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("pres", [False, True], ids=["all-present", "presence"])
@pytest.mark.parametrize("kind", ["none", "gaussian", "masking", "salt_pepper"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("io", F.WIDTHS)
def test_corrupt_batch_from_far_rows(hip, arenas, io, bf16, kind, pres):
    """codae_corrupt_batch / _present: 70 far rows through row_idx against the same rows gathered beforehand, row_idx NULL and
    noise_rows = the far rows (the Philox key and the presence key stay the far row; only the address moves); without noise the near
    call reads the compact table through remapped indices.  Padded out_ld, guard bands."""
    d = _dataset(arenas, io)
    S = F.SLOTS[io]
    far_idx, near_idx, rows = d.batch()
    table, mask_id = _masks(io, S)
    noise = _noise(kind)
    present = near_present = None
    if pres:
        present, sub = _presence(d.n, S, d.rows)
        near_present = torch.tensor(sub, device=DEV)
    got = _gather(hip, d.t, far_idx, mask_id, table, io, _out(io, bf16), noise, None, present, S)
    if noise is None:
        want = _gather(hip, d.near, near_idx, mask_id, table, io, _out(io, bf16), None, None, near_present, S)
    else:
        gathered = d.near[near_idx.long()].clone()
        want = _gather(hip, gathered, None, mask_id, table, io, _out(io, bf16), noise, far_idx, present, S)
    assert _same(got, want), (io, bf16, kind, pres)
    assert _guards_ok(got, io) and d.guard_ok()
    v = got[:, :io].float()
    assert not torch.isnan(v).any() and bool((v != 0).any())
    keep = table[mask_id.long()] != 0
    assert bool((v[~keep] == 0).all())                                            # the blank lies behind every noise kind


def test_corrupt_batch_looks_its_mask_up_by_the_far_row(hip, arenas):
    """the mask_to_use route: the id of batch row b is mask_to_use[row_idx[b] * nb_run + run], a table keyed by the far row"""
    io, S, nb_run, run = 1536, F.SLOTS[1536], 2, 1
    d = _dataset(arenas, io)
    far_idx, near_idx, rows = d.batch(seed=2)
    table, _ = _masks(io, S)
    rng = np.random.default_rng(3)
    ids = rng.integers(1, S, (len(d.rows), nb_run)).astype(np.int32)
    mtu = torch.zeros((d.n, nb_run), dtype=torch.int32, device=DEV)                # mask 0 wherever no probe row is: never a probe row's id
    mtu[torch.tensor(np.asarray(d.rows), device=DEV)] = torch.tensor(ids, device=DEV)
    near_mtu = torch.tensor(ids, device=DEV)
    for bf16 in (False, True):
        for kind in ("none", "masking"):
            noise = _noise(kind)
            got = _gather(hip, d.t, far_idx, None, table, io, _out(io, bf16), noise, None, mask_to_use=mtu, run=run)
            mask_id = torch.tensor(ids[d.idx(rows), run], device=DEV)
            if noise is None:
                want = _gather(hip, d.near, near_idx, None, table, io, _out(io, bf16), mask_to_use=near_mtu, run=run)
            else:
                want = _gather(hip, d.near[near_idx.long()].clone(), None, mask_id, table, io, _out(io, bf16), noise, far_idx)
            assert _same(got, want), (bf16, kind)
            assert not torch.isnan(got[:, :io].float()).any() and _guards_ok(got, io)


def _image_gather(hip, image, row_idx, mask_id, table, io, present, S):
    out = _out(io, True)
    batch = hip.Batch(None, hip.ptr(row_idx), hip.ptr(mask_id), hip.ptr(table), B, io, None, 0, 0)
    hip.check(hip.lib().codae_corrupt_batch_image(C.byref(batch), hip.ptr(image), hip.ptr(present), S, hip.ptr(out), out.stride(0),
                                                  hip.current_stream()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("which", ["past-2^32-elements", "dataset-image"])
@pytest.mark.parametrize("io", F.WIDTHS)
def test_corrupt_batch_image_from_far_rows(hip, arenas, io, which):
    """the bf16 image: a table of 2^32 + 2^20 elements in the big arena (rows on either side of 2^31 and 2^32 elements), and the
    image of the fp32 dataset in the second arena with a presence table keyed by the far row"""
    S = F.SLOTS[io]
    table, mask_id = _masks(io, S)
    if which == "dataset-image":
        d = arenas.img.claim(("image", io), lambda: FarTable(arenas.img, io, "bf16", n=F.n_obs(io, 4)))
        present, sub = _presence(d.n, S, d.rows)
        near_present = torch.tensor(sub, device=DEV)
    else:
        d = arenas.big.claim(("bf16", io), lambda: FarTable(arenas.big, io, "bf16"))
        present = near_present = None
        assert d.n * io > 2 ** 32
    far_idx, near_idx, rows = d.batch()
    got = _image_gather(hip, d.t, far_idx, mask_id, table, io, present, S)
    want = _image_gather(hip, d.near, near_idx, mask_id, table, io, near_present, S)
    assert _same(got, want) and _guards_ok(got, io) and d.guard_ok()
    v = got[:, :io].float()
    assert not torch.isnan(v).any() and bool((v != 0).any())
    got = _image_gather(hip, d.t, far_idx, None, None, io, None, 0)                # no mask: the rows themselves
    assert _same(got[:, :io], d.near[near_idx.long()])


class _Rows:
    """the far table as tests/swap_ref.py indexes it: data[row, columns] of the written rows only"""

    def __init__(self, d, host):
        self.d, self.host, self.shape = d, host, (d.n, d.io)

    def __getitem__(self, key):
        r, cols = key
        return self.host[self.d.pos[int(r)], cols]


class _Present:
    def __init__(self, d, sub):
        self.d, self.sub = d, sub

    def __getitem__(self, r):
        return self.sub[self.d.pos[int(r)]]


@pytest.mark.parametrize("image", [False, True], ids=["f32", "image"])
@pytest.mark.parametrize("io", F.WIDTHS)
def test_corrupt_batch_swap_with_a_pool_of_far_rows(hip, arenas, io, image):
    """the swapped-in slot comes from pool[j], a far row: held bit for bit (tests/test_gpu_swap_noise.py compares bits: nothing is
    computed on the values) to tests/swap_ref.py fed the true row ids - the draw is keyed by the far row and cannot be moved"""
    import swap_ref as SR
    from codae.tool import InputNoise
    S, p, out_bf16 = F.SLOTS[io], 0.6, image
    if image:
        d = arenas.big.claim(("bf16", io), lambda: FarTable(arenas.big, io, "bf16"))
    else:
        d = _dataset(arenas, io)
    far_idx, near_idx, rows = d.batch(seed=3)
    table, mask_id = _masks(io, S)
    pool = np.asarray(d.rows, dtype=np.int64)
    present, sub = _presence(d.n, S, d.rows, seed=1)
    host = d.near.float().cpu().numpy()
    keep = table.cpu().numpy()[mask_id.cpu().numpy()]
    noise = InputNoise("swap", p=p, seed=SR.SEED, pool=pool.astype(np.int32))
    st = noise.as_struct()
    pool_t = _i32(pool)
    sw = hip.Swap(hip.ptr(pool_t), len(pool), S)
    for pres_t, pres_ref in ((None, None), (present, _Present(d, sub.astype(bool)))):
        ref, cls = SR.corrupt(host[d.idx(rows)], _Rows(d, host), rows, STEP, S, p, SR.SEED, pool, pres_ref, keep)
        assert (cls == 3).sum() > B // 2 and (cls == 0).any()
        out = _out(io, out_bf16)
        batch = hip.Batch(hip.ptr(d.t), hip.ptr(far_idx), hip.ptr(mask_id), hip.ptr(table), B, io, None, 0, 0)
        hip.check(hip.lib().codae_corrupt_batch_swap(C.byref(batch), C.byref(st), STEP, None, None, C.byref(sw),
                                                     hip.ptr(out), int(out_bf16), out.stride(0), hip.ptr(pres_t), int(image), hip.current_stream()))
        torch.cuda.synchronize()
        want = torch.tensor(ref, device=DEV).to(out.dtype)
        assert _same(out[:, :io], want), (io, image, pres_t is None)
        assert _guards_ok(out, io) and d.guard_ok()


# ---- the loss sweeps --------------------------------------------------------------------------------------------------------------------

def _loss_problem(d, io):
    rng = np.random.default_rng(90 + io)
    y = torch.tensor(rng.standard_normal((B, io)).astype(np.float32), device=DEV)
    cw = torch.tensor(np.repeat(np.float32([0.5, 1.0, 2.0]), io // 3), device=DEV)
    return y, cw


def _loss_outputs_equal(far, near, io):
    for a, b in zip(far[1:], near[1:]):
        assert _same(a, b)
    assert far[0] == 0 and near[0] == 0
    assert not torch.isnan(far[1][:, :io].float()).any() and not torch.isnan(far[3]).any()


@pytest.mark.parametrize("dy_bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("io", F.WIDTHS)
def test_emph_loss_reads_its_targets_from_far_rows(hip, arenas, io, dy_bf16):
    """codae_emph_loss: without replacing noise nothing is keyed by the row, so the far call has the bits of the near call - dY with
    its pad columns, the partial column sums, the per-block sums; under MASKING noise the weights are keyed by the far row: the far
    call is held to tests/emphasis_ref.py with the tolerances of tests/test_gpu_emphasis.py."""
    import test_gpu_emphasis as TE
    from codae.tool import InputNoise
    d = _dataset(arenas, io)
    S = F.SLOTS[io]
    far_idx, near_idx, rows = d.batch(seed=4)
    table, mask_id = _masks(io, S)
    y, cw = _loss_problem(d, io)
    kw = dict(col_weight=cw, dy_bf16=dy_bf16, dy_ld=io + F.GUARD, mask_id=mask_id, table=table)
    far = TE.emph_loss(d.t, y, None, STEP, TE.ALPHA, TE.BETA, row_idx=far_idx, **kw)
    near = TE.emph_loss(d.near, y, None, STEP, TE.ALPHA, TE.BETA, row_idx=near_idx, **kw)
    _loss_outputs_equal(far, near, io)
    noise = InputNoise("masking", seed=TE.SEED, p=0.25)
    out = TE.emph_loss(d.t, y, noise, TE.STEP, TE.ALPHA, TE.BETA, row_idx=far_idx, **kw)
    x = d.near[near_idx.long()].cpu().numpy()
    keep = table.cpu().numpy()[mask_id.cpu().numpy()]
    TE._check_against_reference(out, x, y.cpu().numpy(), np.asarray(rows), keep, ("masking", dict(p=0.25), TE.SEED), cw.cpu().numpy(), B, io, dy_bf16)
    assert d.guard_ok()


@pytest.mark.parametrize("dy_bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("io", F.WIDTHS)
def test_mse_loss_present_reads_its_targets_from_far_rows(hip, arenas, io, dy_bf16):
    """codae_mse_loss_present, with a presence table keyed by the far row (far call) and by the compact row (near call): equal bits"""
    import test_gpu_presence as TP
    d = _dataset(arenas, io)
    S = F.SLOTS[io]
    far_idx, near_idx, rows = d.batch(seed=5)
    table, mask_id = _masks(io, S)
    y, _ = _loss_problem(d, io)
    present, sub = _presence(d.n, S, d.rows, seed=2)
    kw = dict(dy_bf16=dy_bf16, dy_ld=io + F.GUARD, mask_id=mask_id, table=table)
    far = TP.loss_call("mse", d.t, y, present, S, row_idx=far_idx, **kw)
    near = TP.loss_call("mse", d.near, y, torch.tensor(sub, device=DEV), S, row_idx=near_idx, **kw)
    _loss_outputs_equal(far, near, io)
    absent = torch.tensor(np.repeat(sub[d.idx(rows)] == 0, io // S, axis=1), device=DEV)
    assert bool((_bits(far[1][:, :io])[absent] == 0).all()) and bool(absent.any())
    assert (far[1][:, io:].float() == TP.FILL).all() and d.guard_ok()


@pytest.mark.parametrize("kind", ["huber", "slot_cosine"])
@pytest.mark.parametrize("dy_bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("io", F.WIDTHS)
def test_recon_loss_reads_its_targets_from_far_rows(hip, arenas, io, dy_bf16, kind):
    """codae_recon_loss_fwd_bwd with Huber (the element-wise sweep) and the slot cosine (the per-slot sweep), with emphasis: far
    equals near bit for bit without replacing noise; Huber under MASKING noise is held to tests/recon_loss_ref.py with the checks of
    tests/test_gpu_recon_loss.py"""
    import emphasis_ref as ER
    import recon_loss_ref as RR
    import test_gpu_recon_loss as TR
    from codae.tool import InputNoise
    d = _dataset(arenas, io)
    S = F.SLOTS[io]
    far_idx, near_idx, rows = d.batch(seed=6)
    table, mask_id = _masks(io, S)
    y, cw = _loss_problem(d, io)
    loss = TR._struct(kind, 0.75 if kind == "huber" else None, 0.5 if kind == "slot_cosine" else 0.0, S if kind == "slot_cosine" else 0)
    kw = dict(emph=(TR.ALPHA, TR.BETA, cw), dy_bf16=dy_bf16, dy_ld=io + F.GUARD, mask_id=mask_id, table=table)
    far = TR.recon_loss(d.t, y, None, STEP, loss, row_idx=far_idx, **kw)
    near = TR.recon_loss(d.near, y, None, STEP, loss, row_idx=near_idx, **kw)
    _loss_outputs_equal(far, near, io)
    assert (far[1][:, io:].float() == 7.0).all() and d.guard_ok()
    if kind == "huber":
        noise = InputNoise("masking", seed=TR.SEED, p=0.25)
        out = TR.recon_loss(d.t, y, noise, TR.STEP, loss, row_idx=far_idx, **kw)
        x = d.near[near_idx.long()].cpu().numpy()
        keep = table.cpu().numpy()[mask_id.cpu().numpy()]
        w = ER.weights(ER.corrupted(keep, np.asarray(rows), TR.STEP, ("masking", dict(p=0.25), TR.SEED)), TR.ALPHA, TR.BETA, cw.cpu().numpy())
        ref = RR.loss_terms("huber", x, y.cpu().numpy(), keep, w, np.float32(1.0 / (B * io)), param=0.75)
        TR._check_elementwise(out, ref, keep, B, io, dy_bf16)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("io", F.WIDTHS)
def test_slot_contrast_prepare_samples_its_candidates_from_a_far_table(hip, arenas, io, bf16):
    """the candidates' unit vectors, row-major and transposed, have the bits of the near call whose pool holds the compact rows in
    the same order (the draw j depends on the pool's length alone); the recorded ids are the far rows"""
    lib = hip.lib()
    d = _dataset(arenas, io)
    S, K = F.SLOTS[io], 33
    E = io // S
    ws_bytes = lib.codae_slot_contrast_ws_bytes(S, K, E, int(bf16))
    kpad, epad = (K + 31) // 32 * 32, (E + 31) // 32 * 32
    mat = S * kpad * epad * (2 if bf16 else 4)
    assert ws_bytes == 2 * mat + S * kpad * 4                                     # csrc/slot_contrast.hip, ws_layout
    pool_far, pool_near = _i32(d.rows), _i32(range(len(d.rows)))
    ws = []
    for data, n_rows, pool in ((d.t, d.n, pool_far), (d.near, len(d.rows), pool_near)):
        w = torch.full((ws_bytes + 2 * F.GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
        st = hip.SlotContrast(S, K, 0.1, 0.7, 0x5EED0000C0DA0001, n_rows, len(d.rows), ws_bytes, hip.ptr(pool), None, hip.ptr(w))
        hip.check(lib.codae_slot_contrast_prepare(hip.ptr(data), io, C.byref(st), STEP, int(bf16), hip.current_stream()))
        torch.cuda.synchronize()
        assert bool((w[ws_bytes:] == 0xFF).all())
        ws.append(w)
    assert torch.equal(ws[0][:2 * mat], ws[1][:2 * mat])
    vecs = ws[0][:2 * mat].view(torch.bfloat16 if bf16 else torch.float32).float()
    assert not torch.isnan(vecs).any() and bool((vecs != 0).any())
    ids_far = ws[0][2 * mat:ws_bytes].view(torch.int32).view(S, kpad)[:, :K].cpu().numpy()
    ids_near = ws[1][2 * mat:ws_bytes].view(torch.int32).view(S, kpad)[:, :K].cpu().numpy()
    assert np.array_equal(ids_far, np.asarray(d.rows)[ids_near]) and len(set(ids_far.ravel())) > len(d.rows) // 2
    assert d.guard_ok()


# ---- assembled outfits ------------------------------------------------------------------------------------------------------------------

def _items(d, Q=37, seed=0):
    """outfits of far rows: mixed rows, one row in every slot, an empty slot (-1), every written row at least once"""
    rng = np.random.default_rng(seed)
    rows = np.asarray(d.rows, dtype=np.int64)
    S = F.SLOTS[d.io]
    items = rows[rng.integers(0, len(rows), (Q, S))]
    k = min(Q - 2, len(rows) // S)
    items[:k] = rows[:k * S].reshape(k, S)
    items[Q - 1] = rows[-1]
    items[Q - 2, 1] = -1
    near = np.where(items >= 0, np.vectorize(lambda r: d.pos.get(int(r), -1))(items), -1)
    return items, near


@pytest.mark.parametrize("form", ["blank", "loo"])
@pytest.mark.parametrize("src", ["f32", "f32-to-bf16", "bf16"])
@pytest.mark.parametrize("io", F.WIDTHS)
def test_assemble_outfits_from_far_rows(hip, arenas, io, src, form):
    lib = hip.lib()
    S = F.SLOTS[io]
    d = arenas.big.claim(("bf16", io), lambda: FarTable(arenas.big, io, "bf16")) if src == "bf16" else _dataset(arenas, io)
    items, near_items = _items(d)
    Q = len(items)
    present, sub = _presence(d.n, S, d.rows, seed=3)
    blank = None if form == "loo" else torch.tensor(np.random.default_rng(1).integers(-1, S, Q).astype(np.int32), device=DEV)
    rows_out = Q * S if form == "loo" else Q
    out_bf16 = src != "f32"
    outs = []
    for data, n_rows, it, pres in ((d.t, d.n, items, present), (d.near, len(d.rows), near_items, torch.tensor(sub, device=DEV))):
        out = _out(io, out_bf16, rows_out)
        it_t = _i32(it)
        hip.check(lib.codae_assemble_outfits(hip.ptr(data), int(src == "bf16"), n_rows, io, S, hip.ptr(it_t), Q, hip.ptr(blank), int(form == "loo"),
                                             hip.ptr(pres), hip.ptr(out), int(out_bf16), out.stride(0), hip.current_stream()))
        torch.cuda.synchronize()
        outs.append(out)
    assert _same(outs[0], outs[1]) and _guards_ok(outs[0], io) and d.guard_ok()
    v = outs[0][:, :io].float()
    assert not torch.isnan(v).any() and bool((v != 0).any())


@pytest.mark.parametrize("io", F.WIDTHS)
def test_outfit_scores_read_their_items_from_far_rows(hip, arenas, io):
    lib = hip.lib()
    S = F.SLOTS[io]
    d = _dataset(arenas, io)
    items, near_items = _items(d, seed=1)
    Q = len(items)
    present, sub = _presence(d.n, S, d.rows, seed=4)
    Y = torch.tensor(np.random.default_rng(5).standard_normal((Q * S, io + 8)).astype(np.float32), device=DEV)
    res = []
    for data, n_rows, it, pres in ((d.t, d.n, items, present), (d.near, len(d.rows), near_items, torch.tensor(sub, device=DEV))):
        cos, sq = _filled((Q * S + F.GUARD,), torch.float32), _filled((Q * S + F.GUARD,), torch.float32)
        score, npres = _filled((Q + F.GUARD,), torch.float32), torch.full((Q + F.GUARD,), -7, dtype=torch.int32, device=DEV)
        it_t = _i32(it)
        hip.check(lib.codae_outfit_scores(hip.ptr(data), n_rows, io, S, hip.ptr(it_t), Q, hip.ptr(pres), hip.ptr(Y), Y.stride(0), hip.ptr(cos),
                                          hip.ptr(sq), hip.ptr(score), hip.ptr(npres), hip.current_stream()))
        torch.cuda.synchronize()
        assert _is_fill(cos[Q * S:]) and _is_fill(sq[Q * S:]) and _is_fill(score[Q:]) and bool((npres[Q:] == -7).all())
        res.append((cos, sq, score, npres))
    for a, b in zip(*res):
        assert _same(a, b)
    cos, sq, score, npres = res[0]
    assert not torch.isnan(cos[:Q * S]).any() and not torch.isnan(sq[:Q * S]).any() and bool((sq[:Q * S] > 0).any())
    assert bool((npres[:Q] >= 2).any()) and bool(torch.isfinite(score[:Q][npres[:Q] >= 2]).all())
    assert d.guard_ok()


# ---- leading dimensions -----------------------------------------------------------------------------------------------------------------
# B = 70 rows `ld` apart: row 68 ends on the top boundary of its element size (2^31 elements of fp32, 2^32 of bf16 and of the mask
# bytes) and row 69 lies wholly above it.  Several matrices of one call share the arena: their bases are SLOT_BYTES apart and their
# rows interleave (a row and its guard band are shorter than that, the row spacings are 60 MiB and more).
SLOT_BYTES = 16384
# (bf16, width): the widths of the small kernel files - the bf16 16-byte path, the fp32 element path, the fp32 16-byte path ending in
# half a chunk, and the same three at the headline width
LD_SHAPES = [(True, 24), (False, 21), (False, 20), (True, 1536), (False, 1537), (False, 1540)]
LD_IDS = ["bf16-w24", "f32-w21-elem", "f32-w20", "bf16-w1536", "f32-w1537-elem", "f32-w1540"]


class FarMatrix:
    """values [B][width] at rows far_ld apart, slot `k` of the big arena; every row is followed by F.GUARD elements of fill"""

    def __init__(self, arena, kind, values, k):
        self.kind, self.dtype, es = kind, DT[kind], ES[kind]
        self.width = int(values.shape[1])
        self.ld = F.far_ld(es, {4: 4, 2: 8, 1: 1}[es])
        assert (self.width + F.GUARD) * es + 256 <= SLOT_BYTES and F.ld_span_bytes(es, 1, self.width) + (k + 1) * SLOT_BYTES <= F.TABLE_REGION + F.TAIL
        n = (B - 1) * self.ld + self.width + F.GUARD
        flat = arena.raw[arena.head + k * SLOT_BYTES:arena.head + k * SLOT_BYTES + n * es].view(self.dtype)
        self.all = torch.as_strided(flat, (B, self.width + F.GUARD), (self.ld, 1))
        arena.touch(self.all)
        self.m = self.all[:, :self.width]
        self.m.copy_(values)
        self.ptr = C.c_void_p(flat.data_ptr())
        assert flat.data_ptr() % 16 == 0

    def values(self):
        return self.m.clone()

    def guards_ok(self):
        return _is_fill(self.all[:, self.width:])


class NearMatrix:
    """the same values at a tight leading dimension of the same alignment class, in a fresh allocation of fill"""

    def __init__(self, kind, values, far_ld):
        self.kind, self.dtype, es = kind, DT[kind], ES[kind]
        self.width = int(values.shape[1])
        align = {4: 4, 2: 8, 1: 1}[es]
        self.ld = (self.width + align - 1) // align * align + 2 * align
        if es == 1:
            self.ld = self.width + 1 + (self.width + 1 + far_ld) % 2                 # the parity of the far spacing
        assert self.ld % align == 0 and self.ld > self.width
        self.all = _filled((B + 1, self.ld), self.dtype)
        self.m = self.all[:B, :self.width]
        self.m.copy_(values)
        self.ptr = C.c_void_p(self.all.data_ptr())

    def values(self):
        return self.m.clone()

    def guards_ok(self):
        return _is_fill(self.all[:B, self.width:]) and _is_fill(self.all[B:])


def _ld_pair(arenas, mats):
    """mats: [(name, kind, values [B][width])] -> (far {name: FarMatrix}, near {name: NearMatrix}); the big arena is wiped first"""
    arenas.big.wipe()
    far = {name: FarMatrix(arenas.big, kind, v, k) for k, (name, kind, v) in enumerate(mats)}
    near = {name: NearMatrix(kind, v, far[name].ld) for name, kind, v in mats}
    for name in far:
        last = (B - 1) * far[name].ld
        assert last > F.top_boundary(ES[far[name].kind]) and _same(far[name].values(), near[name].values())
    return far, near


def _ld_check(far, near, extra_far=(), extra_near=()):
    for name in far:
        assert _same(far[name].values(), near[name].values()), name
        assert far[name].guards_ok() and near[name].guards_ok(), name
    for a, b in zip(extra_far, extra_near):
        assert _same(a, b)


def _work_values(rng, bf16, width, special=True):
    a = rng.standard_normal((B, width)).astype(np.float32)
    if special:
        a[rng.random((B, width)) < 0.15] = 0.0
        a[0, 0] = -0.0
    t = torch.tensor(a, device=DEV)
    return t.to(torch.bfloat16) if bf16 else t


def _kind(bf16):
    return "bf16" if bf16 else "f32"


@pytest.mark.parametrize("bf16,width", LD_SHAPES, ids=LD_IDS)
def test_dropout_forward_and_backward_at_a_far_leading_dimension(hip, arenas, bf16, width):
    lib = hip.lib()
    rng = np.random.default_rng(width + int(bf16))
    rows_t = _i32(rng.permutation(500)[:B])
    layer, step, p, seed = 1, 5, 0.25, SEED
    far, near = _ld_pair(arenas, [("a", _kind(bf16), _work_values(rng, bf16, width)), ("d", _kind(bf16), _work_values(rng, bf16, width))])
    cs = []
    for m in (far, near):
        hip.check(lib.codae_dropout_fwd(m["a"].ptr, int(bf16), m["a"].ld, B, width, hip.ptr(rows_t), layer, step, p, seed, hip.current_stream()))
        colsum = _filled((lib.codae_dropout_blocks(B) + 1, width), torch.float32)
        hip.check(lib.codae_dropout_bwd(m["d"].ptr, int(bf16), m["d"].ld, B, width, hip.ptr(rows_t), layer, step, p, seed, hip.ptr(colsum),
                                        hip.current_stream()))
        torch.cuda.synchronize()
        assert _is_fill(colsum[-1])
        cs.append(colsum)
    _ld_check(far, near, cs[:1], cs[1:])
    a = far["a"].values().float()
    assert not torch.isnan(a).any() and 0.1 < float((a == 0).float().mean()) < 0.5 and not torch.isnan(cs[0][:-1]).any()


@pytest.mark.parametrize("bf16,width", LD_SHAPES, ids=LD_IDS)
def test_residual_forward_and_backward_at_far_leading_dimensions(hip, arenas, bf16, width):
    """y, x and the mask bytes of the forward; d, G in, G out and the mask bytes of the backward: every one of them far"""
    lib = hip.lib()
    rng = np.random.default_rng(2 * width + int(bf16))
    k = _kind(bf16)
    nb = (width + 7) // 8
    far, near = _ld_pair(arenas, [("y", k, _work_values(rng, bf16, width)), ("x", k, _work_values(rng, bf16, width)),
                                  ("bits", "u8", torch.full((B, nb), 0xAA, dtype=torch.uint8, device=DEV)),
                                  ("d", k, _work_values(rng, bf16, width, special=False)),
                                  ("g_in", "f32", _work_values(rng, False, width, special=False)),
                                  ("g_out", "f32", torch.full((B, width), 7.0, device=DEV))])
    cs = []
    slope = (C.c_float * 3)(0.0, 0.0, 0.0)
    for m in (far, near):
        hip.check(lib.codae_residual_fwd(m["y"].ptr, m["x"].ptr, int(bf16), m["y"].ld, m["x"].ld, B, width, m["bits"].ptr, m["bits"].ld,
                                         hip.current_stream()))
        colsum = _filled((lib.codae_residual_blocks(B) + 1, width), torch.float32)
        hip.check(lib.codae_residual_bwd(m["d"].ptr, int(bf16), m["d"].ld, B, width, m["g_in"].ptr, m["g_out"].ptr, m["g_in"].ld, m["bits"].ptr,
                                         m["bits"].ld, None, 0, 1, slope, hip.ptr(colsum), hip.current_stream()))
        torch.cuda.synchronize()
        assert _is_fill(colsum[-1])
        cs.append(colsum)
    assert far["g_in"].ld == far["g_out"].ld and near["g_in"].ld == near["g_out"].ld
    _ld_check(far, near, cs[:1], cs[1:])
    assert not torch.isnan(far["y"].values().float()).any() and not torch.isnan(far["g_out"].values()).any()
    assert bool((far["bits"].values() != 0xAA).any()) and bool((far["g_out"].values() != 7.0).all())


@pytest.mark.parametrize("kind", ["layer", "rms"])
@pytest.mark.parametrize("bf16,width", LD_SHAPES, ids=LD_IDS)
def test_norm_forward_and_backward_at_far_leading_dimensions(hip, arenas, bf16, width, kind):
    lib = hip.lib()
    rng = np.random.default_rng(3 * width + int(bf16))
    k = _kind(bf16)
    nb = (width + 7) // 8
    far, near = _ld_pair(arenas, [("y", k, _work_values(rng, bf16, width)),
                                  ("bits", "u8", torch.full((B, nb), 0xAA, dtype=torch.uint8, device=DEV)),
                                  ("d", k, _work_values(rng, bf16, width, special=False)),
                                  ("g_in", "f32", _work_values(rng, False, width, special=False)),
                                  ("g_out", "f32", torch.full((B, width), 7.0, device=DEV))])
    kid = {"layer": 1, "rms": 2}[kind]
    slope = (C.c_float * 3)(0.0, 0.0, 0.0)
    extra = []
    for m in (far, near):
        rstd = _filled((B + 1,), torch.float32)
        hip.check(lib.codae_norm_fwd(m["y"].ptr, int(bf16), m["y"].ld, B, width, kid, 1e-5, hip.ptr(rstd), m["bits"].ptr, m["bits"].ld,
                                     hip.current_stream()))
        colsum = _filled((lib.codae_norm_blocks(B) + 1, width), torch.float32)
        # the backward on what the forward left: xhat = y (far as well), its r and its mask
        hip.check(lib.codae_norm_bwd(m["d"].ptr, int(bf16), m["d"].ld, B, width, kid, m["y"].ptr, m["y"].ld, hip.ptr(rstd), m["g_in"].ptr,
                                     m["g_out"].ptr, m["g_in"].ld, m["bits"].ptr, m["bits"].ld, 1, slope, hip.ptr(colsum), hip.current_stream()))
        torch.cuda.synchronize()
        assert _is_fill(colsum[-1]) and _is_fill(rstd[B:])
        extra.append((rstd, colsum))
    _ld_check(far, near, extra[0], extra[1])
    assert not torch.isnan(far["y"].values().float()).any() and not torch.isnan(extra[0][0][:B]).any()
    assert not torch.isnan(far["d"].values().float()).any() and bool((far["g_out"].values() != 7.0).all())


@pytest.mark.parametrize("keep_id", ["1", "5", "w-1"])
@pytest.mark.parametrize("bf16,width", LD_SHAPES, ids=LD_IDS)
def test_sparse_code_forward_and_backward_at_far_leading_dimensions(hip, arenas, bf16, width, keep_id):
    lib = hip.lib()
    keep = {"1": 1, "5": 5, "w-1": width - 1}[keep_id]
    rng = np.random.default_rng(5 * width + int(bf16) + keep)
    k = _kind(bf16)
    nb = (width + 7) // 8
    far, near = _ld_pair(arenas, [("y", k, _work_values(rng, bf16, width)),
                                  ("bits", "u8", torch.full((B, nb), 0xAA, dtype=torch.uint8, device=DEV)),
                                  ("d", k, _work_values(rng, bf16, width, special=False))])
    cs = []
    for m in (far, near):
        hip.check(lib.codae_sparse_code_fwd(m["y"].ptr, int(bf16), m["y"].ld, B, width, keep, m["bits"].ptr, m["bits"].ld, hip.current_stream()))
        colsum = _filled((lib.codae_sparse_code_blocks(B) + 1, width), torch.float32)
        hip.check(lib.codae_sparse_code_bwd(m["d"].ptr, int(bf16), m["d"].ld, B, width, m["bits"].ptr, m["bits"].ld, hip.ptr(colsum),
                                            hip.current_stream()))
        torch.cuda.synchronize()
        assert _is_fill(colsum[-1])
        cs.append(colsum)
    _ld_check(far, near, cs[:1], cs[1:])
    y = far["y"].values().float()
    assert not torch.isnan(y).any() and int((y != 0).sum(dim=1).max()) <= keep and int((y != 0).sum(dim=1)[B - 1]) >= min(keep, 1)
    assert int((far["d"].values().float() != 0).sum(dim=1).max()) <= keep


@pytest.mark.parametrize("bf16,width", LD_SHAPES, ids=LD_IDS)
def test_export_rows_with_both_leading_dimensions_far(hip, arenas, bf16, width):
    lib = hip.lib()
    rng = np.random.default_rng(7 * width + int(bf16))
    far, near = _ld_pair(arenas, [("src", _kind(bf16), _work_values(rng, bf16, width)), ("dst", "f32", torch.full((B, width), 7.0, device=DEV))])
    norms = []
    for m in (far, near):
        norm = _filled((B + 1,), torch.float32)
        hip.check(lib.codae_export_rows(m["src"].ptr, int(bf16), m["src"].ld, B, width, m["dst"].ptr, m["dst"].ld, hip.ptr(norm), hip.current_stream()))
        torch.cuda.synchronize()
        assert _is_fill(norm[B:])
        norms.append(norm)
    _ld_check(far, near, norms[:1], norms[1:])
    assert _same(far["dst"].values(), far["src"].values().float()) and not torch.isnan(norms[0][:B]).any()


@pytest.mark.parametrize("op_bf16", [False, True], ids=["f32-op", "bf16-op"])
@pytest.mark.parametrize("Z", [8, 19, 40])
def test_nearest_centroid_with_a_far_bank_stride(hip, arenas, Z, op_bf16):
    """the widths of tests/test_gpu_clusters.py (16-byte rows and the element path), K = 129: two centroid groups"""
    lib = hip.lib()
    K = 129
    rng = np.random.default_rng(Z + 11 * int(op_bf16))
    c = torch.tensor(rng.standard_normal((K, Z)).astype(np.float32), device=DEV)
    far, near = _ld_pair(arenas, [("x", "f32", _work_values(rng, False, Z))])
    res = []
    for m in (far, near):
        assign = torch.full((B + 1,), -7, dtype=torch.long, device=DEV)
        best = _filled((B + 1,), torch.float32)
        ws = torch.empty(int(lib.codae_nearest_centroid_ws_bytes(Z, K, int(op_bf16))), dtype=torch.uint8, device=DEV)
        hip.check(lib.codae_nearest_centroid(m["x"].ptr, m["x"].ld, B, Z, hip.ptr(c), c.stride(0), K, int(op_bf16), None, hip.ptr(assign),
                                             hip.ptr(best), hip.ptr(ws), hip.current_stream()))
        torch.cuda.synchronize()
        assert int(assign[B]) == -7 and _is_fill(best[B:])
        res.append((assign, best))
    _ld_check(far, near, res[0], res[1])
    assert bool((res[0][0][:B] >= 0).all()) and len(set(res[0][0][:B].tolist())) > 10 and not torch.isnan(res[0][1][:B]).any()


@pytest.mark.parametrize("n", [37, 300])
def test_topk_merge_with_a_far_score_stride(hip, arenas, n):
    lib = hip.lib()
    k = 5
    rng = np.random.default_rng(n)
    s = rng.standard_normal((B, n)).astype(np.float32)
    s[:, 3] = s[:, 9]                                                             # ties: the lower position wins
    far, near = _ld_pair(arenas, [("s", "f32", torch.tensor(s, device=DEV))])
    res = []
    for m in (far, near):
        state = torch.empty(B * k, dtype=torch.int64, device=DEV)
        oi = torch.full((B + 1, k), -7, dtype=torch.int32, device=DEV)
        os_ = _filled((B + 1, k), torch.float32)
        st = hip.current_stream()
        hip.check(lib.codae_topk_init(hip.ptr(state), B, k, st))
        half = n // 2
        hip.check(lib.codae_topk_merge(m["s"].ptr, m["s"].ld, B, half, 0, k, None, None, hip.ptr(state), st))
        second = C.c_void_p(m["s"].ptr.value + 4 * half)                         # columns half .. n - 1: a view of the same far matrix
        hip.check(lib.codae_topk_merge(second, m["s"].ld, B, n - half, half, k, None, None, hip.ptr(state), st))
        hip.check(lib.codae_topk_finish(hip.ptr(state), B, k, None, hip.ptr(oi), hip.ptr(os_), st))
        torch.cuda.synchronize()
        assert bool((oi[B] == -7).all()) and _is_fill(os_[B:])
        res.append((oi, os_))
    _ld_check(far, near, res[0], res[1])
    want = np.argsort(-s, axis=1, kind="stable")[:, :k]
    assert np.array_equal(res[0][0][:B].cpu().numpy(), want)


# ---- the step ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_two_train_steps_from_far_rows(hip, arenas, precision):
    """codae_train_step through DaeEngine, make_batch on the arena view, masks through a mask_to_use table keyed by the far row;
    bf16: 6 layers at 1536 with the dataset image registered (the image gather and the fused-loss epilogue's target fetch at far
    rows), the image in the second arena.  Against an identical engine on the compact table, mask_to_use compacted alike: the
    scalars after each step, every gradient of each step and every parameter and moment after the second, bit for bit."""
    from codae.hip.engine import DaeEngine
    lib = hip.lib()
    io, S, nb_run = 1536, F.SLOTS[1536], 2
    d = _dataset(arenas, io)
    sched = [(io, io, True)] * 5 + [(io, io, False)] if precision == "bf16" else [(io, 64, True), (64, io, False)]
    rng = np.random.default_rng(77)
    params = [((rng.standard_normal((o, i)) * (1.0 / i) ** 0.5).astype(np.float32), (0.05 * rng.standard_normal(o)).astype(np.float32)) for i, o, _ in sched]
    table, _ = _masks(io, S)
    ids = rng.integers(0, S, (len(d.rows), nb_run)).astype(np.int32)
    mtu_far = torch.zeros((d.n, nb_run), dtype=torch.int32, device=DEV)
    mtu_far[torch.tensor(np.asarray(d.rows), device=DEV)] = torch.tensor(ids, device=DEV)
    mtu_near = torch.tensor(ids, device=DEV)
    batches = [d.batch(seed=9), d.batch(seed=10)]
    runs = []
    for far in (True, False):
        eng = DaeEngine(sched, B, precision, DEV)
        eng.load_params(params)
        data, mtu = (d.t, mtu_far) if far else (d.near, mtu_near)
        if precision == "bf16":
            if far:
                arenas.img.wipe()
                image = arenas.img.flat(torch.bfloat16, d.n * io + F.GUARD)
                arenas.img.dirty.append((arenas.img.head, d.n * io * 2))
                hip.check(lib.codae_cast_f32_to_bf16(hip.ptr(d.t), hip.ptr(image), d.n * io, hip.current_stream()))
                hip.check(lib.codae_set_dataset_image(eng._h, hip.ptr(d.t), hip.ptr(image), d.n, io))
                eng._dataset_image = (d.t, image)
            else:
                assert eng.set_dataset_image(d.near) is not None
        seen = []
        for step, (far_idx, near_idx, rows) in enumerate(batches):
            batch = eng.make_batch(data, far_idx if far else near_idx, None, table, mask_to_use=mtu, run=step % nb_run)
            eng.train_step(batch, eng.hyper(1e-3, 1e-4, clip=1.0, global_rows=B))
            eng.join()
            torch.cuda.synchronize()
            seen.append((eng.scalars.clone(), eng.grads.clone()))
        seen.append((eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone()))
        if precision == "bf16":
            seen.append((eng.shadow.clone(), eng.shadow_t.clone()))
            if far:
                assert _is_fill(image[d.n * io:])
        runs.append(seen)
        del eng
    for a, b in zip(*runs):
        for x, y in zip(a, b):
            assert _same(x, y)
    for scalars, grads in runs[0][:2]:
        assert bool(torch.isfinite(scalars).all()) and bool(torch.isfinite(grads).all()) and float(grads.abs().max()) > 0
    assert float(runs[0][1][0].abs().max()) > 0 and not _same(runs[0][0][1], runs[0][1][1])
    assert d.guard_ok()
    if precision == "bf16":
        # the far engine really read the image in the arena: with the image's probe rows halved its first step gives another loss
        eng = DaeEngine(sched, B, precision, DEV)
        eng.load_params(params)
        hip.check(lib.codae_set_dataset_image(eng._h, hip.ptr(d.t), hip.ptr(image), d.n, io))
        eng._dataset_image = (d.t, image)
        img = image[:d.n * io].view(d.n, io)
        for r in d.rows:
            img[r].mul_(0.5)
        far_idx, _, _ = batches[0]
        eng.train_step(eng.make_batch(d.t, far_idx, None, table, mask_to_use=mtu_far, run=0), eng.hyper(1e-3, 1e-4, clip=1.0, global_rows=B))
        eng.join()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(eng.scalars).all()) and not _same(eng.scalars, runs[0][0][0])
        del eng
    arenas.img.wipe()


# ---- inventory readers ------------------------------------------------------------------------------------------------------------------

class FarInventory:
    """[S][n_obs][E] fp32 in the big arena: as S * n_obs rows of E it has the dataset table's size, and the probe rows of that flat
    table are (c, r) pairs.  Written: rows r of EVERY slot for r in `rows` - the probe pairs' r and `extra` rows below each -, so a
    reader of any slot finds data there.  near: [S][V][E], those rows read back; V is a multiple of 4."""

    def __init__(self, arena, io, extra=40):
        self.S, self.E, self.io = F.SLOTS[io], io // F.SLOTS[io], io
        S, E = self.S, self.E
        self.n_obs = F.n_obs(io, 4)
        self.arena = arena
        self.flat = arena.flat(torch.float32, S * self.n_obs * E + F.GUARD)
        self.t = self.flat[:S * self.n_obs * E].view(S, self.n_obs, E)
        self.pairs = [divmod(f, self.n_obs) for f in F.distinct_rows(E, 4, S * self.n_obs)]       # (c, r): the flat probe rows
        assert any(c == S - 1 for c, _ in self.pairs)
        rows = set()
        for _, r in self.pairs:
            rows.update(range(max(0, r - extra), r + 1))
        k = 1
        while len(rows) % 4:
            rows.add(max(r for _, r in self.pairs) - extra - k)
            k += 1
        self.rows = sorted(rows)
        self.V = len(self.rows)
        self.pos = {r: i for i, r in enumerate(self.rows)}
        rng = np.random.default_rng(300 + io)
        vals = torch.tensor(rng.standard_normal((S, self.V, E)).astype(np.float32), device=DEV)
        near = []
        for c in range(S):
            i = 0
            while i < self.V:
                j = i
                while j + 1 < self.V and self.rows[j + 1] == self.rows[j] + 1:
                    j += 1
                dst = self.t[c, self.rows[i]:self.rows[j] + 1]
                arena.touch(dst)
                dst.copy_(vals[c, i:j + 1])
                i = j + 1
            near.append(torch.stack([self.t[c, r] for r in self.rows]))
        self.near = torch.stack(near).clone()
        assert _same(self.near, vals)
        self._norms = None

    def norms(self, hip):
        """(far [S][n_obs] over the whole arena view, near [S][V]) by codae_row_norms"""
        if self._norms is None:
            far = _filled((self.S * self.n_obs + F.GUARD,), torch.float32)
            near = _filled((self.S * self.V + F.GUARD,), torch.float32)
            hip.check(hip.lib().codae_row_norms(hip.ptr(self.t), self.S * self.n_obs, self.E, hip.ptr(far), hip.current_stream()))
            hip.check(hip.lib().codae_row_norms(hip.ptr(self.near), self.S * self.V, self.E, hip.ptr(near), hip.current_stream()))
            torch.cuda.synchronize()
            self._norms = (far, near)
        return self._norms

    def batch(self, seed):
        """70 queries on the probe pairs: (far rows int32, near rows int32, the blanked slot of each = the pair's slot)"""
        rng = np.random.default_rng(seed)
        order = np.concatenate([np.arange(len(self.pairs)), rng.integers(0, len(self.pairs), B - len(self.pairs))])
        rng.shuffle(order)
        c = np.asarray([self.pairs[i][0] for i in order])
        r = np.asarray([self.pairs[i][1] for i in order])
        return _i32(r), _i32([self.pos[int(v)] for v in r]), _i32(c), r, c

    def pred(self, r, c, seed):
        """a prediction whose blanked slot is the row's own item plus noise, scaled so that the own item's cosine sits near the best
        of the V - 1 competitors' (0.86 in 8 dimensions, 0.13 in 512): about half the queries rank their own item first"""
        rng = np.random.default_rng(seed)
        scale = {8: 0.6, 512: 7.75}[self.E]
        p = rng.standard_normal((B, self.io)).astype(np.float32)
        own = self.near.cpu().numpy()
        for b in range(B):
            p[b, c[b] * self.E:(c[b] + 1) * self.E] = own[c[b], self.pos[int(r[b])]] + scale * p[b, c[b] * self.E:(c[b] + 1) * self.E]
        return torch.tensor(p, device=DEV)

    def row_table(self, width, fill, values):
        """an int32 [width-major] table keyed by the dataset row: `fill` everywhere, values [.., V] at self.rows"""
        t = torch.full(tuple(values.shape[:-1]) + (self.n_obs,), fill, dtype=torch.int32, device=DEV)
        t[..., torch.tensor(np.asarray(self.rows), device=DEV)] = values
        return t


def _inventory(arenas, io):
    arenas.release_image()
    return arenas.big.claim(("inventory", io), lambda: FarInventory(arenas.big, io))


@pytest.mark.parametrize("io", F.WIDTHS)
def test_row_norms_over_the_whole_far_inventory(hip, arenas, io):
    v = _inventory(arenas, io)
    far, near = v.norms(hip)
    assert _is_fill(far[v.S * v.n_obs:]) and _is_fill(near[v.S * v.V:])
    far2, near2 = far[:v.S * v.n_obs].view(v.S, v.n_obs), near[:v.S * v.V].view(v.S, v.V)
    got = far2[:, torch.tensor(np.asarray(v.rows), device=DEV)]
    assert _same(got, near2) and not torch.isnan(got).any() and bool((got > 0).all())
    for c, r in v.pairs:
        assert _same(far2[c, r], near2[c, v.pos[r]])
    assert torch.isnan(far2[:, 0]).all() and torch.isnan(far2[v.S - 1, v.rows[0] - 1]) and int(torch.isfinite(far2).sum()) == v.S * v.V


@pytest.mark.parametrize("io", F.WIDTHS)
def test_gather_inventory_rows_from_far_rows(hip, arenas, io):
    v = _inventory(arenas, io)
    lib = hip.lib()
    outs = []
    for inv, n_obs, idx in ((v.t, v.n_obs, _i32(v.rows)), (v.near, v.V, _i32(range(v.V)))):
        dst = _filled((v.S * v.V * v.E + F.GUARD,), torch.float32)
        hip.check(lib.codae_gather_inventory_rows(hip.ptr(inv), n_obs, v.E, v.S, hip.ptr(idx), v.V, hip.ptr(dst), hip.current_stream()))
        torch.cuda.synchronize()
        assert _is_fill(dst[v.S * v.V * v.E:])
        outs.append(dst)
    assert _same(outs[0], outs[1]) and _same(outs[0][:v.S * v.V * v.E].view(v.S, v.V, v.E), v.near)


@pytest.mark.parametrize("io", F.WIDTHS)
def test_ranking_loss_per_item_reads_far_inventory_rows(hip, arenas, io):
    v = _inventory(arenas, io)
    lib = hip.lib()
    far_norm, near_norm = v.norms(hip)
    far_idx, near_idx, slot, r, c = v.batch(1)
    pred = v.pred(r, c, 2)
    table, _ = _masks(io, v.S)
    fmask = table[slot.long()].float().contiguous()
    outs = []
    for inv, norm, n_obs, idx, val in ((v.t, far_norm, v.n_obs, far_idx, _i32(v.rows)), (v.near, near_norm, v.V, near_idx, _i32(range(v.V)))):
        out = torch.zeros(2, dtype=torch.float64, device=DEV)
        hip.check(lib.codae_ranking_loss(hip.ptr(pred), hip.ptr(fmask), hip.ptr(idx), B, io, v.S, v.E, hip.ptr(inv), hip.ptr(norm), n_obs,
                                         hip.ptr(val), v.V, hip.ptr(out), hip.current_stream()))
        torch.cuda.synchronize()
        outs.append(out)
    assert _same(outs[0], outs[1]) and float(outs[0][1]) == 0.0
    assert 0 < float(outs[0][0]) < B, float(outs[0][0])                            # some query ranks first, some does not


def _val_tables(hip, v):
    """the validation inventory of the batched readers: every written row, gathered from the compact table, and its norms"""
    lib = hip.lib()
    idx = _i32(range(v.V))
    inv_val = torch.empty((v.S, v.V, v.E), dtype=torch.float32, device=DEV)
    norm = torch.empty((v.S, v.V), dtype=torch.float32, device=DEV)
    hip.check(lib.codae_gather_inventory_rows(hip.ptr(v.near), v.V, v.E, v.S, hip.ptr(idx), v.V, hip.ptr(inv_val), hip.current_stream()))
    hip.check(lib.codae_row_norms(hip.ptr(inv_val), v.S * v.V, v.E, hip.ptr(norm), hip.current_stream()))
    torch.cuda.synchronize()
    return inv_val, norm


@pytest.mark.parametrize("io", F.WIDTHS)
def test_ranking_loss_batched_reads_far_inventory_rows(hip, arenas, io):
    v = _inventory(arenas, io)
    lib = hip.lib()
    far_norm, near_norm = v.norms(hip)
    far_idx, near_idx, slot, r, c = v.batch(3)
    pred = v.pred(r, c, 4)
    table, _ = _masks(io, v.S)
    inv_val, inv_val_norm = _val_tables(hip, v)
    arange = torch.arange(v.V, dtype=torch.int32, device=DEV)
    pos_far, pos_near = v.row_table(1, -1, arange), arange.clone()
    chunk = 128
    outs = []
    for inv, norm, n_obs, idx, pos in ((v.t, far_norm, v.n_obs, far_idx, pos_far), (v.near, near_norm, v.V, near_idx, pos_near)):
        work = torch.empty(B * chunk, dtype=torch.float32, device=DEV)
        state = torch.empty(8 * B, dtype=torch.int32, device=DEV)
        perm = torch.empty(v.S * B + v.S, dtype=torch.int32, device=DEV)
        q = torch.empty(B * v.E, dtype=torch.float32, device=DEV)
        out = torch.zeros(2, dtype=torch.float64, device=DEV)
        hip.check(lib.codae_ranking_loss_batched(hip.ptr(pred), B, io, v.S, v.E, hip.ptr(idx), hip.ptr(slot), None, 0, 0, hip.ptr(table),
                                                 hip.ptr(inv), hip.ptr(norm), n_obs, hip.ptr(inv_val), hip.ptr(inv_val_norm), hip.ptr(pos), None,
                                                 v.V, hip.ptr(work), chunk, hip.ptr(state), hip.ptr(perm), hip.ptr(q), hip.ptr(out),
                                                 hip.current_stream()))
        torch.cuda.synchronize()
        outs.append(out)
    assert _same(outs[0], outs[1]) and float(outs[0][1]) == 0.0
    assert 0 < float(outs[0][0]) < B, float(outs[0][0])                            # some query ranks first, some does not


@pytest.mark.parametrize("io", F.WIDTHS)
def test_complete_topk_excludes_through_a_table_keyed_by_the_far_row(hip, arenas, io):
    """the candidates are the written rows (compact, as the retriever builds them); what is keyed by the far row is cand_pos
    [S][n_obs], through which `exclude` finds the candidate a query must not get, and cand_row_id, which names the answers"""
    v = _inventory(arenas, io)
    lib = hip.lib()
    k, chunk = 7, 128
    far_idx, near_idx, slot, r, c = v.batch(5)
    pred = v.pred(r, c, 6)
    cand, cand_norm = _val_tables(hip, v)
    arange = torch.arange(v.V, dtype=torch.int32, device=DEV).expand(v.S, v.V).contiguous()
    rows_t = _i32(v.rows).expand(v.S, v.V).contiguous()
    res = []
    for row_id, pos, n_obs, ex in ((rows_t, v.row_table(v.S, -1, arange), v.n_obs, far_idx), (arange, arange.clone(), v.V, near_idx)):
        work = torch.empty(B * chunk, dtype=torch.float32, device=DEV)
        state = torch.empty(3 * B, dtype=torch.int32, device=DEV)
        perm = torch.empty(v.S * B + v.S, dtype=torch.int32, device=DEV)
        q = torch.empty(B * v.E, dtype=torch.float32, device=DEV)
        topk = torch.empty(B * k, dtype=torch.int64, device=DEV)
        oi = torch.full((B + 1, k), -7, dtype=torch.int32, device=DEV)
        os_ = _filled((B + 1, k), torch.float32)
        hip.check(lib.codae_complete_topk(hip.ptr(pred), B, io, v.S, v.E, hip.ptr(slot), None, None, None, 0, 0, None, hip.ptr(cand),
                                          hip.ptr(cand_norm), hip.ptr(row_id), v.V, None, hip.ptr(ex), hip.ptr(pos), n_obs, k, hip.ptr(work), chunk,
                                          hip.ptr(state), hip.ptr(perm), hip.ptr(q), hip.ptr(topk), hip.ptr(oi), hip.ptr(os_), hip.current_stream()))
        torch.cuda.synchronize()
        assert bool((oi[B] == -7).all()) and _is_fill(os_[B:])
        res.append((oi[:B].cpu().numpy(), os_[:B]))
    assert _same(res[0][1], res[1][1]) and not torch.isnan(res[0][1]).any()
    assert (res[1][0] >= 0).all() and np.array_equal(res[0][0], np.asarray(v.rows)[res[1][0]])               # ids through the remap
    assert not (res[0][0] == r[:, None]).any()                                                               # the excluded row never comes back


@pytest.mark.parametrize("io", F.WIDTHS)
def test_retrieval_metrics_batched_read_far_inventory_rows(hip, arenas, io):
    v = _inventory(arenas, io)
    lib = hip.lib()
    far_norm, near_norm = v.norms(hip)
    far_idx, near_idx, slot, r, c = v.batch(7)
    pred = v.pred(r, c, 8)
    table, _ = _masks(io, v.S)
    cand, cand_norm = _val_tables(hip, v)
    arange = torch.arange(v.V, dtype=torch.int32, device=DEV).expand(v.S, v.V).contiguous()
    pres_far, sub = _presence(v.n_obs, v.S, v.rows, seed=9)
    for (cc, rr) in v.pairs:                                                       # the probe pairs stay present: they are the queries
        sub[v.pos[rr], cc] = 1
    pres_far[torch.tensor(np.asarray(v.rows), device=DEV)] = torch.tensor(sub, device=DEV)
    pres_near = torch.tensor(sub, device=DEV)
    count = (C.c_int32 * v.S)(*([v.V] * v.S))
    ks = (C.c_int32 * 3)(1, 5, 20)
    chunk = 128
    accs = []
    for inv, norm, n_obs, idx, pos, pres in ((v.t, far_norm, v.n_obs, far_idx, v.row_table(v.S, -1, arange), pres_far),
                                             (v.near, near_norm, v.V, near_idx, arange.clone(), pres_near)):
        work = torch.empty(B * chunk, dtype=torch.float32, device=DEV)
        state = torch.empty(4 * v.S * B, dtype=torch.int32, device=DEV)
        perm = torch.empty(v.S * B + v.S, dtype=torch.int32, device=DEV)
        q = torch.empty(B * v.E, dtype=torch.float32, device=DEV)
        acc = torch.zeros((v.S + 1, 48), dtype=torch.float64, device=DEV)
        hip.check(lib.codae_retrieval_metrics_batched(hip.ptr(pred), B, io, v.S, v.E, hip.ptr(idx), hip.ptr(slot), None, 0, 0, hip.ptr(table),
                                                      hip.ptr(pres), hip.ptr(inv), hip.ptr(norm), n_obs, hip.ptr(cand), hip.ptr(cand_norm), v.V, count,
                                                      hip.ptr(pos), ks, 3, hip.ptr(work), chunk, hip.ptr(state), hip.ptr(perm), hip.ptr(q),
                                                      hip.ptr(acc), hip.current_stream()))
        torch.cuda.synchronize()
        assert bool((acc[v.S] == 0).all())
        accs.append(acc)
    assert _same(accs[0], accs[1])
    a = accs[0].cpu().numpy()
    assert a[:v.S, 0].sum() == B and not np.isnan(a).any()                          # every query is a pair; counts and sums are finite
    assert 0 < a[:v.S, 3].sum() < B                                                 # hit@1: some, not all
