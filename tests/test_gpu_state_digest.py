"""codae_state_digest on the device against its numpy restatement (tests/snapshot_ref.py): every size at which the kernel takes another
path (empty, a partial group alone, whole groups, one workgroup and many), the 16-byte and the dword path, the copy made in the same
pass, and the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from snapshot_ref import VECTORS, digest_numpy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 0x5A5A5A5A
# 0 / 1 / 3: no whole group; 4 / 5: one; 255 .. 257: around a wave's worth of groups; 1023 .. 4100: one workgroup's unrolled loop, its
# remainder loop and the step to several workgroups; the last: 49 workgroups with a 3-word tail
WORDS = [0, 1, 3, 4, 5, 255, 256, 257, 1023, 4096, 4100, 64 * 1024 * 3 + 3]
# the grid is capped at 2048 workgroups of 256 lanes, each lane taking 4 groups per turn of its loop: twice that and a little more
# makes every lane go round more than once and leaves work for the remainder loop and the tail (67 MB)
CAPPED = 2048 * 256 * 4 * 4 * 2 + 4 * 1000 + 3


def _call(src_ptr, dst_ptr, n_bytes, out):
    from codae.hip import current_stream, lib
    with torch.cuda.device(DEV):
        return lib().codae_state_digest(src_ptr, dst_ptr, n_bytes, C.c_void_p(out.data_ptr()) if out is not None else None, current_stream())


def _digest(t, dst=None):
    out = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    n = t.numel() * t.element_size()
    rc = _call(C.c_void_p(t.data_ptr()) if n else None, None if dst is None or not n else C.c_void_p(dst.data_ptr()), n, out)
    assert rc == 0
    a, b = out.cpu().tolist()
    return a & (2 ** 64 - 1), b & (2 ** 64 - 1)


def _words(n, seed=0):
    return np.random.default_rng(seed + n).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("n", WORDS)
def test_matches_numpy_at_every_path_boundary(n):
    w = _words(n)
    t = torch.from_numpy(w.view(np.int32).copy()).to(DEV)
    want = digest_numpy(w)
    assert _digest(t) == want
    assert _digest(t) == want                                  # two calls, the same bits


def test_published_vectors_on_the_device():
    for name, array, out0, out1 in VECTORS:
        t = torch.from_numpy(array.view(np.int32).copy()).to(DEV)
        assert _digest(t) == (out0, out1), name


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
def test_tensor_types_are_read_as_bytes(dtype):
    g = torch.Generator().manual_seed(3)
    t = torch.randn(3002, generator=g).to(dtype)
    t[5] = -0.0
    t[6] = float("nan")
    want = digest_numpy(t.view(torch.uint8).numpy())
    assert _digest(t.to(DEV)) == want
    flipped = t.clone()
    flipped[5] = 0.0
    assert _digest(flipped.to(DEV)) != want                    # -0.0 is not +0.0


@pytest.mark.parametrize("n", [1, 5, 257, 4100, 64 * 1024 * 3 + 3])
@pytest.mark.parametrize("offset_words", [1, 2, 3])
def test_unaligned_views_take_the_dword_path(n, offset_words):
    """A base 4, 8 and 12 bytes past a 16-byte boundary: the same digest, and the bytes around the view neither count nor change."""
    w = _words(n, seed=7)
    big = torch.full((n + 16,), GUARD, dtype=torch.int32, device=DEV)
    assert big.data_ptr() % 16 == 0
    view = big[offset_words:offset_words + n]
    view.copy_(torch.from_numpy(w.view(np.int32).copy()))
    want = digest_numpy(w)
    assert _digest(view) == want
    big[:offset_words] = 0x1234567                             # other bytes around the view: the same digest
    big[offset_words + n:] = -7
    assert _digest(view) == want
    back = big.cpu().numpy()
    assert (back[:offset_words] == 0x1234567).all() and (back[offset_words + n:] == -7).all()
    assert np.array_equal(back[offset_words:offset_words + n].view(np.uint32), w)


@pytest.mark.parametrize("n", [1, 5, 257, 4100, 64 * 1024 * 3 + 3])
@pytest.mark.parametrize("src_off,dst_off", [(0, 0), (0, 1), (2, 0), (3, 3)], ids=["vec", "dst+4", "src+8", "both+12"])
def test_copy_in_the_same_pass(n, src_off, dst_off):
    w = _words(n, seed=11)
    src_big = torch.full((n + 8,), GUARD, dtype=torch.int32, device=DEV)
    dst_big = torch.full((n + 8,), GUARD, dtype=torch.int32, device=DEV)
    src, dst = src_big[src_off:src_off + n], dst_big[dst_off:dst_off + n]
    src.copy_(torch.from_numpy(w.view(np.int32).copy()))
    want = digest_numpy(w)
    assert _digest(src, dst=dst) == want == _digest(src)       # the same digest with and without the copy
    back = dst_big.cpu().numpy()
    assert np.array_equal(back[dst_off:dst_off + n].view(np.uint32), w)                  # bit for bit
    assert (back[:dst_off] == GUARD).all() and (back[dst_off + n:] == GUARD).all()      # the guard words around dst
    assert np.array_equal(src_big.cpu().numpy()[src_off:src_off + n].view(np.uint32), w)


def test_capped_grid_goes_round_more_than_once():
    w = _words(CAPPED, seed=13)
    want = digest_numpy(w)
    big = torch.zeros(CAPPED + 4, dtype=torch.int32, device=DEV)
    dst_big = torch.full((CAPPED + 8,), GUARD, dtype=torch.int32, device=DEV)
    for off in (0, 1):                                          # the 16-byte path, then the dword path
        src, dst = big[off:off + CAPPED], dst_big[off:off + CAPPED]
        src.copy_(torch.from_numpy(w.view(np.int32).copy()))
        dst_big.fill_(GUARD)
        assert _digest(src) == want and _digest(src, dst=dst) == want
        assert torch.equal(src, dst) and bool((dst_big[:off] == GUARD).all()) and bool((dst_big[off + CAPPED:] == GUARD).all())


def test_engine_digest_of_a_tensor():
    from codae.hip.engine import DaeEngine
    eng = DaeEngine([(64, 64, True), (64, 64, False)], 64, "f32", DEV)
    t = torch.arange(8, dtype=torch.float32, device=DEV)
    assert eng.digest(t) == (VECTORS[4][2], VECTORS[4][3])
    d = eng.digests()
    assert list(d) == ["params", "adam_m", "adam_v", "scalars"] and d["params"] == eng.digest("params") == digest_numpy(eng.params.cpu().numpy())
    assert d["scalars"] == digest_numpy(eng.scalars.cpu().numpy())


def test_argument_errors_are_refused_before_any_launch():
    from codae.hip import lib
    t = torch.zeros(4, dtype=torch.int32, device=DEV)
    out = torch.full((2,), 77, dtype=torch.int64, device=DEV)
    p = C.c_void_p(t.data_ptr())
    assert _call(p, None, 6, out) == -1 and b"multiple of 4" in lib().codae_last_error()
    assert _call(p, None, -4, out) == -1 and b"negative" in lib().codae_last_error()
    assert _call(p, None, 16, None) == -1 and b"out is NULL" in lib().codae_last_error()
    assert _call(None, None, 16, out) == -1 and b"src is NULL" in lib().codae_last_error()
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [77, 77]                      # nothing ran
    assert _call(None, None, 0, out) == 0                      # empty is valid, src may be NULL
    a, b = out.cpu().tolist()
    assert (a & (2 ** 64 - 1), b) == (VECTORS[0][2], 0)
