"""The training step's gather (the bf16 kernel that moves 8 elements per thread) against the generic gather kernel: out[b] =
data[row_idx[b]] * mask_table[mask id of b], the fp32 output of the generic path rounded to bf16 as the kernel rounds (round to
nearest even) - EQUAL bit for bit, no tolerance.  Widths: one 8-element item per row (8), a row shorter than one wave (72), the
headline width (1536).  Rows: 1, 5 (odd), 257 (more than one block, odd tail).  Row ids given or not; mask ids given per row,
looked up through mask_to_use (2 runs), or no mask at all; and an output row stride wider than io, whose pad columns must keep
the value they had.  (Written with a rows-per-wave rewrite of the kernel that did not measure faster and was dropped, DESIGN.md
5g; the cases pin whatever kernel serves this path.)"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
POISON = -7.0
N_ROWS = 300
_DATA = {}


def _dataset(io):
    """dataset, 4 masks that blank one span each, mask_to_use with 2 runs: built once per width"""
    if io not in _DATA:
        rng = np.random.default_rng(50 + io)
        data = rng.standard_normal((N_ROWS, io)).astype(np.float32)
        table = np.ones((4, io), dtype=np.uint8)
        w = max(1, io // 4)
        for k in range(4):
            table[k, k * w:(k + 1) * w] = 0
        mtu = rng.integers(0, 4, (N_ROWS, 2)).astype(np.int32)
        _DATA[io] = (torch.tensor(data, device=DEV), torch.tensor(table, device=DEV), torch.tensor(mtu, device=DEV), rng)
    return _DATA[io]


def _gather(data, row_idx, B, mask_id, table, mtu, run, out):
    from codae import hip
    io = int(data.shape[1])
    batch = hip.Batch(hip.ptr(data), hip.ptr(row_idx), hip.ptr(mask_id), hip.ptr(table), B, io, hip.ptr(mtu),
                      0 if mtu is None else int(mtu.shape[1]), run)
    hip.check(hip.lib().codae_corrupt_batch(C.byref(batch), None, 1, None, hip.ptr(out), int(out.dtype == torch.bfloat16),
                                            int(out.shape[1]), hip.current_stream()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("mask", ["mask_id", "mask_to_use", "unmasked"])
@pytest.mark.parametrize("with_row_idx", [True, False], ids=["row_idx", "rows-in-place"])
@pytest.mark.parametrize("B", [1, 5, 257])
@pytest.mark.parametrize("io", [8, 72, 1536])
def test_row_gather_equals_the_generic_gather(io, B, with_row_idx, mask):
    data, table, mtu, rng = _dataset(io)
    row_idx = torch.tensor(rng.permutation(N_ROWS)[:B].astype(np.int32), device=DEV) if with_row_idx else None
    mask_id = torch.tensor(rng.integers(0, 4, B).astype(np.int32), device=DEV) if mask == "mask_id" else None
    tb = None if mask == "unmasked" else table
    mt = mtu if mask == "mask_to_use" else None
    ref = _gather(data, row_idx, B, mask_id, tb, mt, 1, torch.full((B, io), POISON, device=DEV))
    assert bool((ref != POISON).all())
    if mask != "unmasked":
        assert bool((ref == 0).any()), "no element was blanked"
    want = ref.bfloat16()
    for ld in (io, io + 40):                      # contiguous rows, and a wider stride with 40 pad columns
        out = _gather(data, row_idx, B, mask_id, tb, mt, 1, torch.full((B, ld), POISON, device=DEV, dtype=torch.bfloat16))
        assert torch.equal(out[:, :io].view(torch.int16), want.view(torch.int16)), "ld %d: gathered rows differ from the generic kernel's" % ld
        assert bool((out[:, io:] == POISON).all()), "ld %d: pad columns were written" % ld
