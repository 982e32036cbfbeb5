"""The streaming kernels past the first trip of their capped grids, on a real MI355X.  The wave-per-row forwards (sparse code, norm,
export rows) launch at most 4096 blocks of 4 rows and loop beyond 16384 rows; the thread-per-chunk forwards (residual, dropout) launch
at most 2048 blocks of 256 chunks.  The kernel files of those features stop at 130 rows, 2 % of one trip; here each kernel runs one
whole trip and a ragged second one (tests/test_second_trip_shapes_host.py holds the shapes to the caps in the sources) and is checked
over the WHOLE matrix against the restatement of its own file, with that file's helpers, poison and guards:

  B_WAVE = 16454 = 4096 * 4 + 70 rows: the second trip has 17 whole blocks and one block with two live waves, which idle through the
  sparse forward's LDS histograms and barriers beside two waves that work
  B_CHUNK = 2800 rows of 1536 / 1537 / 1540 columns: 537600 (bf16, 8 columns a chunk) to 1078000 chunks against 524288 a trip

Tolerances are those of the kernel's own file: bit for bit for the sparse values and mask, the exported rows, the residual values
and mask and the dropout values; tests/test_gpu_norm.py's bounds for xhat and r and tests/test_gpu_codes.py's for the row norms;
column sums bit for bit against the sweep's restated order."""
import numpy as np
import pytest

import dropout_ref as DR
import norm_ref as NR
import residual_ref as RR
import sparse_ref as SR
from golden_util import close, max_err
from test_gpu_codes import _export, _source
from test_gpu_dropout import FILL, SEED, _same_bits, drop_bwd, drop_fwd
from test_gpu_dropout import _matrix as _drop_matrix
from test_gpu_norm import EPS, _bits32, _raw, _within, _work
from test_gpu_norm import _fwd as _norm_fwd
from test_gpu_norm import _matrix as _norm_matrix
from test_gpu_residual import _bwd as _res_bwd
from test_gpu_residual import _matrix as _res_matrix
from test_gpu_residual import _round
from test_gpu_sparse_code import POISON, _bf16_valued, _device, _host_bits, _padded, _rows
from test_gpu_sparse_code import _bwd as _sparse_bwd
from test_gpu_sparse_code import _fwd as _sparse_fwd

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
WAVE_ROWS_PER_BLOCK = 4             # rows (waves) per block of the wave-per-row forwards
B_WAVE = 4096 * WAVE_ROWS_PER_BLOCK + 70
TAIL = 70                           # the rows of the second trip
# (bf16, width, ld): the bf16 16-byte path, the fp32 element path, the fp32 16-byte path ending in half a chunk
WAVE_SHAPES = [(True, 24, 32), (False, 21, 23), (False, 20, 20)]
WAVE_IDS = ["bf16-w24", "f32-w21-elem", "f32-w20"]
B_CHUNK = 2800
CHUNK_SHAPES = [(True, 1536, 1536), (False, 1537, 1540), (False, 1540, 1540)]
CHUNK_IDS = ["bf16-w1536", "f32-w1537-elem", "f32-w1540"]
SPARSE_KEEPS = ("1", "5", "w-1")


def chunk_cols(bf16, width, ld):
    """columns per work item of the thread-per-chunk forwards, as (residual, dropout): 16 bytes of the working type where the rows
    allow 16-byte access, else the element path's 8 (residual) or 4 (dropout) columns one by one"""
    vec = (width * (2 if bf16 else 4)) % 16 == 0 and (ld * (2 if bf16 else 4)) % 16 == 0
    return 8, (8 if bf16 and vec else 4)


# ---- wave per row -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("keep_id", SPARSE_KEEPS)
@pytest.mark.parametrize("bf16,width,ld", WAVE_SHAPES, ids=WAVE_IDS)
def test_sparse_forward_and_backward_past_the_first_grid_trip(bf16, width, ld, keep_id):
    """values, +0 stores, mask bytes, pads and guards of all 16454 rows; the backward on the mask the forward wrote; and rows
    16384 .. 16453 have the bits of the same 70 rows in a 70-row call.  The sparse file's tie rows and planted rows stand in the
    first rows and again in the last 70."""
    from codae import hip
    keep = {"1": 1, "5": 5, "w-1": width - 1}[keep_id]
    B, nb = B_WAVE, (width + 7) // 8
    rng = np.random.default_rng(width * 3 + keep)
    a = _rows(rng, B, width, keep, bf16)
    a[B - TAIL:] = _rows(rng, TAIL, width, keep, bf16)
    full = _padded(a, ld)
    want_mask = SR.select(a, keep, bf16)
    want = _padded(SR.apply_bits(a, want_mask), ld)
    y = _device(full, bf16)
    bits = torch.full((B + 1, nb + 1), 0xAA, dtype=torch.uint8, device=DEV)
    assert _sparse_fwd(y, bf16, ld, B, width, keep, bits, nb + 1) == 0, hip.lib().codae_last_error()
    got = _host_bits(y)
    assert np.array_equal(got, want.view(np.uint32)), np.argwhere(got != want.view(np.uint32))[:8]               # values, +0, pads
    gb = bits.cpu().numpy()
    assert np.array_equal(gb[:B, :nb], SR.packed(want_mask)), np.flatnonzero((gb[:B, :nb] != SR.packed(want_mask)).any(axis=1))[:8]
    assert (gb[:B, nb] == 0xAA).all() and (gb[B] == 0xAA).all()
    y2 = _device(full, bf16)                                                  # the evaluation form (no mask buffer): the same values
    assert _sparse_fwd(y2, bf16, ld, B, width, keep) == 0
    assert np.array_equal(_host_bits(y2), got)
    # the backward, on the mask the forward wrote
    g = rng.standard_normal((B, width)).astype(np.float32)
    g[rng.random((B, width)) < 0.1] = -0.0
    if bf16:
        g = _bf16_valued(g)
    gfull = _padded(g, ld)
    want_d = _padded(SR.apply_bits(g, want_mask), ld)
    d = _device(gfull, bf16)
    rc, cs = _sparse_bwd(d, bf16, ld, B, width, bits, nb + 1)
    assert rc == 0, hip.lib().codae_last_error()
    got_d = _host_bits(d)
    assert np.array_equal(got_d, want_d.view(np.uint32)), np.argwhere(got_d != want_d.view(np.uint32))[:8]
    blocks = (B + 63) // 64
    csn = cs.cpu().numpy()
    assert (csn[blocks] == POISON).all()
    assert np.array_equal(csn[:blocks].view(np.uint32), RR.colsum_parts_fixed_order(want_d[:B, :width], B).view(np.uint32))
    assert np.array_equal(bits.cpu().numpy(), gb)
    # the second trip's rows in a call of their own
    y70 = _device(full[B - TAIL:], bf16)
    bits70 = torch.full((TAIL + 1, nb + 1), 0xAA, dtype=torch.uint8, device=DEV)
    assert _sparse_fwd(y70, bf16, ld, TAIL, width, keep, bits70, nb + 1) == 0
    d70 = _device(gfull[B - TAIL:], bf16)
    rc, _ = _sparse_bwd(d70, bf16, ld, TAIL, width, bits70, nb + 1)
    assert rc == 0
    assert np.array_equal(_host_bits(y70), got[B - TAIL:]) and np.array_equal(bits70.cpu().numpy()[:TAIL], gb[B - TAIL:B])
    assert np.array_equal(_host_bits(d70), got_d[B - TAIL:])


@pytest.mark.parametrize("kind", ["layer", "rms"])
@pytest.mark.parametrize("bf16,width,ld", WAVE_SHAPES, ids=WAVE_IDS)
def test_norm_forward_past_the_first_grid_trip(bf16, width, ld, kind):
    from codae import hip
    B, nb = B_WAVE, (width + 7) // 8
    rng = np.random.default_rng(width * 3 + int(bf16))
    y, a = _norm_matrix(rng, B, width, ld, bf16)
    bits = torch.full((B + 1, nb + 1), 0xAA, dtype=torch.uint8, device=DEV)
    rc, rstd = _norm_fwd(y, bf16, ld, B, width, kind, bits, nb + 1)
    assert rc == 0, hip.lib().codae_last_error()
    got = y.float().cpu().numpy()
    assert (got[:, width:] == POISON).all() and (got[B:] == POISON).all()                         # pad columns and pad rows survive
    gb = bits.cpu().numpy()
    assert np.array_equal(gb[:B, :nb], NR.packed_mask(a[:B, :width]))                             # of the value BEFORE the norm
    assert (gb[:B, nb] == 0xAA).all() and (gb[B] == 0xAA).all()
    xh, r = NR.normalise64(a[:B, :width], kind, EPS)
    gr = rstd.cpu().numpy()
    assert gr[B] == POISON
    assert close(gr[:B], r), max_err(gr[:B], r)
    ok, ratio = _within(got[:B, :width], xh, bf16)
    print("xhat worst / bound", ratio, "second trip alone", _within(got[B - TAIL:B, :width], xh[B - TAIL:], bf16)[1])
    assert ok, ratio
    assert (_bits32(got[B - 1, :width]) == 0).all()                                               # the dead row: the last of the second trip
    y2, _ = _work(a, bf16)                                                                        # without a mask buffer: the same bits
    rc, rstd2 = _norm_fwd(y2, bf16, ld, B, width, kind)
    assert rc == 0 and torch.equal(_raw(y2), _raw(y)) and torch.equal(rstd2.view(torch.int32), rstd.view(torch.int32))
    # the second trip's rows in a call of their own: the same bits
    y70, _ = _work(a[B - TAIL:], bf16)
    rc, rstd70 = _norm_fwd(y70, bf16, ld, TAIL, width, kind)
    assert rc == 0 and torch.equal(_raw(y70), _raw(y)[B - TAIL:]) and torch.equal(rstd70.view(torch.int32)[:TAIL], rstd.view(torch.int32)[B - TAIL:B])


@pytest.mark.parametrize("bf16,width,ld_src", WAVE_SHAPES, ids=WAVE_IDS)
def test_export_rows_past_the_first_grid_trip(bf16, width, ld_src):
    from codae import hip
    B = B_WAVE
    rng = np.random.default_rng(width * 7 + int(bf16))
    src, a, nan_row = _source(rng, B, width, ld_src, bf16)
    a[B - 3, width // 2] = np.nan                                             # a NaN row in the second trip as well
    src, a = _work(a, bf16)
    before = src.clone()
    with np.errstate(invalid="ignore"):
        ref = np.sqrt((a[:B, :width].astype(np.float64) ** 2).sum(axis=1))
    ok = np.isfinite(ref)
    assert (~ok).sum() == 2 and not ok[nan_row] and not ok[B - 3]
    for ld_dst in (width, width + 3):
        dst = torch.full((B + 2, ld_dst), POISON, dtype=torch.float32, device=DEV)
        norm = torch.full((B + 1,), POISON, dtype=torch.float32, device=DEV)
        assert _export(src, bf16, ld_src, B, width, dst, ld_dst, norm) == 0, hip.lib().codae_last_error()
        got, gn = dst.cpu().numpy(), norm.cpu().numpy()
        assert np.array_equal(_bits32(got[:B, :width]), _bits32(a[:B, :width])), ld_dst                         # -0.0 and the NaNs included
        assert (got[:, width:] == POISON).all() and (got[B:] == POISON).all() and gn[B] == POISON
        assert torch.equal(_raw(src), _raw(before))
        assert np.isnan(gn[:B][~ok]).all() and np.isfinite(gn[:B][ok]).all()
        assert close(gn[:B][ok], ref[ok]), (ld_dst, max_err(gn[:B][ok], ref[ok]))
        assert _bits32(gn[B - 1]) == 0                                                                           # the all-zero row: +0
        dst3 = torch.full((B + 2, ld_dst), POISON, dtype=torch.float32, device=DEV)                              # without a norm buffer
        assert _export(src, bf16, ld_src, B, width, dst3, ld_dst, None) == 0
        assert torch.equal(dst3.view(torch.int32), dst.view(torch.int32))
    # the second trip's rows in a call of their own: the same norm bits
    src70, _ = _work(a[B - TAIL:], bf16)
    dst70 = torch.full((TAIL + 2, width), POISON, dtype=torch.float32, device=DEV)
    norm70 = torch.full((TAIL + 1,), POISON, dtype=torch.float32, device=DEV)
    assert _export(src70, bf16, ld_src, TAIL, width, dst70, width, norm70) == 0
    assert np.array_equal(_bits32(norm70.cpu().numpy()[:TAIL]), _bits32(gn[B - TAIL:B]))


# ---- thread per chunk ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bf16,width,ld", CHUNK_SHAPES, ids=CHUNK_IDS)
def test_residual_forward_past_the_first_grid_trip_and_its_backward(bf16, width, ld):
    """y <- y + x with the mask of y before the addition, over all 2800 rows; then the backward (ReLU derivative from those mask
    bits, G = U + G_in) on the mask the forward wrote"""
    from codae import hip
    lib = hip.lib()
    B, nb = B_CHUNK, (width + 7) // 8
    rng = np.random.default_rng(width * 3 + int(bf16))
    y, a = _res_matrix(rng, B, width, ld, bf16)
    x, h = _res_matrix(rng, B, width, ld, bf16)
    bits = torch.full((B + 1, nb + 1), 0xAA, dtype=torch.uint8, device=DEV)
    assert lib.codae_residual_fwd(hip.ptr(y), hip.ptr(x), int(bf16), ld, ld, B, width, hip.ptr(bits), nb + 1, hip.current_stream()) == 0
    torch.cuda.synchronize()
    want = a.copy()
    want[:B, :width] = _round(a[:B, :width] + h[:B, :width], bf16)
    got = y.float().cpu().numpy()
    assert np.array_equal(_bits32(got), _bits32(want)), np.argwhere(_bits32(got) != _bits32(want))[:8]          # values, pad columns, pad rows
    assert np.array_equal(x.float().cpu().numpy(), h)                                                           # the input is read only
    gb = bits.cpu().numpy()
    wb = RR.packed_mask(a[:B, :width])
    assert np.array_equal(gb[:B, :nb], wb), np.flatnonzero((gb[:B, :nb] != wb).any(axis=1))[:8]
    assert (gb[:B, nb] == 0xAA).all() and (gb[B] == 0xAA).all()
    y2, _ = _work(a, bf16)                                                                                      # without a mask buffer
    assert lib.codae_residual_fwd(hip.ptr(y2), hip.ptr(x), int(bf16), ld, ld, B, width, None, 0, hip.current_stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(_raw(y2), _raw(y))
    # the backward on those bits
    ld_g = ld + 4
    d, u = _res_matrix(rng, B, width, ld, bf16, special=False)
    gi = np.full((B + 2, ld_g), POISON, dtype=np.float32)
    gi[:B, :width] = rng.standard_normal((B, width)).astype(np.float32)
    G = (u[:B, :width] + gi[:B, :width]).astype(np.float32)
    D = _round(np.where(RR.positive(a[:B, :width]), G, np.float32(0)), bf16)
    g_in = torch.tensor(gi, device=DEV)
    g_out = torch.full_like(g_in, POISON)
    rc, cs = _res_bwd(d, bf16, ld, B, width, g_in=g_in, g_out=g_out, ld_g=ld_g, bits=bits, ld_bits=nb + 1, kind=1)
    assert rc == 0, lib.codae_last_error()
    gd, go = d.float().cpu().numpy(), g_out.cpu().numpy()
    assert np.array_equal(_bits32(gd[:B, :width]), _bits32(D)) and (gd[:, width:] == POISON).all() and (gd[B:] == POISON).all()
    assert np.array_equal(_bits32(go[:B, :width]), _bits32(G)) and (go[:, width:] == POISON).all() and (go[B:] == POISON).all()
    blocks = (B + 63) // 64
    csn = cs.cpu().numpy()
    assert (csn[blocks] == POISON).all()
    assert np.array_equal(_bits32(csn[:blocks]), _bits32(RR.colsum_parts_fixed_order(D, B)))
    assert np.array_equal(bits.cpu().numpy(), gb)


@pytest.mark.parametrize("bf16,width,ld", CHUNK_SHAPES, ids=CHUNK_IDS)
def test_dropout_forward_past_the_first_grid_trip_and_its_backward(bf16, width, ld):
    """a <- a * f over all 2800 rows under a permuted row_idx, then d <- d * f of the same (rows, layer, step, seed): the mask is
    never stored, the backward regenerates the one the forward applied.  The factor comes from dropout_ref.words_vec, the plain
    Philox of dropout_ref.words in whole-array arithmetic; the two are compared on the first and last rows and the rows either side
    of the trip boundary."""
    B, layer, step, p = B_CHUNK, 1, 5, 0.25
    rng = np.random.default_rng(100 + width)
    rows = rng.permutation(B + 200)[:B].astype(np.int32)
    rows_t = torch.tensor(rows, device=DEV)
    w = DR.words_vec(rows, layer, width, step, SEED)
    c_drop = chunk_cols(bf16, width, ld)[1]
    edge = (2048 * 256) // ((width + c_drop - 1) // c_drop)                   # the batch row the first trip ends in
    assert 0 < edge < B - 1
    for r in (0, edge - 1, edge, edge + 1, B - 1):
        assert np.array_equal(w[r], DR.words(rows[r:r + 1], layer, width, step, SEED)[0]), r
    f = np.where(w.astype(np.uint64) < np.uint64(DR.threshold(p)), np.float32(0), DR.scale(p)).astype(np.float32)
    assert 0.2 < float((f == 0).mean()) < 0.3
    t, a = _drop_matrix(rng, bf16, B + 2, width, ld, B)
    assert drop_fwd(t, bf16, ld, B, width, rows_t, layer, step, p) == 0
    want = a.copy()
    want[:B, :width] = DR.apply(a[:B, :width], f, bf16)
    assert _same_bits(t, want)                                  # values exact; pad columns and the rows past B keep their prefill
    assert (t[:, width:].float() == FILL).all() and (t[B:].float() == FILL).all()
    d, g = _drop_matrix(rng, bf16, B + 2, width, ld, B)
    rc, colsum = drop_bwd(d, bf16, ld, B, width, rows_t, layer, step, p)
    assert rc == 0
    want_d = g.copy()
    want_d[:B, :width] = DR.apply(g[:B, :width], f, bf16)
    assert _same_bits(d, want_d)
    assert (d[:, width:].float() == FILL).all() and (d[B:].float() == FILL).all()
    blocks = (B + 63) // 64
    cs = colsum.cpu().numpy()
    assert (cs[blocks] == FILL).all()
    d64 = want_d[:B, :width].astype(np.float64)
    bound = 1e-5 * np.abs(d64).sum(axis=0)
    assert (np.abs(cs[:blocks].astype(np.float64).sum(axis=0) - d64.sum(axis=0)) <= bound).all()
    assert np.array_equal(_bits32(cs[:blocks]), _bits32(RR.colsum_parts_fixed_order(want_d[:B, :width], B)))
