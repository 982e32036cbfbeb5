"""The shapes of the large-input tests really cross the limits they are named after (no GPU).  The limits are read from the kernel
sources - the sort chunk, the centroid group and MAX_K of csrc/kmeans.hip, the block caps and block shapes of the capped grids, the
staged chunk and block cap of the AUC kernel - and the shapes are imported from the test modules, so a later change of a cap fails
here instead of silently turning a second-trip test back into a single-trip one.  A shape also stays below 1.6 times its limit:
what the tests need is one whole trip and a ragged second one, and anything more only costs time."""
import os
import re

import pytest

pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mui-deepautoencoder_amd", "csrc")
SLACK = 1.6


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _const(text, name):
    m = re.search(r"\b%s\s*=\s*([^,;]+)[,;]" % name, text)
    assert m, name
    return m.group(1).strip()


def _int(text, name):
    return int(_const(text, name))


def _cap(text):
    """the N of the launcher's `if (blocks > N) blocks = N;`"""
    m = re.search(r"if \((?:blocks|b) > (\d+)\) (?:blocks|b) = (\d+);", text)
    assert m and m.group(1) == m.group(2)
    return int(m.group(1))


def _crosses(n, limit):
    return limit < n < SLACK * limit


def test_the_cluster_shapes_cross_the_sort_chunk_and_the_centroid_groups():
    import test_gpu_clusters as T
    km = _src("kmeans.hip")
    chunk = int(re.search(r"SORT_CHUNK = (\d+)", km).group(1))
    ct = int(re.search(r"constexpr int CT = (\d+);", km).group(1))
    assert re.search(r"GROUP = 16 \* CT\b", km)
    group, max_k = 16 * ct, _int(km, "MAX_K")
    assert (T.SORT_CHUNK, T.GROUP, T.MAX_K) == (chunk, group, max_k)
    assert re.search(r"launch_bounds__\(1024\) void cluster_scan_kernel", km) and "const int j = %d * tid + q;" % T.SCAN_CLUSTERS in km
    assert 1024 * T.SCAN_CLUSTERS == max_k                                    # MAX_K puts a cluster on the scan's last thread
    # M: a whole chunk, one row more, and two chunks with a ragged third
    assert T.CHUNK_MS[0] == chunk and T.CHUNK_MS[1] == chunk + 1
    assert _crosses(T.CHUNK_MS[2], 2 * chunk) and T.CHUNK_MS[2] % chunk != 0
    assert T.FIT_CHUNKED[2] == T.CHUNK_MS[2]
    small_k = max(K for K, M in T.KM if M >= 700)                             # the most clusters an update test had before
    assert small_k == 300
    ks = sorted({K for K, Z, M, kind in T.CHUNK_CASES})
    assert ks[-1] == max_k and any((small_k + T.SCAN_CLUSTERS - 1) // T.SCAN_CLUSTERS * T.SCAN_CLUSTERS < K < max_k for K in ks)
    for K, Z, M, kind in T.CHUNK_CASES:
        n_chunks = (M + chunk - 1) // chunk
        if kind != "round_robin":
            assert n_chunks == 3, (K, Z, M, kind)
        if K == max_k:
            assert _crosses(M, K) and n_chunks > 2 and M % chunk != 0        # more rows than clusters, by little
    assert any(Z > 64 for K, Z, M, kind in T.CHUNK_CASES)                     # two column blocks of the member sum
    assert int(re.search(r"SUM_COLS = (\d+)", km).group(1)) == 64
    # K: the last centroid of a whole group, one tile past it, and the most there can be
    ks = {K for K, M in T.KM}
    assert {group, group + 1, max_k} <= ks and all(Z in (8, 40) for Z, K, M in T.ZKM if K == max_k)
    assert all((Z, K, M) in T.ZKM for Z in T.ZS for K, M in T.KM if K < max_k)


def test_the_row_counts_cross_the_capped_grids_of_the_wave_per_row_forwards():
    import test_gpu_second_trips as T
    for name in ("sparse_code.hip", "norm.hip"):
        text = _src(name)
        assert _int(text, "FWD_WAVES") == T.WAVE_ROWS_PER_BLOCK and _const(text, "FWD_NT") == "64 * FWD_WAVES"
        assert _crosses(T.B_WAVE, _cap(text) * _int(text, "FWD_WAVES")), name
    text = _src("codes.hip")
    assert _int(text, "EXP_WAVES") == T.WAVE_ROWS_PER_BLOCK
    assert _crosses(T.B_WAVE, _cap(text) * _int(text, "EXP_WAVES"))
    cap_rows = _cap(text) * T.WAVE_ROWS_PER_BLOCK
    assert T.B_WAVE - cap_rows == T.TAIL and T.TAIL % T.WAVE_ROWS_PER_BLOCK == 2      # whole blocks and one with two live waves
    # the three access paths: bf16 16-byte, fp32 element, fp32 16-byte ending in half a chunk
    assert [(bf16, (w * (2 if bf16 else 4)) % 16 == 0 and (ld * (2 if bf16 else 4)) % 16 == 0, w % 8) for bf16, w, ld in T.WAVE_SHAPES] == \
        [(True, True, 0), (False, False, 5), (False, True, 4)]


def test_the_matrices_cross_the_capped_grids_of_the_thread_per_chunk_forwards():
    import test_gpu_second_trips as T
    res, drop = _src("residual.hip"), _src("dropout.hip")
    assert _int(res, "FWD_C") == 8 and _int(res, "FWD_NT") == 256 and _int(drop, "FWD_NT") == 256
    assert "const int C = (bf16 && vec) ? 8 : 4;" in drop
    per_trip = {"residual": _cap(res) * _int(res, "FWD_NT"), "dropout": _cap(drop) * _int(drop, "FWD_NT")}
    ratios = []
    for bf16, width, ld in T.CHUNK_SHAPES:
        for name, cols in zip(("residual", "dropout"), T.chunk_cols(bf16, width, ld)):
            items = T.B_CHUNK * ((width + cols - 1) // cols)
            assert items > per_trip[name], (name, bf16, width)
            # B is set by the coarsest chunking (8 columns); a 4-column one makes twice the items of the same matrix
            assert items < SLACK * per_trip[name] * 8 / cols, (name, bf16, width)
            ratios.append(items / per_trip[name])
    assert min(ratios) < 1.1                                                  # the coarsest only just crosses
    assert [T.chunk_cols(*s) for s in T.CHUNK_SHAPES] == [(8, 8), (8, 4), (8, 4)]


def test_the_large_gather_crosses_the_capped_grid_of_both_output_types():
    import test_gpu_gather_widths as T
    common, gather = _src("codae_common.h"), _src("gather.hip")
    m = re.search(r"inline int grid_for\(int64_t work_items\) \{(.*?)\n\}", common, re.S)
    per_trip = _cap(m.group(1)) * _int(common, "GRID_NT")
    assert "const int grid = grid_for(x8 ? items / 2 : items);" in gather and "(vec ? b->io / 4 : b->io)" in gather
    assert T.BIG_IO % 8 == 0 and T.BIG_IO % T.BIG_SLOTS == 0
    assert _crosses(T.big_groups(True), per_trip)                             # 8-wide: one trip and a little
    assert per_trip < T.big_groups(False) < 2 * SLACK * per_trip              # 4-wide: twice the groups of the same matrix


def test_the_auc_cases_cross_the_staged_chunk_and_the_capped_grid():
    import test_gpu_compat as T
    common, compat = _src("codae_common.h"), _src("compat.hip")
    nt = _int(common, "GRID_NT")
    assert re.search(r"constexpr int NT = GRID_NT;", compat) and _const(compat, "AUC_CHUNK") == "4 * NT"
    per_trip = _int(compat, "AUC_MAX_BLOCKS") * nt
    big = [(P, M) for P, M in T.AUC_PM if M > per_trip]
    assert len(big) == 2 and all(_crosses(M, per_trip) and M % nt != 0 for P, M in big)
    ps = sorted(P for P, M in big)
    assert ps[0] < 4 * nt and _crosses(ps[1], 4 * nt) and ps[1] % 4 != 0      # no whole chunk; one whole chunk and a ragged one


def test_the_kernel_shape_lists_hold_fp32_widths_that_end_in_half_a_chunk_on_the_16_byte_path():
    import test_gpu_codes
    import test_gpu_norm
    import test_gpu_residual
    import test_gpu_sparse_code
    assert test_gpu_codes.SHAPES is test_gpu_norm.SHAPES
    for mod in (test_gpu_norm, test_gpu_residual, test_gpu_sparse_code):
        assert len(mod.SHAPES) == len(mod.SHAPE_IDS) == len(set(mod.SHAPE_IDS))
        half = [(w, ld) for bf16, w, ld in mod.SHAPES if not bf16 and w % 8 == 4 and w % 4 == 0 and ld % 4 == 0]
        assert {(12, 12), (20, 24), (516, 516)} <= set(half), mod.__name__
        assert any(w == ld for w, ld in half) and any(w < ld for w, ld in half)
        assert any(512 < w < 520 for w, ld in half)                           # the half chunk in the first lane of the second tile
        assert len(mod.ROWS) >= 3
    assert set(test_gpu_sparse_code.HALF_TIES) == {10, 11, 12, 13, 514, 515, 516, 517}
    assert all(4 in test_gpu_sparse_code._keeps(w) for w in (12, 20, 516))
