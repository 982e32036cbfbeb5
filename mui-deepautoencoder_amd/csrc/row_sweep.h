// The backward sweep of the streaming kernels that sit between a step's GEMMs (dropout.hip, residual.hip, norm.hip), written once,
// with what their launchers share: the gradient carry and the 1-bit-mask derivative of StreamBwd, the 16-B predicate and the
// <BF16, VEC> dispatch.
//
// One block per 64 batch rows and all columns (the row blocks of the fp32 GEMM's column sums, so the layer's partial-sum rows are
// enough).  1024 threads: wave w of 16 owns rows 4 w .. 4 w + 3 of the block, its 64 lanes own 64 consecutive chunks of C columns;
// the block walks the width in tiles of 64 chunks.  Per tile a thread has its four rows' 16-B loads in flight together (64 KiB per
// block - a batch of 8192 rows is 128 blocks, one per CU on half the chip, so the bytes in flight per CU must be high: 4 waves per
// SIMD x 64 B per lane), adds their STORED values in row order in registers, and the 16 waves' sums meet in LDS, added in wave order
// by one thread per column: a fixed order, no atomics, and LDS sized by the tile (C = 8: 32 KiB), not by the width.  (A 256-thread
// block that loops over the rows keeps 4 x fewer bytes in flight per CU; one column chunk per thread with all 64 rows in a loop
// needs no LDS but gives 3 waves per block at width 1536.)
#pragma once
#include <initializer_list>
#include <type_traits>
#include "row_access.h"

namespace codae {
namespace {

constexpr int SWEEP_ROWS = 64, SWEEP_WAVES = 16, SWEEP_NT = 64 * SWEEP_WAVES, SWEEP_RPW = SWEEP_ROWS / SWEEP_WAVES;

// the first of the SWEEP_RPW rows of this thread's wave (a kernel's prologue walks the same rows as the sweep)
__device__ __forceinline__ int sweep_row0() { return blockIdx.x * SWEEP_ROWS + (threadIdx.x >> 6) * SWEEP_RPW; }

// chunk(b, i, c, out): the kernel's work on columns [c, c + C) of batch row b < B, the wave's row i; out[k] = the value it STORED,
// widened to fp32 (0 for a column past the width).  colsum_part [blocks][width]: the block's column sums of those values, or null.
template <int C, class Chunk>
__device__ __forceinline__ void row_sweep(int B, int width, float* __restrict__ colsum_part, Chunk chunk) {
    constexpr int TILE = 64 * C;                               // columns per tile
    __shared__ float red[SWEEP_WAVES][TILE];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row0 = sweep_row0();
    for (int t0 = 0; t0 < width; t0 += TILE) {
        const int c = t0 + lane * C;
        float sum[C];
#pragma unroll
        for (int k = 0; k < C; ++k) sum[k] = 0.f;
        if (c < width) {
#pragma unroll
            for (int i = 0; i < SWEEP_RPW; ++i) {
                const int b = row0 + i;
                if (b < B) {
                    float out[C];
                    chunk(b, i, c, out);
#pragma unroll
                    for (int k = 0; k < C; ++k) sum[k] = opaque(sum[k] + out[k]);
                }
            }
        }
        if (colsum_part != nullptr) {                          // (block-uniform)
#pragma unroll
            for (int k = 0; k < C; ++k) red[wave][lane * C + k] = sum[k];
            __syncthreads();
            if (threadIdx.x < TILE && t0 + (int)threadIdx.x < width) {
                float s = red[0][threadIdx.x];
#pragma unroll
                for (int w = 1; w < SWEEP_WAVES; ++w) s = opaque(s + red[w][threadIdx.x]);
                colsum_part[(int64_t)blockIdx.x * width + t0 + threadIdx.x] = s;
            }
            __syncthreads();
        }
    }
}

// columns per thread and step of the dropout and residual sweeps: 8 bf16 or 4 fp32 in one 16-B access, 4 element by element
template <bool BF16, bool VEC>
constexpr int access_cols() { return (BF16 && VEC) ? 8 : 4; }

// Gh columns [c, c + C) of row b: U from the row of d, + G when the layer behind is skipped (one fp32 add)
template <bool BF16, bool VEC, int C>
__device__ __forceinline__ void load_gh(const void* drow, const StreamBwd& s, int b, int c, int width, float* g) {
    load_work<BF16, VEC, C>(drow, c, width, g);
    if (s.g_in != nullptr) {
        float gi[C];
        load_work<false, VEC, C>(s.g_in + (int64_t)b * s.ld_g, c, width, gi);
#pragma unroll
        for (int k = 0; k < C; ++k) g[k] = opaque(g[k] + gi[k]);
    }
}

// G columns [c, c + C) of row b <- g, when the layer this gradient reaches is skipped too
template <bool VEC, int C>
__device__ __forceinline__ void store_g(const StreamBwd& s, int b, int c, int width, const float* g) {
    if (s.g_out != nullptr) {
        float unused[C];
        store_work<false, VEC, C>(s.g_out + (int64_t)b * s.ld_g, c, width, g, unused);
    }
}

// g <- g * act' from the 1-bit mask of row b (column 8 j + k in bit k of byte j): ReLU selects 0 under a dead unit, LeakyReLU
// multiplies by the slope.  A 4-column chunk is one half of its byte.
template <int C>
__device__ __forceinline__ void mask_deriv(const StreamBwd& s, int b, int c, float* g) {
    uint32_t m = (uint32_t)s.bits[(int64_t)b * s.ld_bits + (c >> 3)];
    if constexpr (C < 8) m >>= (c & 7);
    const bool selects = s.act_kind == CODAE_ACT_RELU;
#pragma unroll
    for (int k = 0; k < C; ++k) g[k] = ((m >> k) & 1u) ? g[k] : (selects ? 0.f : opaque(g[k] * s.slope));
}

// ---- host side --------------------------------------------------------------------------------------------------------------
// what launch_residual_bwd and launch_norm_bwd ask of the part they share
inline int check_stream_bwd(const char* who, const StreamBwd& s, int width) {
    CODAE_REQUIRE((s.g_in == nullptr && s.g_out == nullptr) || s.ld_g >= width, "%s: ld_g %lld for %d columns", who, (long long)s.ld_g, width);
    CODAE_REQUIRE(s.bits == nullptr || s.ld_bits >= (width + 7) / 8, "%s: ld_bits %lld for %d columns", who, (long long)s.ld_bits, width);
    CODAE_REQUIRE(s.bits == nullptr || s.act_kind == CODAE_ACT_RELU || s.act_kind == CODAE_ACT_LEAKY,
                  "%s: 1-bit masks carry the derivative of ReLU and LeakyReLU only (kind %d)", who, s.act_kind);
    return CODAE_OK;
}

// 16-B accesses: every row of every matrix starts 16-B aligned and holds whole chunks (a null matrix is not accessed)
struct RowMatrix { const void* p; int64_t ld; };
inline bool rows_vec16(int bf16, int width, std::initializer_list<RowMatrix> work, const StreamBwd* carry = nullptr) {
    const int per = bf16 ? 8 : 4;
    bool vec = width % per == 0;
    for (const RowMatrix& m : work) vec = vec && aligned16(m.p) && m.ld % per == 0;
    if (carry != nullptr && (carry->g_in != nullptr || carry->g_out != nullptr))
        vec = vec && aligned16(carry->g_in) && aligned16(carry->g_out) && carry->ld_g % 4 == 0;
    return vec;
}

// launch(std::bool_constant<BF16>, std::bool_constant<VEC>): the instantiation picked at run time
template <class Launch>
inline void dispatch_bf16_vec(int bf16, bool vec, Launch launch) {
    if (bf16) { if (vec) launch(std::true_type{}, std::true_type{}); else launch(std::true_type{}, std::false_type{}); }
    else { if (vec) launch(std::false_type{}, std::true_type{}); else launch(std::false_type{}, std::false_type{}); }
}

}  // namespace
}  // namespace codae
