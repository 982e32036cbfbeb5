// Hidden dropout (codae_dropout, include/codae_hip.h): two in-place streaming kernels between the GEMMs of a training step.
//   forward   act[l + 1] <- act[l + 1] * f      behind the forward GEMM of a dropped layer l
//   backward  dA_l <- dA_l * f, + column sums   behind the data-gradient GEMM that produced dA_l
// f = 0 or 1 / (1 - p) from one Philox4x32-10 word per element, counter (column / 4, DATASET row, Adam step, 1 + layer): a
// thread always covers whole Philox groups, so one generator call serves four columns.  16 B per lane where the matrix allows
// (bf16: two groups, fp32: one), element accesses otherwise (the fp32 engine runs widths like 21 and 11); pad columns and pad
// rows are never written.
#include "codae_common.h"

namespace codae {
namespace {

struct DropArgs {
    uint32_t key0, key1;       // seed & 0xffffffff, seed >> 32
    uint32_t step;             // counter word 2 ...
    const double* step_dev;    // ... or, when not null, *step_dev (graph replay)
    uint32_t word3;            // counter word 3: 1 + layer
    uint64_t thresh;           // T = floor(p 2^32)
    float scale;               // (float)(1 / (1 - p))
};

// the factors of columns 4 g .. 4 g + 3 of dataset row `row`
__device__ __forceinline__ void drop_factors4(float* f, uint32_t g, uint32_t row, uint32_t step, const DropArgs& a) {
    const uint4 r = philox4x32_10(g, row, step, a.word3, a.key0, a.key1);
    f[0] = (uint64_t)r.x < a.thresh ? 0.f : a.scale;
    f[1] = (uint64_t)r.y < a.thresh ? 0.f : a.scale;
    f[2] = (uint64_t)r.z < a.thresh ? 0.f : a.scale;
    f[3] = (uint64_t)r.w < a.thresh ? 0.f : a.scale;
}

// columns per thread and step: 8 bf16 or 4 fp32 in one 16-B access; 4 (one Philox group) element by element otherwise
template <bool BF16, bool VEC>
constexpr int chunk_cols() { return (BF16 && VEC) ? 8 : 4; }

// columns [c, c + chunk) of the row at `row_ptr` <- value * factor (fp32 product, bf16 stored round-to-nearest-even); out[k] = the
// STORED value widened to fp32 (0 for a column past the width, which is neither read nor written)
template <bool BF16, bool VEC>
__device__ __forceinline__ void drop_chunk(void* row_ptr, int c, int width, uint32_t row, uint32_t step, const DropArgs& a, float* out) {
    constexpr int C = chunk_cols<BF16, VEC>();
    float f[C];
    drop_factors4(f, (uint32_t)(c >> 2), row, step, a);
    if constexpr (C == 8) drop_factors4(f + 4, (uint32_t)(c >> 2) + 1u, row, step, a);
    if constexpr (BF16 && VEC) {
        uint4* p = reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(row_ptr) + c);
        const uint4 v = *p;
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint32_t o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float lo = opaque(bf16_to_f32((bf16_t)(w[k] & 0xffffu)) * f[2 * k]);
            const float hi = opaque(bf16_to_f32((bf16_t)(w[k] >> 16)) * f[2 * k + 1]);
            o[k] = pack_bf16x2(lo, hi);
            out[2 * k] = __uint_as_float(o[k] << 16);
            out[2 * k + 1] = __uint_as_float(o[k] & 0xffff0000u);
        }
        *p = make_uint4(o[0], o[1], o[2], o[3]);
    } else if constexpr (VEC) {
        float4* p = reinterpret_cast<float4*>(reinterpret_cast<float*>(row_ptr) + c);
        const float4 v = *p;
        out[0] = opaque(v.x * f[0]); out[1] = opaque(v.y * f[1]); out[2] = opaque(v.z * f[2]); out[3] = opaque(v.w * f[3]);
        *p = make_float4(out[0], out[1], out[2], out[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            out[k] = 0.f;
            if (c + k < width) {
                if constexpr (BF16) {
                    bf16_t* p = reinterpret_cast<bf16_t*>(row_ptr) + c + k;
                    const bf16_t o = f32_to_bf16(opaque(bf16_to_f32(*p) * f[k]));
                    *p = o;
                    out[k] = bf16_to_f32(o);
                } else {
                    float* p = reinterpret_cast<float*>(row_ptr) + c + k;
                    out[k] = opaque(*p * f[k]);
                    *p = out[k];
                }
            }
        }
    }
}

// ---- forward ----------------------------------------------------------------------------------------------------------------
// Block shape: 256 threads, one 16-B chunk per thread and iteration, grid capped at 2048 blocks (8 per CU) with a grid-stride
// loop - the shape of the gather kernels, which this kernel resembles (same Philox work per element, read + write instead of a
// random-row read + write).  27 VGPRs: eight waves per SIMD, so the 16-B loads of 32 waves per CU cover the HBM latency.
constexpr int FWD_NT = 256;

template <bool BF16, bool VEC>
__global__ __launch_bounds__(FWD_NT) void dropout_fwd_kernel(void* __restrict__ a, int64_t ld, int B, int width,
                                                             const int32_t* __restrict__ row_idx, DropArgs da) {
    constexpr int C = chunk_cols<BF16, VEC>();
    constexpr int ES = BF16 ? 2 : 4;
    const uint32_t step = da.step_dev ? (uint32_t)*da.step_dev : da.step;
    const int chunks = (width + C - 1) / C;
    const int64_t total = (int64_t)B * chunks;
    for (int64_t e = (int64_t)blockIdx.x * FWD_NT + threadIdx.x; e < total; e += (int64_t)gridDim.x * FWD_NT) {
        const int b = (int)(e / chunks);
        const int c = (int)(e - (int64_t)b * chunks) * C;
        const uint32_t row = row_idx ? (uint32_t)row_idx[b] : (uint32_t)b;
        float out[C];
        drop_chunk<BF16, VEC>(reinterpret_cast<char*>(a) + (int64_t)b * ld * ES, c, width, row, step, da, out);
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
// One block per 64 batch rows and all columns (the row blocks of the fp32 GEMM's column sums, so the layer's partial-sum rows are
// enough).  1024 threads: wave w of 16 owns rows 4 w .. 4 w + 3 of the block, its 64 lanes own 64 consecutive chunks; the block
// walks the width in tiles of 64 chunks (512 bf16 / 256 fp32 columns).  Per tile a thread has its four rows' 16-B loads in flight
// together (64 KiB per block - a batch of 8192 rows is 128 blocks, one per CU on half the chip, so the bytes in flight per CU must
// be high: 4 waves per SIMD x 64 B per lane), adds their stored values in row order in registers, and the 16 waves' sums meet in
// LDS, added in wave order by one thread per column: a fixed order, no atomics, and LDS sized by the tile (32 KiB), not by the
// width.  (A 256-thread block that loops over the rows keeps 4 x fewer bytes in flight per CU; one column chunk per thread with all
// 64 rows in a loop needs no LDS but gives 3 waves per block at width 1536.)
constexpr int BWD_ROWS = 64, BWD_WAVES = 16, BWD_NT = 64 * BWD_WAVES, BWD_ROWS_PER_WAVE = BWD_ROWS / BWD_WAVES;

template <bool BF16, bool VEC>
__global__ __launch_bounds__(BWD_NT) void dropout_bwd_kernel(void* __restrict__ d, int64_t ld, int B, int width,
                                                             const int32_t* __restrict__ row_idx, float* __restrict__ colsum_part,
                                                             DropArgs da) {
    constexpr int C = chunk_cols<BF16, VEC>();
    constexpr int ES = BF16 ? 2 : 4;
    constexpr int TILE = 64 * C;                               // columns per tile
    __shared__ float red[BWD_WAVES][TILE];
    const uint32_t step = da.step_dev ? (uint32_t)*da.step_dev : da.step;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row0 = blockIdx.x * BWD_ROWS + wave * BWD_ROWS_PER_WAVE;
    uint32_t rid[BWD_ROWS_PER_WAVE];
#pragma unroll
    for (int i = 0; i < BWD_ROWS_PER_WAVE; ++i) {
        const int b = row0 + i;
        rid[i] = b < B ? (row_idx ? (uint32_t)row_idx[b] : (uint32_t)b) : 0u;
    }
    for (int t0 = 0; t0 < width; t0 += TILE) {
        const int c = t0 + lane * C;
        float sum[C];
#pragma unroll
        for (int k = 0; k < C; ++k) sum[k] = 0.f;
        if (c < width) {
#pragma unroll
            for (int i = 0; i < BWD_ROWS_PER_WAVE; ++i) {
                const int b = row0 + i;
                if (b < B) {
                    float out[C];
                    drop_chunk<BF16, VEC>(reinterpret_cast<char*>(d) + (int64_t)b * ld * ES, c, width, rid[i], step, da, out);
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
                for (int w = 1; w < BWD_WAVES; ++w) s = opaque(s + red[w][threadIdx.x]);
                colsum_part[(int64_t)blockIdx.x * width + t0 + threadIdx.x] = s;
            }
            __syncthreads();
        }
    }
}

int drop_args(const char* who, const void* a, int64_t ld, int B, int width, int layer, int32_t step, float p, uint64_t seed,
              const double* step_dev, DropArgs* out) {
    CODAE_REQUIRE(a != nullptr, "%s: null matrix", who);
    CODAE_REQUIRE(B > 0 && width > 0 && ld >= width, "%s: B %d, width %d, ld %lld", who, B, width, (long long)ld);
    CODAE_REQUIRE(layer >= 0 && layer <= 254, "%s: layer %d outside [0, 254]", who, layer);
    CODAE_REQUIRE(step >= 0, "%s: step %d", who, step);
    int rc = check_dropout_p(p, who);
    if (rc) return rc;
    DropArgs d{};
    d.key0 = (uint32_t)(seed & 0xffffffffu); d.key1 = (uint32_t)(seed >> 32);
    d.step = (uint32_t)step; d.step_dev = step_dev;
    d.word3 = 1u + (uint32_t)layer;
    d.thresh = (uint64_t)((double)p * 4294967296.0);           // floor: the product is exact (24 significant bits) and >= 0
    d.scale = (float)(1.0 / (1.0 - (double)p));
    *out = d;
    return CODAE_OK;
}

// 16-B accesses: every row starts 16-B aligned and holds whole chunks
bool drop_vec(const void* a, int bf16, int64_t ld, int width) {
    const int per = bf16 ? 8 : 4;
    return (reinterpret_cast<uintptr_t>(a) & 15u) == 0 && ld % per == 0 && width % per == 0;
}

}  // namespace

int check_dropout_p(float p, const char* who) {
    CODAE_REQUIRE(p == p && p >= 0.f && p < 1.f, "%s: p %g outside [0, 1)", who, (double)p);
    return CODAE_OK;
}

int launch_dropout_fwd(void* a, int bf16, int64_t ld, int B, int width, const int32_t* row_idx, int layer, int32_t step,
                       const double* step_dev, float p, uint64_t seed, hipStream_t s) {
    DropArgs da;
    int rc = drop_args("codae_dropout_fwd", a, ld, B, width, layer, step, p, seed, step_dev, &da);
    if (rc) return rc;
    const bool vec = drop_vec(a, bf16, ld, width);
    const int C = (bf16 && vec) ? 8 : 4;
    int64_t blocks = ((int64_t)B * ((width + C - 1) / C) + FWD_NT - 1) / FWD_NT;
    if (blocks > 2048) blocks = 2048;
#define DF(BF, V) hipLaunchKernelGGL((dropout_fwd_kernel<BF, V>), dim3((unsigned)blocks), dim3(FWD_NT), 0, s, a, ld, B, width, row_idx, da)
    if (bf16) { if (vec) DF(true, true); else DF(true, false); }
    else { if (vec) DF(false, true); else DF(false, false); }
#undef DF
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_dropout_bwd(void* d, int bf16, int64_t ld, int B, int width, const int32_t* row_idx, int layer, int32_t step,
                       const double* step_dev, float p, uint64_t seed, float* colsum_part, hipStream_t s) {
    DropArgs da;
    int rc = drop_args("codae_dropout_bwd", d, ld, B, width, layer, step, p, seed, step_dev, &da);
    if (rc) return rc;
    const bool vec = drop_vec(d, bf16, ld, width);
    const int blocks = dropout_blocks(B);
#define DB(BF, V) hipLaunchKernelGGL((dropout_bwd_kernel<BF, V>), dim3(blocks), dim3(BWD_NT), 0, s, d, ld, B, width, row_idx, colsum_part, da)
    if (bf16) { if (vec) DB(true, true); else DB(true, false); }
    else { if (vec) DB(false, true); else DB(false, false); }
#undef DB
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

}  // namespace codae
