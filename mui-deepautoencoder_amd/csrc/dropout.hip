// Hidden dropout (codae_dropout, include/codae_hip.h): two in-place streaming kernels between the GEMMs of a training step.
//   forward   act[l + 1] <- act[l + 1] * f      behind the forward GEMM of a dropped layer l
//   backward  dA_l <- dA_l * f, + column sums   behind the data-gradient GEMM that produced dA_l
// f = 0 or 1 / (1 - p) from one Philox4x32-10 word per element, counter (column / 4, DATASET row, Adam step, 1 + layer): a
// thread always covers whole Philox groups, so one generator call serves four columns.  16 B per lane where the matrix allows
// (bf16: two groups, fp32: one), element accesses otherwise (the fp32 engine runs widths like 21 and 11), through the accessors of
// row_access.h; pad columns and pad rows are never written.  The backward kernel is the sweep of row_sweep.h.
#include "codae_common.h"
#include "row_sweep.h"

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

// columns [c, c + chunk) of the row at `row_ptr` <- value * factor (fp32 product, bf16 stored round-to-nearest-even); out[k] = the
// STORED value widened to fp32 (0 for a column past the width, which is neither read nor written).  One Philox call per 4 columns.
template <bool BF16, bool VEC>
__device__ __forceinline__ void drop_chunk(void* row_ptr, int c, int width, uint32_t row, uint32_t step, const DropArgs& a, float* out) {
    constexpr int C = access_cols<BF16, VEC>();
    float f[C], v[C];
    drop_factors4(f, (uint32_t)(c >> 2), row, step, a);
    if constexpr (C == 8) drop_factors4(f + 4, (uint32_t)(c >> 2) + 1u, row, step, a);
    load_work<BF16, VEC, C>(row_ptr, c, width, v);
#pragma unroll
    for (int k = 0; k < C; ++k) v[k] = opaque(v[k] * f[k]);
    store_work<BF16, VEC, C>(row_ptr, c, width, v, out);
}

// ---- forward ----------------------------------------------------------------------------------------------------------------
// Block shape: 256 threads, one 16-B chunk per thread and iteration, grid capped at 2048 blocks (8 per CU) with a grid-stride
// loop - the shape of the gather kernels, which this kernel resembles (same Philox work per element, read + write instead of a
// random-row read + write).  27 VGPRs: eight waves per SIMD, so the 16-B loads of 32 waves per CU cover the HBM latency.
constexpr int FWD_NT = 256;

template <bool BF16, bool VEC>
__global__ __launch_bounds__(FWD_NT) void dropout_fwd_kernel(void* __restrict__ a, int64_t ld, int B, int width,
                                                             const int32_t* __restrict__ row_idx, DropArgs da) {
    constexpr int C = access_cols<BF16, VEC>();
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
// The shared sweep (row_sweep.h) over drop_chunk; the prologue: the dataset rows of the wave's four batch rows.
template <bool BF16, bool VEC>
__global__ __launch_bounds__(SWEEP_NT) void dropout_bwd_kernel(void* __restrict__ d, int64_t ld, int B, int width,
                                                               const int32_t* __restrict__ row_idx, float* __restrict__ colsum_part,
                                                               DropArgs da) {
    constexpr int ES = BF16 ? 2 : 4;
    const uint32_t step = da.step_dev ? (uint32_t)*da.step_dev : da.step;
    const int row0 = sweep_row0();
    uint32_t rid[SWEEP_RPW];
#pragma unroll
    for (int i = 0; i < SWEEP_RPW; ++i) {
        const int b = row0 + i;
        rid[i] = b < B ? (row_idx ? (uint32_t)row_idx[b] : (uint32_t)b) : 0u;
    }
    row_sweep<access_cols<BF16, VEC>()>(B, width, colsum_part, [=](int b, int i, int c, float* out) {
        drop_chunk<BF16, VEC>(reinterpret_cast<char*>(d) + (int64_t)b * ld * ES, c, width, rid[i], step, da, out);
    });
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
    const bool vec = rows_vec16(bf16, width, {{a, ld}});
    const int C = (bf16 && vec) ? 8 : 4;
    int64_t blocks = ((int64_t)B * ((width + C - 1) / C) + FWD_NT - 1) / FWD_NT;
    if (blocks > 2048) blocks = 2048;
    dispatch_bf16_vec(bf16, vec, [&](auto BF, auto V) {
        hipLaunchKernelGGL((dropout_fwd_kernel<decltype(BF)::value, decltype(V)::value>), dim3((unsigned)blocks), dim3(FWD_NT), 0, s, a, ld, B,
                           width, row_idx, da);
    });
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_dropout_bwd(void* d, int bf16, int64_t ld, int B, int width, const int32_t* row_idx, int layer, int32_t step,
                       const double* step_dev, float p, uint64_t seed, float* colsum_part, hipStream_t s) {
    DropArgs da;
    int rc = drop_args("codae_dropout_bwd", d, ld, B, width, layer, step, p, seed, step_dev, &da);
    if (rc) return rc;
    dispatch_bf16_vec(bf16, rows_vec16(bf16, width, {{d, ld}}), [&](auto BF, auto V) {
        hipLaunchKernelGGL((dropout_bwd_kernel<decltype(BF)::value, decltype(V)::value>), dim3(row_sweep_blocks(B)), dim3(SWEEP_NT), 0, s, d, ld,
                           B, width, row_idx, colsum_part, da);
    });
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

}  // namespace codae
