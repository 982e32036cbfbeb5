// Outfit codes (codae_export_rows, include/codae_hip.h): one streaming kernel behind the forward GEMMs of codae_encode; a wave owns
// a row, as in norm.hip's forward.
//   export   dst[b][c] <- the STORED src[b][c] widened to fp32, exactly (a bf16 is its 16 bits shifted up; -0, NaN payloads and all),
//            norm[b] <- sqrt(sum_c v^2) in fp32: the row norm the bank search divides by, in the pass that writes the bank
// One pass: every element is read once and written once, nothing is kept across chunks but the lane's partial sum.
// Templates on <BF16, VEC>: 16 B per access where both sides allow it (row_access.h's rule for src; dst 16-B aligned with ld_dst a
// multiple of 4), element accesses otherwise.  A lane owns the same 8 columns per chunk on either path and adds them in ascending
// order, the 64 lanes are combined in one fixed tree (wave_sum): the bits of norm[b] depend on the row's values and the width alone.
// No atomics: a NaN or Inf stays in its row.  Pad columns and pad rows of dst are never written, src is never written.
#include "codae_common.h"
#include "row_sweep.h"

namespace codae {
namespace {

constexpr int NC = 8;                                          // columns of a lane per chunk, whatever the type (norm.hip's)
constexpr int EXP_WAVES = 4, EXP_NT = 64 * EXP_WAVES;

template <bool BF16, bool VEC>
__global__ __launch_bounds__(EXP_NT) void export_rows_kernel(const void* __restrict__ src, int64_t ld_src, int B, int width,
                                                             float* __restrict__ dst, int64_t ld_dst, float* __restrict__ norm) {
    constexpr int ES = BF16 ? 2 : 4;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int b = blockIdx.x * EXP_WAVES + wave; b < B; b += gridDim.x * EXP_WAVES) {
        const char* row = reinterpret_cast<const char*>(src) + (int64_t)b * ld_src * ES;
        float* out = dst + (int64_t)b * ld_dst;
        float s = 0.f;
        for (int c = lane * NC; c < width; c += 64 * NC) {
            float x[NC];
            load_work<BF16, VEC, NC>(row, c, width, x);
#pragma unroll
            for (int k = 0; k < NC; ++k) s = opaque(s + opaque(x[k] * x[k]));      // (a column past the width was loaded as +0)
            if constexpr (VEC) {
#pragma unroll
                for (int q = 0; q < NC / 4; ++q)
                    if (c + 4 * q < width) *reinterpret_cast<float4*>(out + c + 4 * q) = make_float4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
            } else {
#pragma unroll
                for (int k = 0; k < NC; ++k)
                    if (c + k < width) out[c + k] = x[k];
            }
        }
        if (norm != nullptr) {                                 // (kernel-uniform)
            s = wave_sum(s);
            if (lane == 0) norm[b] = sqrtf(s);
        }
    }
}

}  // namespace

int launch_export_rows(const void* src, int bf16, int64_t ld_src, int B, int width, float* dst, int64_t ld_dst, float* norm, hipStream_t s) {
    CODAE_REQUIRE(src != nullptr && dst != nullptr && src != (const void*)dst, "codae_export_rows: null or aliased src and dst");
    CODAE_REQUIRE(bf16 == 0 || bf16 == 1, "codae_export_rows: bf16 %d is neither 0 nor 1", bf16);
    CODAE_REQUIRE(B > 0 && width > 0 && ld_src >= width && ld_dst >= width, "codae_export_rows: B %d, width %d, ld_src %lld, ld_dst %lld", B, width,
                  (long long)ld_src, (long long)ld_dst);
    CODAE_REQUIRE(norm == nullptr || (const void*)norm != src, "codae_export_rows: norm aliases src");
    int blocks = (B + EXP_WAVES - 1) / EXP_WAVES;
    if (blocks > 4096) blocks = 4096;
    const bool vec = rows_vec16(bf16, width, {{src, ld_src}}) && aligned16(dst) && ld_dst % 4 == 0;
    dispatch_bf16_vec(bf16, vec, [&](auto BF, auto V) {
        hipLaunchKernelGGL((export_rows_kernel<decltype(BF)::value, decltype(V)::value>), dim3(blocks), dim3(EXP_NT), 0, s, src, ld_src, B, width, dst,
                           ld_dst, norm);
    });
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

}  // namespace codae
