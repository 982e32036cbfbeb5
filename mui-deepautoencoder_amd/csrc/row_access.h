// Row accessors shared by the streaming kernels that sit between a step's GEMMs (dropout.hip, residual.hip, norm.hip, codes.hip): C columns of a
// working-precision row widened to fp32 and back, templated on <BF16, VEC> - 16 B per access where every row is 16-B aligned and the
// width is whole chunks, element accesses otherwise; a column past the width is neither read nor written.
#pragma once
#include "codae_common.h"

namespace codae {
namespace {

// "> 0" of a stored value as the forward GEMM's 1-bit masks test it (gemm_bf16_pipe.hip, `pos` / `keep`): sign clear and
// magnitude not zero - a NaN with a clear sign counts as positive, one with the sign set does not.  A bf16 widened to fp32
// keeps both fields, so one form serves both types.
__device__ __forceinline__ uint32_t positive_bit(float v) {
    const uint32_t u = __float_as_uint(v);
    return ((u >> 31) == 0u && (u & 0x7fffffffu) != 0u) ? 1u : 0u;
}

// columns [c, c + C) of a working-precision row widened to fp32; 0 for a column past the width, which is not read
template <bool BF16, bool VEC, int C>
__device__ __forceinline__ void load_work(const void* row, int c, int width, float* v) {
    if constexpr (BF16 && VEC) {
        static_assert(C == 8, "one 16-B access is 8 bf16");
        const uint4 q = *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16_t*>(row) + c);
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[2 * k] = __uint_as_float(w[k] << 16);
            v[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
        }
    } else if constexpr (VEC) {
#pragma unroll
        for (int q = 0; q < C / 4; ++q) {
            float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c + 4 * q < width) f = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(row) + c + 4 * q);
            v[4 * q] = f.x; v[4 * q + 1] = f.y; v[4 * q + 2] = f.z; v[4 * q + 3] = f.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < C; ++k) {
            v[k] = 0.f;
            if (c + k < width) {
                if constexpr (BF16) v[k] = bf16_to_f32(reinterpret_cast<const bf16_t*>(row)[c + k]);
                else v[k] = reinterpret_cast<const float*>(row)[c + k];
            }
        }
    }
}

// columns [c, c + C) of a working-precision row <- v (bf16: round to nearest even); out[k] = the STORED value widened to fp32
// (0 for a column past the width, which is not written)
template <bool BF16, bool VEC, int C>
__device__ __forceinline__ void store_work(void* row, int c, int width, const float* v, float* out) {
    if constexpr (BF16 && VEC) {
        uint32_t o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o[k] = pack_bf16x2(v[2 * k], v[2 * k + 1]);
            out[2 * k] = __uint_as_float(o[k] << 16);
            out[2 * k + 1] = __uint_as_float(o[k] & 0xffff0000u);
        }
        *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(row) + c) = make_uint4(o[0], o[1], o[2], o[3]);
    } else if constexpr (VEC) {
#pragma unroll
        for (int q = 0; q < C / 4; ++q) {
            const bool in = c + 4 * q < width;
#pragma unroll
            for (int k = 0; k < 4; ++k) out[4 * q + k] = in ? v[4 * q + k] : 0.f;
            if (in) *reinterpret_cast<float4*>(reinterpret_cast<float*>(row) + c + 4 * q) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < C; ++k) {
            out[k] = 0.f;
            if (c + k < width) {
                if constexpr (BF16) {
                    const bf16_t o = f32_to_bf16(v[k]);
                    reinterpret_cast<bf16_t*>(row)[c + k] = o;
                    out[k] = bf16_to_f32(o);
                } else {
                    reinterpret_cast<float*>(row)[c + k] = v[k];
                    out[k] = v[k];
                }
            }
        }
    }
}

// The sum of the wave's 64 values: a butterfly.  a + b and b + a have the same bits, so after every stage the two partners hold
// the same value and the result does not depend on the lane; lane 0's copy is broadcast to say so.  (norm.hip, codes.hip)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = opaque(v + __shfl_xor(v, m, 64));
    return __shfl(v, 0, 64);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace
}  // namespace codae
