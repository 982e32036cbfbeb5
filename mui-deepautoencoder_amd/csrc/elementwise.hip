// HBM-bound pieces of the DAE step: batch gather + slot corruption, mask expansion,
// fused MSE loss forward/backward with the reference's per-step metrics, gradient norm,
// clip + Adam with bf16 shadow refresh.  All are single-pass, 16 B per lane where the
// row width allows, grid capped at 2048 blocks with a grid-stride loop.
#include "loss_sweep.h"

namespace codae {
namespace {

constexpr int NT = 256;
static_assert(NT == LOSS_NT, "loss_sweep strides the columns by LOSS_NT threads");

inline int grid_for(int64_t work_items) {
    int64_t b = (work_items + NT - 1) / NT;
    if (b < 1) b = 1;
    if (b > 2048) b = 2048;
    return (int)b;
}

// the gather's presence rule: exactly 0 in every column of an absent slot, behind the noise and the slot mask
template <int W>
__device__ __forceinline__ void zero_absent(float* v, const PresArgs& pa, int64_t row, int c) {
    int sl[W];
    slots_of<W>(c, pa.E, sl);
    const uint32_t pb = present_bits<W>(pa, row, sl);
#pragma unroll
    for (int k = 0; k < W; ++k) v[k] = ((pb >> k) & 1u) ? v[k] : 0.f;
}

// zero_norm != null (the fused step whose loss finish rides in the bias-finish launch): the launch's first block clears the
// clip_grad_norm_ accumulators - what finish_loss_kernel does in front of the backward when it runs as a launch of its own
__device__ __forceinline__ void zero_norm_scalars(double* zero_norm) {
    if (zero_norm != nullptr && blockIdx.x == 0) {
        if (threadIdx.x == 0) zero_norm[CODAE_S_GRAD_SQ] = 0.0;
        if (threadIdx.x < CODAE_S_N_SLOTS) zero_norm[CODAE_S_GRAD_SQ_SLOTS + threadIdx.x] = 0.0;
    }
}

// The training step's form of the kernel below (bf16 out, io % 8 == 0): 8 elements per thread = two 16-B loads, one
// 8-B mask load, one 16-B store (the 4-element form stores 8 B per lane, half-width store instructions).
// (Measured and dropped: whole rows per wave - 2 rows x up to 4 column chunks of 16-B loads in flight per lane, row index and mask
// id read once per row: 28.0 -> 27.1 us per launch on one box, 27.3 -> 27.8 on another: inside the noise)
template <bool PRES>
__global__ __launch_bounds__(NT) void gather_corrupt_bf16x8_kernel(const float* __restrict__ data,
                                                                   const int32_t* __restrict__ row_idx,
                                                                   const int32_t* __restrict__ mask_id,
                                                                   const uint8_t* __restrict__ table, int B, int io,
                                                                   bf16_t* __restrict__ out,
                                                                   const int32_t* __restrict__ mask_to_use, int nb_run,
                                                                   int run, int64_t out_ld, double* zero_norm, PresArgs pa) {
    zero_norm_scalars(zero_norm);
    const bool masked = (mask_id != nullptr) || (mask_to_use != nullptr);
    const int cols = io / 8;
    const int64_t total = (int64_t)B * cols;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < total; e += (int64_t)gridDim.x * NT) {
        const int b = (int)(e / cols);
        const int c = (int)(e - (int64_t)b * cols) * 8;
        const int64_t src_row = row_idx ? row_idx[b] : b;
        const float* src = data + src_row * io + c;
        const float4 x0 = *reinterpret_cast<const float4*>(src);
        const float4 x1 = *reinterpret_cast<const float4*>(src + 4);
        float v[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
        if (masked) {
            const int id = mask_id ? mask_id[b] : mask_to_use[src_row * nb_run + run];
            const uint2 m = *reinterpret_cast<const uint2*>(table + (int64_t)id * io + c);
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = (((k < 4 ? m.x : m.y) >> (8 * (k & 3))) & 0xff) ? v[k] : 0.f;
        }
        if constexpr (PRES) zero_absent<8>(v, pa, src_row, c);
        uint4 o;
        o.x = pack_bf16x2(v[0], v[1]); o.y = pack_bf16x2(v[2], v[3]);
        o.z = pack_bf16x2(v[4], v[5]); o.w = pack_bf16x2(v[6], v[7]);
        *reinterpret_cast<uint4*>(out + (int64_t)b * out_ld + c) = o;
    }
}

// 0xffff in the half of a packed bf16 pair whose mask byte (bits 0-7 / 8-15 of m2) is not zero
__device__ __forceinline__ uint32_t keep_pair(uint32_t m2) {
    return ((m2 & 0xffu) ? 0x0000ffffu : 0u) | ((m2 & 0xff00u) ? 0xffff0000u : 0u);
}

// The same rows from the dataset's resident bf16 image (codae_set_dataset_image: image[r][c] = bf16(data[r][c]), rounded as
// pack_bf16x2 rounds): rounding and then clearing gives the bits of clearing and then rounding, since a cleared element is +0
// either way.  Per thread 8 columns: the 8 mask bytes first - a group they blank altogether (the corrupted slot: a third of a
// C3 row) is stored as zeros and never loaded -, else ONE 16-B load, the masked and absent halves cleared by an AND on the
// packed pairs (a masked NaN or -0 comes out +0, as the select on the fp32 value leaves it), one 16-B store.
template <bool PRES>
__global__ __launch_bounds__(NT) void gather_corrupt_image_kernel(const bf16_t* __restrict__ image,
                                                                  const int32_t* __restrict__ row_idx,
                                                                  const int32_t* __restrict__ mask_id,
                                                                  const uint8_t* __restrict__ table, int B, int io,
                                                                  bf16_t* __restrict__ out,
                                                                  const int32_t* __restrict__ mask_to_use, int nb_run,
                                                                  int run, int64_t out_ld, double* zero_norm, PresArgs pa) {
    zero_norm_scalars(zero_norm);
    const bool masked = (mask_id != nullptr) || (mask_to_use != nullptr);
    const int cols = io / 8;
    const int64_t total = (int64_t)B * cols;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < total; e += (int64_t)gridDim.x * NT) {
        const int b = (int)(e / cols);
        const int c = (int)(e - (int64_t)b * cols) * 8;
        const int64_t src_row = row_idx ? row_idx[b] : b;
        uint4 keep = make_uint4(~0u, ~0u, ~0u, ~0u);
        if (masked) {
            const int id = mask_id ? mask_id[b] : mask_to_use[src_row * nb_run + run];
            const uint2 m = *reinterpret_cast<const uint2*>(table + (int64_t)id * io + c);
            keep = make_uint4(keep_pair(m.x), keep_pair(m.x >> 16), keep_pair(m.y), keep_pair(m.y >> 16));
        }
        if constexpr (PRES) {
            int sl[8];
            slots_of<8>(c, pa.E, sl);
            const uint32_t pb = present_bits<8>(pa, src_row, sl);
            keep.x &= ((pb & 1u) ? 0x0000ffffu : 0u) | ((pb & 2u) ? 0xffff0000u : 0u);
            keep.y &= ((pb & 4u) ? 0x0000ffffu : 0u) | ((pb & 8u) ? 0xffff0000u : 0u);
            keep.z &= ((pb & 16u) ? 0x0000ffffu : 0u) | ((pb & 32u) ? 0xffff0000u : 0u);
            keep.w &= ((pb & 64u) ? 0x0000ffffu : 0u) | ((pb & 128u) ? 0xffff0000u : 0u);
        }
        uint4 o = make_uint4(0u, 0u, 0u, 0u);
        if ((keep.x | keep.y | keep.z | keep.w) != 0u) {
            const uint4 x = *reinterpret_cast<const uint4*>(image + src_row * io + c);
            o = make_uint4(x.x & keep.x, x.y & keep.y, x.z & keep.z, x.w & keep.w);
        }
        *reinterpret_cast<uint4*>(out + (int64_t)b * out_ld + c) = o;
    }
}

// ---- a2 + a10: out[b][:] = data[row_idx[b]][:] * mask_table[mask_id[b]][:] -----------------
// (collate_embedding data_tool.py:96-103 + corrupt embedding_...py:226-239 fused; the [B,io]
// fp32 mask of Corrupter.get_masks is never materialised.)
template <bool VEC, bool OUT_BF16, bool PRES>
__global__ __launch_bounds__(NT) void gather_corrupt_kernel(const float* __restrict__ data,
                                                            const int32_t* __restrict__ row_idx,
                                                            const int32_t* __restrict__ mask_id,
                                                            const uint8_t* __restrict__ table, int B, int io,
                                                            void* __restrict__ out,
                                                            const int32_t* __restrict__ mask_to_use, int nb_run,
                                                            int run, int64_t out_ld, double* zero_norm, PresArgs pa) {
    zero_norm_scalars(zero_norm);
    constexpr int W = VEC ? 4 : 1;
    const bool masked = (mask_id != nullptr) || (mask_to_use != nullptr);
    const int cols = io / W;
    const int64_t total = (int64_t)B * cols;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < total; e += (int64_t)gridDim.x * NT) {
        const int b = (int)(e / cols);
        const int c = (int)(e - (int64_t)b * cols) * W;
        const int64_t src_row = row_idx ? row_idx[b] : b;
        const float* src = data + src_row * io + c;
        float v[4];
        if constexpr (VEC) {
            const float4 x = *reinterpret_cast<const float4*>(src);
            v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
            if (masked) {
                const int id = mask_id ? mask_id[b] : mask_to_use[src_row * nb_run + run];
                const uint32_t m = *reinterpret_cast<const uint32_t*>(table + (int64_t)id * io + c);
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = ((m >> (8 * k)) & 0xff) ? v[k] : 0.f;
            }
        } else {
            v[0] = src[0];
            if (masked) {
                const int id = mask_id ? mask_id[b] : mask_to_use[src_row * nb_run + run];
                v[0] = table[(int64_t)id * io + c] ? v[0] : 0.f;
            }
        }
        if constexpr (PRES) zero_absent<W>(v, pa, src_row, c);
        const int64_t o = (int64_t)b * out_ld + c;
        if constexpr (OUT_BF16) {
            bf16_t* op = reinterpret_cast<bf16_t*>(out) + o;
            if constexpr (VEC) *reinterpret_cast<uint2*>(op) = pack_bf16x4(v[0], v[1], v[2], v[3]);
            else op[0] = f32_to_bf16(v[0]);
        } else {
            float* op = reinterpret_cast<float*>(out) + o;
            if constexpr (VEC) *reinterpret_cast<float4*>(op) = make_float4(v[0], v[1], v[2], v[3]);
            else op[0] = v[0];
        }
    }
}

// ---- input noise (codae_noise, include/codae_hip.h): the noise-enabled forms of the three gather kernels above -------------
// Philox4x32-10 keyed by the seed, counter (column / 4, DATASET row, Adam step, 0): one call serves four columns, so a row's
// noise does not depend on where the row sits in the batch or on which rank.  Noise first, then the slot mask.
struct NoiseArgs {
    uint32_t key0, key1;       // seed & 0xffffffff, seed >> 32
    uint32_t step;             // counter word 2 ...
    const double* step_dev;    // ... or, when not null, *step_dev (graph replay)
    const int32_t* rows;       // not null: counter word 1 of batch row b is rows[b] (a batch gathered by the caller), else the row read
    uint64_t thresh;           // MASKING / SALT_PEPPER: T = floor(p 2^32)
    float p0, p1, p2;          // sigma; lo, hi
    double* zero_norm;         // see zero_norm_scalars
};

// Box-Muller pieces from one pair of words.  u1 in (0, 1] and 2 u2 in [0, 2) are exact in fp32; logf keeps its relative accuracy
// for u1 next to 1 (rho is a square root of it), sincospif reduces its argument exactly (tools/noise_accuracy.py: every one of
// the 2^24 values of u1 and of u2 against float64)
__device__ __forceinline__ void box_muller_parts(uint32_t ra, uint32_t rb, float& rho, float& c, float& sn) {
    const float u1 = (float)((ra >> 8) + 1u) * 5.9604644775390625e-8f;       // 2^-24
    const float two_u2 = (float)(rb >> 8) * 1.1920928955078125e-7f;          // 2^-23
    rho = sqrtf(-2.f * logf(u1));
    sincospif(two_u2, &sn, &c);
}

__device__ __forceinline__ float noise_elem(int kind_masking, uint32_t rk, float x, const NoiseArgs& a) {
    const bool hit = (uint64_t)rk < a.thresh;
    if (kind_masking) return hit ? 0.f : x;
    return hit ? ((uint64_t)rk < (a.thresh >> 1) ? a.p1 : a.p2) : x;
}

// v[0..4) = columns 4g .. 4g + 3 of one row <- noised values; r: the group's four words
template <int KIND>
__device__ __forceinline__ void noise_apply4(float* v, const uint4 r, const NoiseArgs& a) {
    if constexpr (KIND == CODAE_NOISE_GAUSSIAN) {
        float rho, c, sn;
        box_muller_parts(r.x, r.y, rho, c, sn);
        v[0] = fmaf(a.p0, rho * c, v[0]); v[1] = fmaf(a.p0, rho * sn, v[1]);
        box_muller_parts(r.z, r.w, rho, c, sn);
        v[2] = fmaf(a.p0, rho * c, v[2]); v[3] = fmaf(a.p0, rho * sn, v[3]);
    } else {
        constexpr int M = KIND == CODAE_NOISE_MASKING;
        v[0] = noise_elem(M, r.x, v[0], a); v[1] = noise_elem(M, r.y, v[1], a);
        v[2] = noise_elem(M, r.z, v[2], a); v[3] = noise_elem(M, r.w, v[3], a);
    }
}

// one column: word k = column % 4 of its group (selects, no indexed register array)
template <int KIND>
__device__ __forceinline__ float noise_apply1(float x, const uint4 r, int k, const NoiseArgs& a) {
    if constexpr (KIND == CODAE_NOISE_GAUSSIAN) {
        float rho, c, sn;
        box_muller_parts((k & 2) ? r.z : r.x, (k & 2) ? r.w : r.y, rho, c, sn);
        return fmaf(a.p0, rho * ((k & 1) ? sn : c), x);
    } else {
        const uint32_t rk = (k & 2) ? ((k & 1) ? r.w : r.z) : ((k & 1) ? r.y : r.x);
        return noise_elem(KIND == CODAE_NOISE_MASKING, rk, x, a);
    }
}

template <int KIND, bool PRES>
__global__ __launch_bounds__(NT) void gather_noise_bf16x8_kernel(const float* __restrict__ data, const int32_t* __restrict__ row_idx,
                                                                 const int32_t* __restrict__ mask_id, const uint8_t* __restrict__ table,
                                                                 int B, int io, bf16_t* __restrict__ out,
                                                                 const int32_t* __restrict__ mask_to_use, int nb_run, int run,
                                                                 int64_t out_ld, NoiseArgs na, PresArgs pa) {
    zero_norm_scalars(na.zero_norm);
    const bool masked = (mask_id != nullptr) || (mask_to_use != nullptr);
    const uint32_t step = na.step_dev ? (uint32_t)*na.step_dev : na.step;
    const int cols = io / 8;
    const int64_t total = (int64_t)B * cols;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < total; e += (int64_t)gridDim.x * NT) {
        const int b = (int)(e / cols);
        const int c = (int)(e - (int64_t)b * cols) * 8;
        const int64_t src_row = row_idx ? row_idx[b] : b;
        const float* src = data + src_row * io + c;
        const float4 x0 = *reinterpret_cast<const float4*>(src);
        const float4 x1 = *reinterpret_cast<const float4*>(src + 4);
        float v[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
        const uint32_t nrow = na.rows ? (uint32_t)na.rows[b] : (uint32_t)src_row;
        noise_apply4<KIND>(v, philox4x32_10((uint32_t)(c >> 2), nrow, step, 0u, na.key0, na.key1), na);
        noise_apply4<KIND>(v + 4, philox4x32_10((uint32_t)(c >> 2) + 1u, nrow, step, 0u, na.key0, na.key1), na);
        if (masked) {
            const int id = mask_id ? mask_id[b] : mask_to_use[src_row * nb_run + run];
            const uint2 m = *reinterpret_cast<const uint2*>(table + (int64_t)id * io + c);
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = (((k < 4 ? m.x : m.y) >> (8 * (k & 3))) & 0xff) ? v[k] : 0.f;
        }
        if constexpr (PRES) zero_absent<8>(v, pa, (int64_t)nrow, c);
        uint4 o;
        o.x = pack_bf16x2(v[0], v[1]); o.y = pack_bf16x2(v[2], v[3]);
        o.z = pack_bf16x2(v[4], v[5]); o.w = pack_bf16x2(v[6], v[7]);
        *reinterpret_cast<uint4*>(out + (int64_t)b * out_ld + c) = o;
    }
}

template <bool VEC, bool OUT_BF16, int KIND, bool PRES>
__global__ __launch_bounds__(NT) void gather_noise_kernel(const float* __restrict__ data, const int32_t* __restrict__ row_idx,
                                                          const int32_t* __restrict__ mask_id, const uint8_t* __restrict__ table, int B,
                                                          int io, void* __restrict__ out, const int32_t* __restrict__ mask_to_use,
                                                          int nb_run, int run, int64_t out_ld, NoiseArgs na, PresArgs pa) {
    zero_norm_scalars(na.zero_norm);
    constexpr int W = VEC ? 4 : 1;
    const bool masked = (mask_id != nullptr) || (mask_to_use != nullptr);
    const uint32_t step = na.step_dev ? (uint32_t)*na.step_dev : na.step;
    const int cols = io / W;
    const int64_t total = (int64_t)B * cols;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < total; e += (int64_t)gridDim.x * NT) {
        const int b = (int)(e / cols);
        const int c = (int)(e - (int64_t)b * cols) * W;
        const int64_t src_row = row_idx ? row_idx[b] : b;
        const float* src = data + src_row * io + c;
        const uint32_t nrow = na.rows ? (uint32_t)na.rows[b] : (uint32_t)src_row;
        const uint4 r = philox4x32_10((uint32_t)(c >> 2), nrow, step, 0u, na.key0, na.key1);
        float v[4];
        if constexpr (VEC) {
            const float4 x = *reinterpret_cast<const float4*>(src);
            v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
            noise_apply4<KIND>(v, r, na);
            if (masked) {
                const int id = mask_id ? mask_id[b] : mask_to_use[src_row * nb_run + run];
                const uint32_t m = *reinterpret_cast<const uint32_t*>(table + (int64_t)id * io + c);
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = ((m >> (8 * k)) & 0xff) ? v[k] : 0.f;
            }
        } else {
            v[0] = src[0];
            v[0] = noise_apply1<KIND>(v[0], r, c & 3, na);
            if (masked) {
                const int id = mask_id ? mask_id[b] : mask_to_use[src_row * nb_run + run];
                v[0] = table[(int64_t)id * io + c] ? v[0] : 0.f;
            }
        }
        if constexpr (PRES) zero_absent<W>(v, pa, (int64_t)nrow, c);
        const int64_t o = (int64_t)b * out_ld + c;
        if constexpr (OUT_BF16) {
            bf16_t* op = reinterpret_cast<bf16_t*>(out) + o;
            if constexpr (VEC) *reinterpret_cast<uint2*>(op) = pack_bf16x4(v[0], v[1], v[2], v[3]);
            else op[0] = f32_to_bf16(v[0]);
        } else {
            float* op = reinterpret_cast<float*>(out) + o;
            if constexpr (VEC) *reinterpret_cast<float4*>(op) = make_float4(v[0], v[1], v[2], v[3]);
            else op[0] = v[0];
        }
    }
}

__global__ __launch_bounds__(NT) void noise_box_muller_kernel(const uint32_t* __restrict__ ra, const uint32_t* __restrict__ rb,
                                                              float* __restrict__ rho, float* __restrict__ c, float* __restrict__ sn,
                                                              int64_t n) {
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT)
        box_muller_parts(ra[e], rb[e], rho[e], c[e], sn[e]);
}

__global__ __launch_bounds__(NT) void cast_bf16_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst,
                                                       int64_t n) {
    const int64_t n4 = n / 4;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n4; e += (int64_t)gridDim.x * NT) {
        const float4 x = reinterpret_cast<const float4*>(src)[e];
        reinterpret_cast<uint2*>(dst)[e] = pack_bf16x4(x.x, x.y, x.z, x.w);
    }
    for (int64_t e = n4 * 4 + (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT)
        dst[e] = f32_to_bf16(src[e]);
}

__global__ __launch_bounds__(NT) void cast_f32_kernel(const bf16_t* __restrict__ src, float* __restrict__ dst,
                                                      int64_t n) {
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT)
        dst[e] = bf16_to_f32(src[e]);
}

// model.corrupt on dense tensors: out = x * mask
__global__ __launch_bounds__(NT) void corrupt_kernel(const float* __restrict__ x, const float* __restrict__ m,
                                                     float* __restrict__ out, int64_t n) {
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT)
        out[e] = x[e] * m[e];
}

// Corrupter.get_masks (data_tool.py:252-262)
__global__ __launch_bounds__(NT) void expand_masks_kernel(const int32_t* __restrict__ mask_id,
                                                          const uint8_t* __restrict__ table,
                                                          const int32_t* __restrict__ k_of_mask, int B, int io,
                                                          int k_max, float* __restrict__ masks,
                                                          float* __restrict__ fmask) {
    const int64_t total = (int64_t)B * io;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < total; e += (int64_t)gridDim.x * NT) {
        const int b = (int)(e / io);
        const int c = (int)(e - (int64_t)b * io);
        const int id = mask_id[b];
        const float v = table[(int64_t)id * io + c] ? 1.f : 0.f;
        const int k = k_of_mask[id] - 1;
        for (int kk = 0; kk < k_max; ++kk) masks[(int64_t)kk * total + e] = (kk == k) ? v : 0.f;
        fmask[e] = v;
    }
}

// ---- a4 + a11: MSELoss(mean) forward/backward + the per-step metric sums --------------------
// One block owns ROWS consecutive batch rows and sweeps all columns; the bias gradient of the last
// Linear (column sums of dy) leaves as one partial-sum row per block (plain stores, added up in block
// order by bias_finish_kernel: deterministic).
//   dy = 2 (y - x) * inv_n                          (autograd of train_dae_on_embedding.py:206)
//   SQ_FULL    += sum (x-y)^2                        (:218-220)
//   SQ_PARTIAL += sum (1-fmask)(x-y)^2               (:223)
// The row sweep and the arithmetic (MseTerm) are loss_sweep.h's; parts[block] = { sq, sqp }
template <bool VEC, bool DY_BF16, bool PRES>
__global__ __launch_bounds__(NT) void mse_loss_kernel(const float* __restrict__ data,
                                                      const int32_t* __restrict__ row_idx,
                                                      const int32_t* __restrict__ mask_id,
                                                      const uint8_t* __restrict__ table, int B, int io,
                                                      const float* __restrict__ y, void* __restrict__ dy,
                                                      float inv_n, float* __restrict__ colsum_part,
                                                      double* __restrict__ loss_parts, int want_grad,
                                                      const int32_t* __restrict__ mask_to_use, int nb_run, int run, int64_t dy_ld,
                                                      PresArgs pa) {
    __shared__ float red[4];
    const bool masked = (mask_id != nullptr) || (mask_to_use != nullptr);
    const BatchArgs ba{data, row_idx, mask_id, table, mask_to_use, nb_run, run, B, io};
    MseTerm term(inv_n, want_grad);
    loss_sweep<VEC, DY_BF16, PRES>(ba, y, dy, dy_ld, colsum_part, pa, WeightArgs{}, term);
    const float bsq = block_sum(term.sq, red);
    const float bsqp = block_sum(term.sqp, red);
    if (threadIdx.x == 0) {
        loss_parts[2 * blockIdx.x] = (double)bsq;
        loss_parts[2 * blockIdx.x + 1] = masked ? (double)bsqp : 0.0;
    }
}

// ---- emphasised denoising loss (codae_emphasis, include/codae_hip.h; Vincent et al. 2010, section 4.3) ----------------------
// mse_loss_kernel's block shape with a weight per element (WeightArgs and EmphTerm, loss_sweep.h):
//   parts[block] = { sum w (x-y)^2, sum (x-y)^2, sum (1-fmask)(x-y)^2 }: the metric sums stay unweighted
template <bool VEC, bool DY_BF16, bool PRES>
__global__ __launch_bounds__(NT) void emph_loss_kernel(const float* __restrict__ data, const int32_t* __restrict__ row_idx,
                                                       const int32_t* __restrict__ mask_id, const uint8_t* __restrict__ table,
                                                       int B, int io, const float* __restrict__ y, void* __restrict__ dy,
                                                       float inv_n, float* __restrict__ colsum_part, double* __restrict__ parts,
                                                       const int32_t* __restrict__ mask_to_use, int nb_run, int run, int64_t dy_ld,
                                                       WeightArgs wa, PresArgs pa) {
    __shared__ float red[4];
    const bool masked = (mask_id != nullptr) || (mask_to_use != nullptr);
    const BatchArgs ba{data, row_idx, mask_id, table, mask_to_use, nb_run, run, B, io};
    EmphTerm term(wa, inv_n);
    loss_sweep<VEC, DY_BF16, PRES>(ba, y, dy, dy_ld, colsum_part, pa, wa, term);
    const float bwsq = block_sum(term.wsq, red);
    const float bsq = block_sum(term.sq, red);
    const float bsqp = block_sum(term.sqp, red);
    if (threadIdx.x == 0) {
        parts[3 * blockIdx.x] = (double)bwsq;
        parts[3 * blockIdx.x + 1] = (double)bsq;
        parts[3 * blockIdx.x + 2] = masked ? (double)bsqp : 0.0;
    }
}

// finish_loss_kernel for the three sums of emph_loss_kernel (added in index order: deterministic): LAST_LOSS = the weighted
// sum * inv_n, the epoch accumulators take the two unweighted sums; resets the per-step accumulators.  One block.
__global__ __launch_bounds__(NT) void finish_emph_loss_kernel(double* scalars, double inv_n, const double* __restrict__ parts,
                                                              int n_parts) {
    __shared__ double red[3][NT];
    double a[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < n_parts; i += NT) { a[0] += parts[3 * i]; a[1] += parts[3 * i + 1]; a[2] += parts[3 * i + 2]; }
    red[0][threadIdx.x] = a[0]; red[1][threadIdx.x] = a[1]; red[2][threadIdx.x] = a[2];
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o)
            for (int j = 0; j < 3; ++j) red[j][threadIdx.x] += red[j][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        scalars[CODAE_S_SQ_FULL] += red[1][0];
        scalars[CODAE_S_SQ_PARTIAL] += red[2][0];
        scalars[CODAE_S_LAST_LOSS] = red[0][0] * inv_n;
        scalars[CODAE_S_STEP_SQ] = 0.0;
        scalars[CODAE_S_GRAD_SQ] = 0.0;
    }
    if (threadIdx.x < CODAE_S_N_SLOTS) scalars[CODAE_S_GRAD_SQ_SLOTS + threadIdx.x] = 0.0;
}

// dense variant for the drop-in path (x, y, fmask already materialised)
__global__ __launch_bounds__(NT) void mse_dense_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                       const float* __restrict__ fmask, float* __restrict__ dy,
                                                       int64_t n, float inv_n, double* __restrict__ scalars) {
    __shared__ float red[4];
    float sq = 0.f, sqp = 0.f;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT) {
        const float d = x[e] - y[e];
        const float se = d * d;
        sq += se;
        if (fmask) sqp += (1.f - fmask[e]) * se;
        if (dy) dy[e] = -2.f * d * inv_n;
    }
    const float bsq = block_sum(sq, red);
    const float bsqp = block_sum(sqp, red);
    if (threadIdx.x == 0) {
        atomicAdd(&scalars[CODAE_S_SQ_FULL], (double)bsq);
        atomicAdd(&scalars[CODAE_S_STEP_SQ], (double)bsq);
        if (fmask) atomicAdd(&scalars[CODAE_S_SQ_PARTIAL], (double)bsqp);
    }
}

// Per-workgroup metric sums -> the epoch accumulators (added in index order: deterministic); LAST_LOSS = step sum * inv_n;
// reset the per-step accumulators.  One block.
__global__ __launch_bounds__(NT) void finish_loss_kernel(double* scalars, double inv_n, const double* __restrict__ parts,
                                                         int n_parts) {
    __shared__ double red[2][NT];
    if (parts != nullptr) {
        double a = 0.0, b = 0.0;
        for (int i = threadIdx.x; i < n_parts; i += NT) { a += parts[2 * i]; b += parts[2 * i + 1]; }
        red[0][threadIdx.x] = a; red[1][threadIdx.x] = b;
        __syncthreads();
        for (int o = NT / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) { red[0][threadIdx.x] += red[0][threadIdx.x + o]; red[1][threadIdx.x] += red[1][threadIdx.x + o]; }
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) {
        double step = scalars[CODAE_S_STEP_SQ];
        if (parts != nullptr) {
            step = red[0][0];
            scalars[CODAE_S_SQ_FULL] += red[0][0];
            scalars[CODAE_S_SQ_PARTIAL] += red[1][0];
        }
        scalars[CODAE_S_LAST_LOSS] = step * inv_n;
        scalars[CODAE_S_STEP_SQ] = 0.0;
        scalars[CODAE_S_GRAD_SQ] = 0.0;
    }
    if (threadIdx.x < CODAE_S_N_SLOTS) scalars[CODAE_S_GRAD_SQ_SLOTS + threadIdx.x] = 0.0;
}

// ---- a7: sum g^2 (clip_grad_norm_, train_dae_on_embedding.py:213) ---------------------------
__global__ __launch_bounds__(NT) void sumsq_kernel(const float* __restrict__ g, int64_t n, double* out) {
    __shared__ float red[4];
    float s = 0.f;
    const int64_t n4 = n / 4;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n4; e += (int64_t)gridDim.x * NT) {
        const float4 v = reinterpret_cast<const float4*>(g)[e];
        s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    for (int64_t e = n4 * 4 + (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT)
        s += g[e] * g[e];
    const float b = block_sum(s, red);
    // `out` points at scalars[GRAD_SQ]; scatter over the slot array that follows the named scalars
    if (threadIdx.x == 0)
        atomicAdd(out + (CODAE_S_GRAD_SQ_SLOTS - CODAE_S_GRAD_SQ) + (blockIdx.x & (CODAE_S_N_SLOTS - 1)), (double)b);
}

// *acc += sum g^2 with at most 64 blocks (a rank's parameter shard in the sharded update): one address, few adders
__global__ __launch_bounds__(NT) void sumsq_to_kernel(const float* __restrict__ g, int64_t n, double* acc) {
    __shared__ float red[4];
    float s = 0.f;
    const int64_t n4 = n / 4;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n4; e += (int64_t)gridDim.x * NT) {
        const float4 v = reinterpret_cast<const float4*>(g)[e];
        s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    for (int64_t e = n4 * 4 + (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT) s += g[e] * g[e];
    const float b = block_sum(s, red);
    if (threadIdx.x == 0) atomicAdd(acc, (double)b);
}

// clip_grad_norm_'s coefficient from a total sum g^2 (train_dae_on_embedding.py:213): min(1, max_norm / (norm + 1e-6))
// as torch.clamp(max=1): a NaN norm gives a NaN coefficient (fminf would give 1), an infinite one gives 0
__device__ __forceinline__ float clip_coef(float max_norm, float total) {
    const float r = max_norm / (total + 1e-6f);
    return r > 1.f ? 1.f : r;
}
__global__ void clip_coef_kernel(const double* total_sq, float max_norm, double* coef_out) {
    const float total = sqrtf((float)*total_sq);
    *coef_out = (double)clip_coef(max_norm, total);
}

// ---- a7 + a8: clip scale folded into Adam (torch.optim.Adam, amsgrad off, L2 decay) ----------
struct AdamConst {
    float lr_over_bc1, inv_sqrt_bc2, beta1, beta2, eps, wd, max_norm;
    float lr;                // graph replay: the bias corrections are rebuilt on the device from *step_dev
};

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float coef, const AdamConst& c) {
    g = g * coef + c.wd * p;
    m = c.beta1 * m + (1.f - c.beta1) * g;
    v = c.beta2 * v + (1.f - c.beta2) * g * g;
    const float denom = sqrtf(v) * c.inv_sqrt_bc2 + c.eps;
    p = p - c.lr_over_bc1 * (m / denom);
}

// ---- optimizer kinds and the learning-rate schedule (codae_optimizer, include/codae_hip.h) ----
// Both update kernels are templated on (KIND, AMS, SCHED); <CODAE_OPT_ADAM, false, false> is the code above, untouched.  Every other
// instantiation rebuilds lr_t and the bias corrections in its prologue, in double, from the step count - the kernel argument in a
// plain step, the device scalar under graph replay: the same code, so a replayed step has the bits of a plain one.
struct OptConst {
    float mu;                // SGD momentum
    int nesterov;
    int sched, warmup, total, period;
    float min_factor, gamma;
    int step;                // hyper->step (a plain step's t)
    float decay;             // ADAMW: lr_t wd, filled by the prologue
};

// f(t) of include/codae_hip.h ("Optimizer and schedule"), in double
__device__ __forceinline__ double lr_factor(const OptConst& o, double t) {
    const double W = (double)o.warmup;
    const double w = (o.warmup > 0 && t <= W) ? t / W : 1.0;
    double f = 1.0;
    if (o.sched == CODAE_SCHED_COSINE || o.sched == CODAE_SCHED_LINEAR) {
        double q = (t - W) / ((double)o.total - W);
        q = q < 0.0 ? 0.0 : (q > 1.0 ? 1.0 : q);
        const double mf = (double)o.min_factor;
        f = o.sched == CODAE_SCHED_COSINE ? mf + (1.0 - mf) * (1.0 + cos(M_PI * q)) / 2.0 : 1.0 - (1.0 - mf) * q;
    } else if (o.sched == CODAE_SCHED_STEP) {
        f = pow((double)o.gamma, floor((t - 1.0) / (double)o.period));
    }
    return w * f;
}

// c.lr <- lr_t, the bias-correction factors from it (ADAM / ADAMW), o.decay (ADAMW)
template <int KIND, bool SCHED>
__device__ __forceinline__ void opt_prologue(AdamConst& c, OptConst& o, const double* __restrict__ step_dev) {
    const double t = step_dev != nullptr ? *step_dev : (double)o.step;
    if constexpr (SCHED) c.lr = (float)((double)c.lr * lr_factor(o, t));
    if constexpr (KIND != CODAE_OPT_SGD) {
        c.lr_over_bc1 = (float)((double)c.lr / (1.0 - pow((double)c.beta1, t)));
        c.inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)c.beta2, t)));
    }
    o.decay = c.lr * c.wd;
}

template <int KIND, bool AMS>
__device__ __forceinline__ void opt_one(float& p, float g, float& m, float& v, float& vm, float coef, const AdamConst& c,
                                        const OptConst& o) {
    if constexpr (KIND == CODAE_OPT_SGD) {
        g = g * coef + c.wd * p;
        m = o.mu * m + g;
        const float u = o.nesterov ? g + o.mu * m : m;
        p = p - c.lr * u;
    } else if constexpr (KIND == CODAE_OPT_ADAM && !AMS) {
        adam_one(p, g, m, v, coef, c);
    } else {
        if constexpr (KIND == CODAE_OPT_ADAMW) { g = g * coef; p = p - o.decay * p; }     // p (1 - lr_t wd), rounded once at p's size
        else g = g * coef + c.wd * p;
        m = c.beta1 * m + (1.f - c.beta1) * g;
        v = c.beta2 * v + (1.f - c.beta2) * g * g;
        float d = v;
        if constexpr (AMS) { vm = (v > vm || v != v) ? v : vm; d = vm; }       // torch.maximum: a NaN on either side stays
        const float denom = sqrtf(d) * c.inv_sqrt_bc2 + c.eps;
        p = p - c.lr_over_bc1 * (m / denom);
    }
}

template <int KIND, bool AMS, bool SCHED>
__global__ __launch_bounds__(NT) void clip_adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                       float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                       AdamConst c, const double* __restrict__ grad_sq,
                                                       bf16_t* __restrict__ shadow, const double* __restrict__ coef_in,
                                                       const double* __restrict__ step_dev, float* __restrict__ vmax, OptConst o) {
    constexpr bool PLAIN = KIND == CODAE_OPT_ADAM && !AMS && !SCHED;
    constexpr bool HAS_V = KIND != CODAE_OPT_SGD;          // SGD neither reads nor writes v
    if constexpr (!PLAIN) {
        opt_prologue<KIND, SCHED>(c, o, step_dev);
    } else if (step_dev != nullptr) {
        // replayed from a hipGraph: the step count lives in device memory (kernel arguments are frozen at capture)
        const double t = *step_dev;
        c.lr_over_bc1 = (float)((double)c.lr / (1.0 - pow((double)c.beta1, t)));
        c.inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)c.beta2, t)));
    }
    float coef = 1.f;
    if (coef_in != nullptr) {
        coef = (float)(*coef_in);
    } else if (c.max_norm > 0.f) {
        // sum g^2 = scalars[GRAD_SQ] + its 64 partial slots (one wave adds them up, LDS broadcasts)
        __shared__ double total_sq;
        if (threadIdx.x < 64) {
            double v = grad_sq[(CODAE_S_GRAD_SQ_SLOTS - CODAE_S_GRAD_SQ) + threadIdx.x];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if (threadIdx.x == 0) total_sq = v + grad_sq[0];
        }
        __syncthreads();
        const float total = sqrtf((float)total_sq);
        coef = clip_coef(c.max_norm, total);
    }
    const int64_t n4 = n / 4;  // n is padded to a multiple of 64 by the engine; tail handled below anyway
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n4; e += (int64_t)gridDim.x * NT) {
        float4 pp = reinterpret_cast<float4*>(p)[e];
        const float4 gg = reinterpret_cast<const float4*>(g)[e];
        float4 mm = reinterpret_cast<float4*>(m)[e];
        float4 vv = make_float4(0.f, 0.f, 0.f, 0.f), xx = vv;
        if constexpr (HAS_V) vv = reinterpret_cast<float4*>(v)[e];
        if constexpr (AMS) xx = reinterpret_cast<float4*>(vmax)[e];
        opt_one<KIND, AMS>(pp.x, gg.x, mm.x, vv.x, xx.x, coef, c, o);
        opt_one<KIND, AMS>(pp.y, gg.y, mm.y, vv.y, xx.y, coef, c, o);
        opt_one<KIND, AMS>(pp.z, gg.z, mm.z, vv.z, xx.z, coef, c, o);
        opt_one<KIND, AMS>(pp.w, gg.w, mm.w, vv.w, xx.w, coef, c, o);
        reinterpret_cast<float4*>(p)[e] = pp;
        reinterpret_cast<float4*>(m)[e] = mm;
        if constexpr (HAS_V) reinterpret_cast<float4*>(v)[e] = vv;
        if constexpr (AMS) reinterpret_cast<float4*>(vmax)[e] = xx;
        if (shadow) reinterpret_cast<uint2*>(shadow)[e] = pack_bf16x4(pp.x, pp.y, pp.z, pp.w);
    }
    for (int64_t e = n4 * 4 + (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT) {
        float pp = p[e], mm = m[e], vv = 0.f, xx = 0.f;
        if constexpr (HAS_V) vv = v[e];
        if constexpr (AMS) xx = vmax[e];
        opt_one<KIND, AMS>(pp, g[e], mm, vv, xx, coef, c, o);
        p[e] = pp; m[e] = mm;
        if constexpr (HAS_V) v[e] = vv;
        if constexpr (AMS) vmax[e] = xx;
        if (shadow) shadow[e] = f32_to_bf16(pp);
    }
}

// out[i] = sum_s slabs[s][i]  (split-K partials of the weight-gradient GEMM); optionally also
// sumsq += sum out[i]^2 so that clip_grad_norm_ needs no second pass over the gradient
__global__ __launch_bounds__(NT) void reduce_slabs_kernel(const float* __restrict__ slabs, int n_slabs,
                                                          int64_t stride, float* __restrict__ out, int64_t n,
                                                          double* __restrict__ sumsq) {
    __shared__ float red[4];
    float sq = 0.f;
    const int64_t n4 = n / 4;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n4; e += (int64_t)gridDim.x * NT) {
        float4 a = reinterpret_cast<const float4*>(slabs)[e];
        for (int s = 1; s < n_slabs; ++s) {
            const float4 b = reinterpret_cast<const float4*>(slabs + s * stride)[e];
            a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        }
        reinterpret_cast<float4*>(out)[e] = a;
        sq += a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w;
    }
    for (int64_t e = n4 * 4 + (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT) {
        float a = slabs[e];
        for (int s = 1; s < n_slabs; ++s) a += slabs[s * stride + e];
        out[e] = a;
        sq += a * a;
    }
    if (sumsq != nullptr) {
        const float bsq = block_sum(sq, red);
        if (threadIdx.x == 0)
            atomicAdd(sumsq + (CODAE_S_GRAD_SQ_SLOTS - CODAE_S_GRAD_SQ) + (blockIdx.x & (CODAE_S_N_SLOTS - 1)), (double)bsq);
    }
}


// Split-K fp32 GEMM, second stage WITH the GEMM's epilogue (exact-fp32 forward / data-gradient launches of a small batch:
// 128 rows of a 1536-wide layer are 12 workgroups walking 48 K-tiles each - 124 / 178 us per launch; split over K they
// fill the chip and this kernel finishes them): C[i][j] = epi(sum_z slabs[z][i][j]), epi = + bias, ReLU, * [relu_src > 0];
// colsum_part[i / 64][j] = sum of the stored values over the block's 64 rows (the next bias gradient's partial rows, as
// gemm_f32 writes them).  One workgroup = 64 rows x 64 columns: thread -> 4 columns x 4 rows (16 apart).
// ACT: the generic-activation epilogue (GemmF32::act: act_fwd, or times act_dy_from_y(relu_src)); false: the ReLU / identity code
template <bool ACT = false>
__global__ __launch_bounds__(NT) void reduce_slabs_epi_kernel(const float* __restrict__ slabs, int n_slabs, int64_t stride, int M, int N,
                                                              float* __restrict__ C, int64_t ldc, const float* __restrict__ bias, int relu,
                                                              const float* __restrict__ relu_src, int64_t ld_relu,
                                                              float* __restrict__ colsum_part, int act, float p0, float p1, float p2) {
    __shared__ float red[16][64 + 4];
    const int cg = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const int j = blockIdx.x * 64 + cg * 4;
    const int i0 = blockIdx.y * 64;
    float cs[4] = {0.f, 0.f, 0.f, 0.f};
    if (j < N) {                                               // (N % 4 == 0: checked by the launcher)
        float4 bj = make_float4(0.f, 0.f, 0.f, 0.f);
        if (bias != nullptr) bj = *reinterpret_cast<const float4*>(bias + j);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + rg + 16 * q;
            if (i >= M) break;
            float4 a = *reinterpret_cast<const float4*>(slabs + (int64_t)i * N + j);
            for (int z = 1; z < n_slabs; ++z) {
                const float4 b = *reinterpret_cast<const float4*>(slabs + z * stride + (int64_t)i * N + j);
                a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
            }
            a.x += bj.x; a.y += bj.y; a.z += bj.z; a.w += bj.w;
            if constexpr (ACT) {
                const float p[3] = {p0, p1, p2};
                if (relu_src != nullptr) {
                    const float4 h = *reinterpret_cast<const float4*>(relu_src + (int64_t)i * ld_relu + j);
                    a.x = act_bwd(act, p, a.x, h.x); a.y = act_bwd(act, p, a.y, h.y);
                    a.z = act_bwd(act, p, a.z, h.z); a.w = act_bwd(act, p, a.w, h.w);
                } else {
                    a.x = act_fwd(act, p, a.x); a.y = act_fwd(act, p, a.y); a.z = act_fwd(act, p, a.z); a.w = act_fwd(act, p, a.w);
                }
            } else {
                if (relu) { a.x = clamp_below(a.x, 0.f); a.y = clamp_below(a.y, 0.f); a.z = clamp_below(a.z, 0.f); a.w = clamp_below(a.w, 0.f); }
                if (relu_src != nullptr) {
                    const float4 h = *reinterpret_cast<const float4*>(relu_src + (int64_t)i * ld_relu + j);
                    a.x = h.x > 0.f ? a.x : 0.f; a.y = h.y > 0.f ? a.y : 0.f; a.z = h.z > 0.f ? a.z : 0.f; a.w = h.w > 0.f ? a.w : 0.f;
                }
            }
            *reinterpret_cast<float4*>(C + (int64_t)i * ldc + j) = a;
            cs[0] += a.x; cs[1] += a.y; cs[2] += a.z; cs[3] += a.w;
        }
    }
    if (colsum_part != nullptr) {
        red[rg][cg * 4 + 0] = cs[0]; red[rg][cg * 4 + 1] = cs[1]; red[rg][cg * 4 + 2] = cs[2]; red[rg][cg * 4 + 3] = cs[3];
        __syncthreads();
        if (threadIdx.x < 64 && blockIdx.x * 64 + (int)threadIdx.x < N) {
            float t = 0.f;
            for (int r = 0; r < 16; ++r) t += red[r][threadIdx.x];
            colsum_part[(int64_t)blockIdx.y * N + blockIdx.x * 64 + threadIdx.x] = t;
        }
    }
}

// parts[block][c] = sum over the block's 64 rows of src[r][c]   (bias gradient of a dense dy, first stage)
// grid (row blocks, column chunks of NT): 8 row loads in flight per thread, added in row order (the same bits as a plain loop:
// that form - 128 blocks walking 64 dependent loads each - took 94 us for the 50 MB dy of the drop-in backward at C3)
__global__ __launch_bounds__(NT) void colsum_parts_f32_kernel(const float* __restrict__ src, int M, int N,
                                                              float* __restrict__ parts) {
    const int r_begin = blockIdx.x * 64;
    const int r_end = min(M, r_begin + 64);
    const int c = blockIdx.y * NT + threadIdx.x;
    if (c >= N) return;
    float s = 0.f;
    for (int r0 = r_begin; r0 < r_end; r0 += 8) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = src[(int64_t)min(r0 + k, r_end - 1) * N + c];
#pragma unroll
        for (int k = 0; k < 8; ++k) s += (r0 + k < r_end) ? v[k] : 0.f;
    }
    parts[(int64_t)blockIdx.x * N + c] = s;
}

// out[c] = sum_r src[r][c], rows in index order, one thread per column (stand-alone primitive: small problems)
__global__ __launch_bounds__(NT) void colsum_f32_kernel(const float* __restrict__ src, int M, int N,
                                                        float* __restrict__ out) {
    const int c = blockIdx.x * NT + threadIdx.x;
    if (c >= N) return;
    float s = 0.f;
    for (int r = 0; r < M; ++r) s += src[(int64_t)r * N + c];
    out[c] = s;
}

// Second stage of every bias gradient (and the deterministic replacement of round 1's float atomics): job j's
// out[c] = parts[0][c] + parts[1][c] + ... in row order; optionally sum out^2 for clip_grad_norm_.
__global__ __launch_bounds__(NT) void bias_finish_kernel(BiasFinishJobs jobs, double* __restrict__ sumsq, LossFinish lf) {
    __shared__ float red[4];
    if (lf.scalars != nullptr && blockIdx.x == gridDim.x - 1) {          // the extra block: metric sums of the step
        __shared__ double lred[2][NT];
        double a = 0.0, b = 0.0;
        for (int i = threadIdx.x; i < lf.n_parts; i += NT) { a += lf.parts[2 * i]; b += lf.parts[2 * i + 1]; }
        lred[0][threadIdx.x] = a; lred[1][threadIdx.x] = b;
        __syncthreads();
        for (int o = NT / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) { lred[0][threadIdx.x] += lred[0][threadIdx.x + o]; lred[1][threadIdx.x] += lred[1][threadIdx.x + o]; }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            lf.scalars[CODAE_S_SQ_FULL] += lred[0][0];
            lf.scalars[CODAE_S_SQ_PARTIAL] += lred[1][0];
            lf.scalars[CODAE_S_LAST_LOSS] = lred[0][0] * lf.inv_n;
            lf.scalars[CODAE_S_STEP_SQ] = 0.0;
        }
        return;
    }
    const int gc = blockIdx.x * NT + threadIdx.x;            // column in the concatenation of all jobs
    float sq = 0.f;
    if (gc < jobs.col_begin[jobs.n]) {
        int j = 0;
        while (j + 1 < jobs.n && gc >= jobs.col_begin[j + 1]) ++j;
        const int c = gc - jobs.col_begin[j];
        const int N = jobs.cols[j], R = jobs.rows[j];
        const float* p = jobs.parts[j] + c;
        float s = 0.f;
        int r = 0;
        for (; r + 32 <= R; r += 32) {              // 32 independent loads in flight (C3: all of a column's rows in ONE trip to
            float v[32];                             // memory; 8 at a time was four dependent trips, 9.5 us), added in row order
#pragma unroll
            for (int u = 0; u < 32; ++u) v[u] = p[(int64_t)(r + u) * N];
#pragma unroll
            for (int u = 0; u < 32; ++u) s += v[u];
        }
        for (; r + 8 <= R; r += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = p[(int64_t)(r + u) * N];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; r < R; ++r) s += p[(int64_t)r * N];
        jobs.out[j][c] = s;
        sq = s * s;
    }
    if (sumsq != nullptr) {
        const float bsq = block_sum(sq, red);
        if (threadIdx.x == 0)
            atomicAdd(sumsq + (CODAE_S_GRAD_SQ_SLOTS - CODAE_S_GRAD_SQ) + (blockIdx.x & (CODAE_S_N_SLOTS - 1)), (double)bsq);
    }
}

// dst[c][r] = src[r][c] for up to 64 bf16 matrices in one launch (the transposed weight shadows);
// 64 x 64 tiles through LDS, 16-byte global accesses on both sides
struct TransposeJobs {
    int n;
    int64_t off[64];        // element offset of the matrix in src and dst
    int rows[64], cols[64]; // src is [rows][cols]
    int tile_begin[65];     // prefix sum of tiles per matrix
};
__global__ __launch_bounds__(NT) void transpose_bf16_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst,
                                                            TransposeJobs jobs) {
    __shared__ bf16_t tile[64][72];          // 72: rows stay 16-byte aligned, banks staggered
    int m = 0;
    while (m + 1 < jobs.n && (int)blockIdx.x >= jobs.tile_begin[m + 1]) ++m;
    const int t = blockIdx.x - jobs.tile_begin[m];
    const int R = jobs.rows[m], C = jobs.cols[m];
    const int tiles_c = (C + 63) / 64;
    const int r0 = (t / tiles_c) * 64, c0 = (t % tiles_c) * 64;
    const bf16_t* S = src + jobs.off[m];
    bf16_t* D = dst + jobs.off[m];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int q = threadIdx.x + p * NT;      // 512 chunks of 8 elements
        const int r = q >> 3, c8 = (q & 7) * 8;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (r0 + r < R && c0 + c8 < C) v = *reinterpret_cast<const uint4*>(S + (int64_t)(r0 + r) * C + c0 + c8);
        *reinterpret_cast<uint4*>(&tile[r][c8]) = v;
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int q = threadIdx.x + p * NT;
        const int c = q >> 3, r8 = (q & 7) * 8;  // output row c (a source column), 8 source rows r8..r8+7
        if (c0 + c < C && r0 + r8 < R) {
            bf16_t e[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) e[k] = tile[r8 + k][c];
            uint4 v;
            v.x = (uint32_t)e[0] | ((uint32_t)e[1] << 16); v.y = (uint32_t)e[2] | ((uint32_t)e[3] << 16);
            v.z = (uint32_t)e[4] | ((uint32_t)e[5] << 16); v.w = (uint32_t)e[6] | ((uint32_t)e[7] << 16);
            *reinterpret_cast<uint4*>(D + (int64_t)(c0 + c) * R + r0 + r8) = v;
        }
    }
}

}  // namespace

int check_presence(const uint8_t* present, int n_slots, int io, const char* who) {
    if (present == nullptr) return CODAE_OK;
    CODAE_REQUIRE(n_slots >= 1 && n_slots <= 128, "%s: slot presence takes 1 .. 128 slots, got %d", who, n_slots);
    CODAE_REQUIRE(io > 0 && io % n_slots == 0, "%s: slot presence: n_slots %d does not divide io %d", who, n_slots, io);
    return CODAE_OK;
}

int launch_gather_corrupt(const codae_batch* b, void* out, int out_bf16, hipStream_t s, int64_t out_ld, double* zero_norm,
                          const uint8_t* present, int n_slots) {
    if (out_ld <= 0) out_ld = b ? b->io : 0;
    CODAE_REQUIRE(b && b->data && out && b->B > 0 && b->io > 0, "gather_corrupt: bad batch");
    int prc = check_presence(present, n_slots, b->io, "gather_corrupt");
    if (prc) return prc;
    const PresArgs pa{present, n_slots, present ? b->io / n_slots : 0};
    const bool masked = b->mask_id || b->mask_to_use;
    CODAE_REQUIRE(!masked || b->mask_table, "gather_corrupt: mask ids without mask_table");
    CODAE_REQUIRE(!b->mask_to_use || b->mask_id || (b->nb_run > 0 && b->run >= 0 && b->run < b->nb_run),
                  "gather_corrupt: run %d outside [0, %d)", b->run, b->nb_run);
    const bool vec = (b->io % 4 == 0) && (out_ld % 4 == 0) && a16(b->data) && a16(out) && (!masked || (reinterpret_cast<uintptr_t>(b->mask_table) & 3) == 0);
    const int64_t items = (int64_t)b->B * (vec ? b->io / 4 : b->io);
    const int grid = grid_for(items);
    if (vec && out_bf16 && b->io % 8 == 0 && (!masked || (reinterpret_cast<uintptr_t>(b->mask_table) & 7) == 0)) {
#define GC8(P) hipLaunchKernelGGL((gather_corrupt_bf16x8_kernel<P>), dim3(grid_for(items / 2)), dim3(NT), 0, s, b->data, b->row_idx, b->mask_id, \
                                  b->mask_table, b->B, b->io, reinterpret_cast<bf16_t*>(out), b->mask_to_use, b->nb_run, b->run, out_ld, zero_norm, pa)
        if (present) GC8(true);
        else GC8(false);
#undef GC8
        CODAE_LAUNCH_CHECK();
        return CODAE_OK;
    }
#define GCP(V, O, P) hipLaunchKernelGGL((gather_corrupt_kernel<V, O, P>), dim3(grid), dim3(NT), 0, s, b->data, b->row_idx, \
                                    b->mask_id, b->mask_table, b->B, b->io, out, b->mask_to_use, b->nb_run, b->run, out_ld, zero_norm, pa)
#define GC(V, O) do { if (present) GCP(V, O, true); else GCP(V, O, false); } while (0)
    if (vec && out_bf16) GC(true, true);
    else if (vec) GC(true, false);
    else if (out_bf16) GC(false, true);
    else GC(false, false);
#undef GC
#undef GCP
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

bool gather_image_takes(const codae_batch* b, const void* image, const void* out, int64_t out_ld) {
    if (b == nullptr || image == nullptr || out == nullptr || b->io <= 0 || b->io % 8 != 0) return false;
    if (out_ld <= 0) out_ld = b->io;
    const bool masked = b->mask_id || b->mask_to_use;
    return out_ld % 8 == 0 && a16(image) && a16(out) && (!masked || (reinterpret_cast<uintptr_t>(b->mask_table) & 7) == 0);
}

int launch_gather_image(const codae_batch* b, const bf16_t* image, bf16_t* out, hipStream_t s, int64_t out_ld, double* zero_norm,
                        const uint8_t* present, int n_slots) {
    if (out_ld <= 0) out_ld = b ? b->io : 0;
    CODAE_REQUIRE(b && image && out && b->B > 0 && b->io > 0, "gather_image: bad batch");
    int prc = check_presence(present, n_slots, b->io, "gather_image");
    if (prc) return prc;
    const PresArgs pa{present, n_slots, present ? b->io / n_slots : 0};
    const bool masked = b->mask_id || b->mask_to_use;
    CODAE_REQUIRE(!masked || b->mask_table, "gather_image: mask ids without mask_table");
    CODAE_REQUIRE(!b->mask_to_use || b->mask_id || (b->nb_run > 0 && b->run >= 0 && b->run < b->nb_run),
                  "gather_image: run %d outside [0, %d)", b->run, b->nb_run);
    CODAE_REQUIRE(gather_image_takes(b, image, out, out_ld),
                  "gather_image: io %d and out_ld %lld must be multiples of 8, image and out 16-byte and mask_table 8-byte aligned", b->io,
                  (long long)out_ld);
    const int grid = grid_for((int64_t)b->B * (b->io / 8));
#define GCI(P) hipLaunchKernelGGL((gather_corrupt_image_kernel<P>), dim3(grid), dim3(NT), 0, s, image, b->row_idx, b->mask_id, b->mask_table, \
                                  b->B, b->io, out, b->mask_to_use, b->nb_run, b->run, out_ld, zero_norm, pa)
    if (present) GCI(true);
    else GCI(false);
#undef GCI
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int check_noise(const codae_noise* n) {
    if (n == nullptr || n->kind == CODAE_NOISE_NONE) return CODAE_OK;
    CODAE_REQUIRE(n->kind == CODAE_NOISE_GAUSSIAN || n->kind == CODAE_NOISE_MASKING || n->kind == CODAE_NOISE_SALT_PEPPER,
                  "input noise: unknown kind %d", n->kind);
    if (n->kind == CODAE_NOISE_GAUSSIAN) {
        CODAE_REQUIRE(finite_f(n->p0) && n->p0 >= 0.f, "input noise: sigma %g must be finite and >= 0", (double)n->p0);
        return CODAE_OK;
    }
    CODAE_REQUIRE(finite_f(n->p0) && n->p0 >= 0.f && n->p0 <= 1.f, "input noise: p %g outside [0, 1]", (double)n->p0);
    if (n->kind == CODAE_NOISE_SALT_PEPPER) {
        CODAE_REQUIRE(finite_f(n->p1), "input noise: lo %g is not finite", (double)n->p1);
        CODAE_REQUIRE(finite_f(n->p2), "input noise: hi %g is not finite", (double)n->p2);
    }
    return CODAE_OK;
}

int launch_gather_noise(const codae_batch* b, const codae_noise* noise, int32_t step, const double* step_dev, void* out, int out_bf16,
                        hipStream_t s, int64_t out_ld, const int32_t* noise_rows, double* zero_norm, const uint8_t* present, int n_slots) {
    if (noise == nullptr || noise->kind == CODAE_NOISE_NONE) {
        // (the plain gather keys the table by the row it reads: a batch gathered by the caller has lost its dataset rows)
        CODAE_REQUIRE(present == nullptr || noise_rows == nullptr, "gather_corrupt: a presence table with noise_rows needs an input noise kind");
        return launch_gather_corrupt(b, out, out_bf16, s, out_ld, zero_norm, present, n_slots);
    }
    int rc = check_noise(noise);
    if (rc) return rc;
    rc = check_presence(present, n_slots, b ? b->io : 0, "gather_corrupt");
    if (rc) return rc;
    const PresArgs pa{present, n_slots, present ? b->io / n_slots : 0};
    if (out_ld <= 0) out_ld = b ? b->io : 0;
    CODAE_REQUIRE(b && b->data && out && b->B > 0 && b->io > 0, "gather_corrupt: bad batch");
    const bool masked = b->mask_id || b->mask_to_use;
    CODAE_REQUIRE(!masked || b->mask_table, "gather_corrupt: mask ids without mask_table");
    CODAE_REQUIRE(!b->mask_to_use || b->mask_id || (b->nb_run > 0 && b->run >= 0 && b->run < b->nb_run),
                  "gather_corrupt: run %d outside [0, %d)", b->run, b->nb_run);
    NoiseArgs na{};
    na.key0 = (uint32_t)(noise->seed & 0xffffffffu); na.key1 = (uint32_t)(noise->seed >> 32);
    na.step = (uint32_t)step; na.step_dev = step_dev; na.rows = noise_rows; na.zero_norm = zero_norm;
    na.thresh = (uint64_t)floor((double)noise->p0 * 4294967296.0);      // (p <= 1: at most 2^32, above every word)
    na.p0 = noise->p0; na.p1 = noise->p1; na.p2 = noise->p2;
    const bool vec = (b->io % 4 == 0) && (out_ld % 4 == 0) && a16(b->data) && a16(out) && (!masked || (reinterpret_cast<uintptr_t>(b->mask_table) & 3) == 0);
    const int64_t items = (int64_t)b->B * (vec ? b->io / 4 : b->io);
    const int grid = grid_for(items);
    const bool x8 = vec && out_bf16 && b->io % 8 == 0 && (!masked || (reinterpret_cast<uintptr_t>(b->mask_table) & 7) == 0);
#define GN8P(K, P) hipLaunchKernelGGL((gather_noise_bf16x8_kernel<K, P>), dim3(grid_for(items / 2)), dim3(NT), 0, s, b->data, b->row_idx, b->mask_id, \
                                  b->mask_table, b->B, b->io, reinterpret_cast<bf16_t*>(out), b->mask_to_use, b->nb_run, b->run, out_ld, na, pa)
#define GNP(V, O, K, P) hipLaunchKernelGGL((gather_noise_kernel<V, O, K, P>), dim3(grid), dim3(NT), 0, s, b->data, b->row_idx, b->mask_id, \
                                       b->mask_table, b->B, b->io, out, b->mask_to_use, b->nb_run, b->run, out_ld, na, pa)
#define GN8(K) do { if (present) GN8P(K, true); else GN8P(K, false); } while (0)
#define GN(V, O, K) do { if (present) GNP(V, O, K, true); else GNP(V, O, K, false); } while (0)
#define GN_KIND(K)                           \
    do {                                     \
        if (x8) GN8(K);                      \
        else if (vec && out_bf16) GN(true, true, K);  \
        else if (vec) GN(true, false, K);    \
        else if (out_bf16) GN(false, true, K);        \
        else GN(false, false, K);            \
    } while (0)
    if (noise->kind == CODAE_NOISE_GAUSSIAN) GN_KIND(CODAE_NOISE_GAUSSIAN);
    else if (noise->kind == CODAE_NOISE_MASKING) GN_KIND(CODAE_NOISE_MASKING);
    else GN_KIND(CODAE_NOISE_SALT_PEPPER);
#undef GN_KIND
#undef GN
#undef GN8
#undef GNP
#undef GN8P
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_noise_box_muller(const uint32_t* ra, const uint32_t* rb, float* rho, float* c, float* sn, int64_t n, hipStream_t s) {
    CODAE_REQUIRE(ra && rb && rho && c && sn && n > 0, "noise_box_muller: bad args");
    hipLaunchKernelGGL(noise_box_muller_kernel, dim3(grid_for(n)), dim3(NT), 0, s, ra, rb, rho, c, sn, n);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_cast_bf16(const float* src, bf16_t* dst, int64_t n, hipStream_t s) {
    CODAE_REQUIRE(src && dst && n > 0 && a16(src) && (reinterpret_cast<uintptr_t>(dst) & 7) == 0, "cast: bad args");
    hipLaunchKernelGGL(cast_bf16_kernel, dim3(grid_for(n / 4 + 1)), dim3(NT), 0, s, src, dst, n);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_cast_f32(const bf16_t* src, float* dst, int64_t n, hipStream_t s) {
    CODAE_REQUIRE(src && dst && n > 0, "cast: bad args");
    hipLaunchKernelGGL(cast_f32_kernel, dim3(grid_for(n)), dim3(NT), 0, s, src, dst, n);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_corrupt(const float* x, const float* mask, float* out, int64_t n, hipStream_t s) {
    CODAE_REQUIRE(x && mask && out && n > 0, "corrupt: bad args");
    hipLaunchKernelGGL(corrupt_kernel, dim3(grid_for(n)), dim3(NT), 0, s, x, mask, out, n);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_expand_masks(const int32_t* mask_id, const uint8_t* table, const int32_t* k_of_mask, int B, int io,
                        int k_max, float* masks_out, float* fmask_out, hipStream_t s) {
    CODAE_REQUIRE(mask_id && table && k_of_mask && masks_out && fmask_out && B > 0 && io > 0 && k_max > 0,
                  "expand_masks: bad args");
    hipLaunchKernelGGL(expand_masks_kernel, dim3(grid_for((int64_t)B * io)), dim3(NT), 0, s, mask_id, table,
                       k_of_mask, B, io, k_max, masks_out, fmask_out);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int mse_loss_colsum_rows(int B) { return (B + LOSS_ROWS - 1) / LOSS_ROWS; }

int check_loss_launch(const char* who, const LossLaunch& ll, bool needs_dy) {
    const codae_batch* b = ll.batch;
    CODAE_REQUIRE(b && b->data && ll.y && ll.parts && (ll.dy || !needs_dy) && b->B > 0 && b->io > 0, "%s: bad args", who);
    int rc = check_presence(ll.present, ll.n_slots, b->io, who);
    if (rc) return rc;
    rc = check_emphasis(ll.emph);
    if (rc) return rc;
    rc = check_noise(ll.noise);
    if (rc) return rc;
    const bool masked = b->mask_id || b->mask_to_use;
    CODAE_REQUIRE(!masked || b->mask_table, "%s: mask ids without mask_table", who);
    if (!needs_dy) return CODAE_OK;      // (a launch that may run for its sums alone takes dy's stride and the run as they come)
    CODAE_REQUIRE(loss_dy_ld(ll) >= b->io, "%s: dy_ld %lld below io %d", who, (long long)loss_dy_ld(ll), b->io);
    CODAE_REQUIRE(!b->mask_to_use || b->mask_id || (b->nb_run > 0 && b->run >= 0 && b->run < b->nb_run),
                  "%s: run %d outside [0, %d)", who, b->run, b->nb_run);
    return CODAE_OK;
}

int launch_mse_loss(const LossLaunch& ll, int want_grad, hipStream_t s) {
    int rc = check_loss_launch("mse_loss", ll, false);
    if (rc) return rc;
    CODAE_REQUIRE(!want_grad || ll.dy, "mse_loss: gradient requested without dy");
    const codae_batch* b = ll.batch;
    const int64_t dy_ld = loss_dy_ld(ll);
    const bool vec = (b->io % 4 == 0) && (dy_ld % 4 == 0) && loss_inputs_a16(ll) && (!ll.dy || a16(ll.dy));
    const dim3 grid(mse_loss_colsum_rows(b->B));
    loss_dispatch(vec, ll.dy_bf16, ll.present != nullptr, [&](auto V, auto O, auto P) {
        hipLaunchKernelGGL((mse_loss_kernel<decltype(V)::value, decltype(O)::value, decltype(P)::value>), grid, dim3(NT), 0, s, b->data,
                           b->row_idx, b->mask_id, b->mask_table, b->B, b->io, ll.y, ll.dy, ll.scale, ll.colsum_part, ll.parts, want_grad,
                           b->mask_to_use, b->nb_run, b->run, dy_ld, pres_args(ll));
    });
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int check_emphasis(const codae_emphasis* e) {
    if (e == nullptr) return CODAE_OK;
    CODAE_REQUIRE(finite_f(e->alpha) && e->alpha >= 0.f, "loss emphasis: alpha %g must be finite and >= 0", (double)e->alpha);
    CODAE_REQUIRE(finite_f(e->beta) && e->beta >= 0.f, "loss emphasis: beta %g must be finite and >= 0", (double)e->beta);
    return CODAE_OK;
}

int launch_emph_loss(const LossLaunch& ll, hipStream_t s) {
    CODAE_REQUIRE(ll.emph, "emph_loss: bad args");
    int rc = check_loss_launch("emph_loss", ll, true);
    if (rc) return rc;
    const codae_batch* b = ll.batch;
    const int64_t dy_ld = loss_dy_ld(ll);
    const WeightArgs wa = weight_args(ll, true);
    const bool vec = (b->io % 4 == 0) && (dy_ld % 4 == 0) && loss_inputs_a16(ll) && a16(ll.dy) && (!wa.col_weight || a16(wa.col_weight));
    const dim3 grid(mse_loss_colsum_rows(b->B));
    loss_dispatch(vec, ll.dy_bf16, ll.present != nullptr, [&](auto V, auto O, auto P) {
        hipLaunchKernelGGL((emph_loss_kernel<decltype(V)::value, decltype(O)::value, decltype(P)::value>), grid, dim3(NT), 0, s, b->data,
                           b->row_idx, b->mask_id, b->mask_table, b->B, b->io, ll.y, ll.dy, ll.scale, ll.colsum_part, ll.parts, b->mask_to_use, b->nb_run,
                           b->run, dy_ld, wa, pres_args(ll));
    });
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_finish_emph_loss(double* scalars, double inv_n, hipStream_t s, const double* parts, int n_parts) {
    CODAE_REQUIRE(scalars && parts && n_parts > 0, "finish_emph_loss: bad args");
    hipLaunchKernelGGL(finish_emph_loss_kernel, dim3(1), dim3(NT), 0, s, scalars, inv_n, parts, n_parts);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_mse_dense(const float* x, const float* y, const float* fmask, float* dy, int64_t n, float inv_n,
                     double* scalars, hipStream_t s) {
    CODAE_REQUIRE(x && y && scalars && n > 0, "mse_dense: bad args");
    hipLaunchKernelGGL(mse_dense_kernel, dim3(grid_for(n)), dim3(NT), 0, s, x, y, fmask, dy, n, inv_n, scalars);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_finish_loss(double* scalars, double inv_n, hipStream_t s, const double* parts, int n_parts) {
    hipLaunchKernelGGL(finish_loss_kernel, dim3(1), dim3(NT), 0, s, scalars, inv_n, parts, parts ? n_parts : 0);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_sumsq(const float* g, int64_t n, double* out, hipStream_t s) {
    CODAE_REQUIRE(g && out && n > 0 && a16(g), "sumsq: bad args");
    hipLaunchKernelGGL(sumsq_kernel, dim3(grid_for(n / 4 + 1)), dim3(NT), 0, s, g, n, out);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

// Tiled form of clip_adam for the bf16 engine: the weight matrices are walked in 64 x 128 tiles so that the same
// pass can also write the TRANSPOSED bf16 shadow (Wt_l [in][out], what the data-gradient GEMM reads) through LDS;
// the blocks past the last tile do the flat bias block.  Replaces clip_adam_kernel + transpose_bf16_kernel: 85 MB
// less traffic per step at C3 and no cross-stream hand-off for the transposes.
struct AdamTiles {
    int n_layers;
    int64_t off[64];          // element offset of W_l in the flat vectors (same in the shadows)
    int rows[64], cols[64];   // W_l is [rows = out][cols = in]
    int tile_begin[65];       // prefix sum of 64 x 128 tiles per layer
    int transposed_from;      // layers >= this also get the transposed shadow
    int64_t bias_off, bias_n; // flat tail
};
constexpr int AT_R = 64, AT_C = 128;

template <int KIND, bool AMS, bool SCHED>
__global__ __launch_bounds__(NT) void clip_adam_tiled_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                             float* __restrict__ m, float* __restrict__ v, AdamConst c,
                                                             const double* __restrict__ grad_sq, bf16_t* __restrict__ shadow,
                                                             bf16_t* __restrict__ shadow_t, AdamTiles jobs,
                                                             const double* __restrict__ step_dev, float* __restrict__ vmax, OptConst o) {
    constexpr bool PLAIN = KIND == CODAE_OPT_ADAM && !AMS && !SCHED;
    constexpr bool HAS_V = KIND != CODAE_OPT_SGD;
    __shared__ bf16_t tt[AT_C][AT_R + 8];          // transposed tile: [col][row], rows stay 16-byte aligned
    __shared__ double total_sq;
    if constexpr (!PLAIN) {
        opt_prologue<KIND, SCHED>(c, o, step_dev);
    } else if (step_dev != nullptr) {
        const double t = *step_dev;
        c.lr_over_bc1 = (float)((double)c.lr / (1.0 - pow((double)c.beta1, t)));
        c.inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)c.beta2, t)));
    }
    float coef = 1.f;
    if (c.max_norm > 0.f) {
        if (threadIdx.x < 64) {
            double sv = grad_sq[(CODAE_S_GRAD_SQ_SLOTS - CODAE_S_GRAD_SQ) + threadIdx.x];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) sv += __shfl_xor(sv, o);
            if (threadIdx.x == 0) total_sq = sv + grad_sq[0];
        }
        __syncthreads();
        coef = clip_coef(c.max_norm, sqrtf((float)total_sq));
    }
    const int n_tiles = jobs.tile_begin[jobs.n_layers];
    if ((int)blockIdx.x >= n_tiles) {
        // flat bias block, grid-strided over the remaining blocks
        const int64_t nb = (int64_t)gridDim.x - n_tiles;
        for (int64_t e = ((int64_t)blockIdx.x - n_tiles) * NT + threadIdx.x; e < jobs.bias_n; e += nb * NT) {
            const int64_t i = jobs.bias_off + e;
            float pp = p[i], mm = m[i], vv = 0.f, xx = 0.f;
            if constexpr (HAS_V) vv = v[i];
            if constexpr (AMS) xx = vmax[i];
            opt_one<KIND, AMS>(pp, g[i], mm, vv, xx, coef, c, o);
            p[i] = pp; m[i] = mm;
            if constexpr (HAS_V) v[i] = vv;
            if constexpr (AMS) vmax[i] = xx;
            shadow[i] = f32_to_bf16(pp);
        }
        return;
    }
    int l = 0;
    while (l + 1 < jobs.n_layers && (int)blockIdx.x >= jobs.tile_begin[l + 1]) ++l;
    const int t = blockIdx.x - jobs.tile_begin[l];
    const int R = jobs.rows[l], C = jobs.cols[l];
    const int tiles_c = (C + AT_C - 1) / AT_C;
    const int r0 = (t / tiles_c) * AT_R, c0 = (t % tiles_c) * AT_C;
    const int64_t base = jobs.off[l];
    const bool want_t = shadow_t != nullptr && l >= jobs.transposed_from;
#pragma unroll
    for (int it = 0; it < AT_R * AT_C / 4 / NT; ++it) {
        const int q = threadIdx.x + it * NT;          // float4 index inside the tile
        const int r = q / (AT_C / 4), cc = (q % (AT_C / 4)) * 4;
        if (r0 + r < R && c0 + cc < C) {
            const int64_t e = base + (int64_t)(r0 + r) * C + c0 + cc;
            float4 pp = *reinterpret_cast<float4*>(p + e);
            const float4 gg = *reinterpret_cast<const float4*>(g + e);
            float4 mm = *reinterpret_cast<float4*>(m + e);
            float4 vv = make_float4(0.f, 0.f, 0.f, 0.f), xx = vv;
            if constexpr (HAS_V) vv = *reinterpret_cast<float4*>(v + e);
            if constexpr (AMS) xx = *reinterpret_cast<float4*>(vmax + e);
            opt_one<KIND, AMS>(pp.x, gg.x, mm.x, vv.x, xx.x, coef, c, o);
            opt_one<KIND, AMS>(pp.y, gg.y, mm.y, vv.y, xx.y, coef, c, o);
            opt_one<KIND, AMS>(pp.z, gg.z, mm.z, vv.z, xx.z, coef, c, o);
            opt_one<KIND, AMS>(pp.w, gg.w, mm.w, vv.w, xx.w, coef, c, o);
            *reinterpret_cast<float4*>(p + e) = pp;
            *reinterpret_cast<float4*>(m + e) = mm;
            if constexpr (HAS_V) *reinterpret_cast<float4*>(v + e) = vv;
            if constexpr (AMS) *reinterpret_cast<float4*>(vmax + e) = xx;
            const uint2 sh = pack_bf16x4(pp.x, pp.y, pp.z, pp.w);
            *reinterpret_cast<uint2*>(shadow + e) = sh;
            if (want_t) {
                tt[cc + 0][r] = (bf16_t)(sh.x & 0xffff); tt[cc + 1][r] = (bf16_t)(sh.x >> 16);
                tt[cc + 2][r] = (bf16_t)(sh.y & 0xffff); tt[cc + 3][r] = (bf16_t)(sh.y >> 16);
            }
        }
    }
    if (!want_t) return;
    __syncthreads();
    // Wt[c0 + c][r0 .. r0 + 63]: 128-B row segments, 16 B per lane
#pragma unroll
    for (int it = 0; it < AT_C * (AT_R / 8) / NT; ++it) {
        const int q = threadIdx.x + it * NT;
        const int cidx = q / (AT_R / 8), r8 = (q % (AT_R / 8)) * 8;
        if (c0 + cidx < C && r0 + r8 < R)
            *reinterpret_cast<uint4*>(shadow_t + base + (int64_t)(c0 + cidx) * R + r0 + r8) =
                *reinterpret_cast<const uint4*>(&tt[cidx][r8]);
    }
}

__global__ void set_scalar_kernel(double* dst, double value) { *dst = value; }

int launch_set_scalar(double* dst, double value, hipStream_t s) {
    CODAE_REQUIRE(dst != nullptr, "set_scalar: null destination");
    hipLaunchKernelGGL(set_scalar_kernel, dim3(1), dim3(1), 0, s, dst, value);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

// ---- the optimizer setting on the host: checks, kernel constants, instantiation --------------
bool optimizer_is_default(const codae_optimizer* o) {
    return o == nullptr || (o->kind == CODAE_OPT_ADAM && o->amsgrad == 0 && o->sched == CODAE_SCHED_CONSTANT && o->warmup == 0);
}

int check_optimizer(const codae_optimizer* o) {
    if (o == nullptr) return CODAE_OK;
    CODAE_REQUIRE(o->kind == CODAE_OPT_ADAM || o->kind == CODAE_OPT_ADAMW || o->kind == CODAE_OPT_SGD, "optimizer: unknown kind %d", o->kind);
    CODAE_REQUIRE(o->amsgrad == 0 || o->amsgrad == 1, "optimizer: amsgrad %d is neither 0 nor 1", o->amsgrad);
    CODAE_REQUIRE(o->nesterov == 0 || o->nesterov == 1, "optimizer: nesterov %d is neither 0 nor 1", o->nesterov);
    CODAE_REQUIRE(!(o->kind == CODAE_OPT_SGD && o->amsgrad), "optimizer: amsgrad belongs to adam / adamw, not to sgd");
    CODAE_REQUIRE(finite_f(o->momentum) && o->momentum >= 0.f && o->momentum < 1.f, "optimizer: momentum %g outside [0, 1)", (double)o->momentum);
    CODAE_REQUIRE(!o->nesterov || o->momentum > 0.f, "optimizer: nesterov needs momentum > 0");
    CODAE_REQUIRE(o->sched >= CODAE_SCHED_CONSTANT && o->sched <= CODAE_SCHED_STEP, "optimizer: unknown schedule %d", o->sched);
    CODAE_REQUIRE(o->warmup >= 0, "optimizer: warmup %d < 0", o->warmup);
    if (o->sched == CODAE_SCHED_COSINE || o->sched == CODAE_SCHED_LINEAR) {
        CODAE_REQUIRE(o->total > o->warmup, "optimizer: total %d must exceed warmup %d", o->total, o->warmup);
        CODAE_REQUIRE(finite_f(o->min_factor) && o->min_factor >= 0.f && o->min_factor <= 1.f, "optimizer: min_factor %g outside [0, 1]",
                      (double)o->min_factor);
    }
    if (o->sched == CODAE_SCHED_STEP) {
        CODAE_REQUIRE(o->period >= 1, "optimizer: period %d < 1", o->period);
        CODAE_REQUIRE(finite_f(o->gamma) && o->gamma > 0.f && o->gamma <= 1.f, "optimizer: gamma %g outside (0, 1]", (double)o->gamma);
    }
    CODAE_REQUIRE(!o->amsgrad || (o->vmax != nullptr && a16(o->vmax)), "optimizer: amsgrad needs a 16-byte aligned vmax");
    return CODAE_OK;
}

// Only the fields the kind and the schedule read, everything else zero: the setter stores this form, and the graph key compares its bytes
codae_optimizer optimizer_canonical(const codae_optimizer* o) {
    codae_optimizer c{};
    if (optimizer_is_default(o)) return c;
    c.kind = o->kind; c.sched = o->sched; c.warmup = o->warmup;
    if (o->kind == CODAE_OPT_SGD) { c.momentum = o->momentum; c.nesterov = o->nesterov; }
    else if (o->amsgrad) { c.amsgrad = 1; c.vmax = o->vmax; }
    if (o->sched == CODAE_SCHED_COSINE || o->sched == CODAE_SCHED_LINEAR) { c.total = o->total; c.min_factor = o->min_factor; }
    if (o->sched == CODAE_SCHED_STEP) { c.period = o->period; c.gamma = o->gamma; }
    return c;
}

static AdamConst adam_const(const codae_hyper* hp) {
    AdamConst c;
    const double bc1 = 1.0 - pow((double)hp->beta1, (double)hp->step);
    const double bc2 = 1.0 - pow((double)hp->beta2, (double)hp->step);
    c.lr_over_bc1 = (float)((double)hp->lr / bc1);
    c.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
    c.beta1 = hp->beta1; c.beta2 = hp->beta2; c.eps = hp->eps; c.wd = hp->weight_decay;
    c.max_norm = hp->max_grad_norm; c.lr = hp->lr;
    return c;
}

static OptConst opt_const(const codae_optimizer* opt, const codae_hyper* hp) {
    OptConst o{};
    o.step = hp->step;
    if (!optimizer_is_default(opt)) {
        o.mu = opt->momentum; o.nesterov = opt->nesterov; o.sched = opt->sched; o.warmup = opt->warmup; o.total = opt->total;
        o.period = opt->period; o.min_factor = opt->min_factor; o.gamma = opt->gamma;
    }
    return o;
}

// f(std::integral_constant<int, KIND>, std::bool_constant<AMS>, std::bool_constant<SCHED>) for the setting's instantiation
template <typename F>
static void opt_dispatch(const codae_optimizer* opt, F&& f) {
    const bool dflt = optimizer_is_default(opt);
    const int kind = dflt ? CODAE_OPT_ADAM : opt->kind;
    const bool ams = !dflt && opt->amsgrad != 0;
    const bool sched = !dflt && (opt->sched != CODAE_SCHED_CONSTANT || opt->warmup > 0);
    auto with_sched = [&](auto k, auto a) {
        if (sched) f(k, a, std::true_type{}); else f(k, a, std::false_type{});
    };
    if (kind == CODAE_OPT_SGD) with_sched(std::integral_constant<int, CODAE_OPT_SGD>{}, std::false_type{});
    else if (kind == CODAE_OPT_ADAMW) { if (ams) with_sched(std::integral_constant<int, CODAE_OPT_ADAMW>{}, std::true_type{}); else with_sched(std::integral_constant<int, CODAE_OPT_ADAMW>{}, std::false_type{}); }
    else { if (ams) with_sched(std::integral_constant<int, CODAE_OPT_ADAM>{}, std::true_type{}); else with_sched(std::integral_constant<int, CODAE_OPT_ADAM>{}, std::false_type{}); }
}

int launch_clip_adam(float* p, float* g, float* m, float* v, int64_t n, const codae_hyper* hp,
                     const double* grad_sq, bf16_t* shadow, const double* coef_in, hipStream_t s,
                     const double* step_dev, const codae_optimizer* opt, float* vmax) {
    const bool sgd = !optimizer_is_default(opt) && opt->kind == CODAE_OPT_SGD;
    const bool ams = !optimizer_is_default(opt) && opt->amsgrad != 0;
    CODAE_REQUIRE(p && g && m && (v || sgd) && hp && n > 0, "clip_adam: bad args");
    CODAE_REQUIRE(a16(p) && a16(g) && a16(m) && (sgd || a16(v)), "clip_adam: buffers must be 16-byte aligned");
    CODAE_REQUIRE(!ams || (vmax != nullptr && a16(vmax)), "clip_adam: amsgrad needs a 16-byte aligned vmax");
    CODAE_REQUIRE(hp->step >= 1, "clip_adam: step must be >= 1");
    CODAE_REQUIRE(hp->max_grad_norm <= 0.f || grad_sq || coef_in, "clip_adam: clipping needs the grad_sq scalar");
    const AdamConst c = adam_const(hp);
    const OptConst o = opt_const(opt, hp);
    opt_dispatch(opt, [&](auto K, auto A, auto S) {
        hipLaunchKernelGGL((clip_adam_kernel<decltype(K)::value, decltype(A)::value, decltype(S)::value>), dim3(grid_for(n / 4 + 1)), dim3(NT),
                           0, s, p, g, m, v, n, c, grad_sq, shadow, coef_in, step_dev, vmax, o);
    });
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_clip_adam_tiled(float* p, float* g, float* m, float* v, const codae_hyper* hp, const double* grad_sq,
                           bf16_t* shadow, bf16_t* shadow_t, int n_layers, const int64_t* w_off, const int* rows,
                           const int* cols, int transposed_from, int64_t bias_off, int64_t bias_n, hipStream_t s,
                           const double* step_dev, const codae_optimizer* opt, float* vmax) {
    const bool sgd = !optimizer_is_default(opt) && opt->kind == CODAE_OPT_SGD;
    const bool ams = !optimizer_is_default(opt) && opt->amsgrad != 0;
    CODAE_REQUIRE(p && g && m && (v || sgd) && hp && shadow && n_layers > 0 && n_layers <= 64, "clip_adam_tiled: bad args");
    CODAE_REQUIRE(a16(p) && a16(g) && a16(m) && (sgd || a16(v)), "clip_adam_tiled: buffers must be 16-byte aligned");
    CODAE_REQUIRE(!ams || (vmax != nullptr && a16(vmax)), "clip_adam_tiled: amsgrad needs a 16-byte aligned vmax");
    CODAE_REQUIRE(hp->step >= 1, "clip_adam_tiled: step must be >= 1");
    CODAE_REQUIRE(hp->max_grad_norm <= 0.f || grad_sq, "clip_adam_tiled: clipping needs the grad_sq scalar");
    const AdamConst c = adam_const(hp);
    const OptConst o = opt_const(opt, hp);
    AdamTiles jobs;
    jobs.n_layers = n_layers; jobs.transposed_from = transposed_from; jobs.bias_off = bias_off; jobs.bias_n = bias_n;
    int total = 0;
    for (int l = 0; l < n_layers; ++l) {
        CODAE_REQUIRE(rows[l] % 8 == 0 && cols[l] % 4 == 0 && w_off[l] % 8 == 0, "clip_adam_tiled: layer %d shape %d x %d", l, rows[l], cols[l]);
        jobs.off[l] = w_off[l]; jobs.rows[l] = rows[l]; jobs.cols[l] = cols[l];
        jobs.tile_begin[l] = total;
        total += ((rows[l] + AT_R - 1) / AT_R) * ((cols[l] + AT_C - 1) / AT_C);
    }
    jobs.tile_begin[n_layers] = total;
    const int bias_blocks = (int)((bias_n + NT * 8 - 1) / (NT * 8)) > 0 ? (int)((bias_n + NT * 8 - 1) / (NT * 8)) : 1;
    opt_dispatch(opt, [&](auto K, auto A, auto S) {
        hipLaunchKernelGGL((clip_adam_tiled_kernel<decltype(K)::value, decltype(A)::value, decltype(S)::value>), dim3(total + bias_blocks),
                           dim3(NT), 0, s, p, g, m, v, c, grad_sq, shadow, shadow_t, jobs, step_dev, vmax, o);
    });
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_sumsq_to(const float* g, int64_t n, double* acc, hipStream_t s) {
    CODAE_REQUIRE(g && acc && n > 0, "sumsq_to: bad args");
    int grid = grid_for(n / 4 + 1);
    if (grid > 64) grid = 64;
    hipLaunchKernelGGL(sumsq_to_kernel, dim3(grid), dim3(NT), 0, s, g, n, acc);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_clip_coef(const double* total_sq, float max_norm, double* coef_out, hipStream_t s) {
    hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(1), 0, s, total_sq, max_norm, coef_out);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_colsum_f32(const float* src, int M, int N, float* out, hipStream_t s) {
    CODAE_REQUIRE(src && out && M > 0 && N > 0, "colsum: bad args");
    hipLaunchKernelGGL(colsum_f32_kernel, dim3((N + NT - 1) / NT), dim3(NT), 0, s, src, M, N, out);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_colsum_parts_f32(const float* src, int M, int N, float* parts, hipStream_t s) {
    CODAE_REQUIRE(src && parts && M > 0 && N > 0, "colsum_parts: bad args");
    hipLaunchKernelGGL(colsum_parts_f32_kernel, dim3((M + 63) / 64, (N + NT - 1) / NT), dim3(NT), 0, s, src, M, N, parts);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_bias_finish(const BiasFinishJobs& jobs, double* sumsq, hipStream_t s, const LossFinish* loss) {
    CODAE_REQUIRE(jobs.n > 0 && jobs.n <= 64, "bias_finish: %d jobs", jobs.n);
    const int total = jobs.col_begin[jobs.n];
    CODAE_REQUIRE(total > 0, "bias_finish: no columns");
    LossFinish lf{};
    if (loss != nullptr) { lf = *loss; CODAE_REQUIRE(lf.scalars && lf.parts && lf.n_parts > 0, "bias_finish: bad loss block"); }
    hipLaunchKernelGGL(bias_finish_kernel, dim3((total + NT - 1) / NT + (loss != nullptr ? 1 : 0)), dim3(NT), 0, s, jobs, sumsq, lf);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_transpose_bf16(const bf16_t* src, bf16_t* dst, int n, const int64_t* off, const int* rows, const int* cols,
                          hipStream_t s) {
    CODAE_REQUIRE(src && dst && n > 0 && n <= 64, "transpose: bad args");
    TransposeJobs jobs;
    jobs.n = n;
    int total = 0;
    for (int i = 0; i < n; ++i) {
        CODAE_REQUIRE(rows[i] % 8 == 0 && cols[i] % 8 == 0, "transpose: matrix %d is %d x %d (need multiples of 8)", i, rows[i], cols[i]);
        jobs.off[i] = off[i]; jobs.rows[i] = rows[i]; jobs.cols[i] = cols[i];
        jobs.tile_begin[i] = total;
        total += ((rows[i] + 63) / 64) * ((cols[i] + 63) / 64);
    }
    jobs.tile_begin[n] = total;
    hipLaunchKernelGGL(transpose_bf16_kernel, dim3(total), dim3(NT), 0, s, src, dst, jobs);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_reduce_slabs(const float* slabs, int n_slabs, int64_t stride, float* out, int64_t n, double* sumsq,
                        hipStream_t s) {
    CODAE_REQUIRE(slabs && out && n_slabs >= 1 && n > 0, "reduce_slabs: bad args");
    hipLaunchKernelGGL(reduce_slabs_kernel, dim3(grid_for(n / 4 + 1)), dim3(NT), 0, s, slabs, n_slabs, stride, out, n, sumsq);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_reduce_slabs_epi(const float* slabs, int n_slabs, int64_t stride, int M, int N, float* C, int64_t ldc, const float* bias,
                            int relu, const float* relu_src, int64_t ld_relu, float* colsum_part, hipStream_t s, int act,
                            const float* act_p) {
    CODAE_REQUIRE(slabs && C && n_slabs >= 1 && M > 0 && N > 0 && N % 4 == 0 && ldc % 4 == 0 && (relu_src == nullptr || ld_relu % 4 == 0) &&
                      a16(slabs) && a16(C) && (bias == nullptr || a16(bias)) && (relu_src == nullptr || a16(relu_src)),
                  "reduce_slabs_epi: bad args");
    CODAE_REQUIRE(act == CODAE_ACT_NONE || act_p != nullptr, "reduce_slabs_epi: activation without parameters");
    if (act != CODAE_ACT_NONE)
        hipLaunchKernelGGL(reduce_slabs_epi_kernel<true>, dim3((N + 63) / 64, (M + 63) / 64), dim3(NT), 0, s, slabs, n_slabs, stride, M, N, C, ldc,
                           bias, relu, relu_src, ld_relu, colsum_part, act, act_p[0], act_p[1], act_p[2]);
    else
        hipLaunchKernelGGL(reduce_slabs_epi_kernel<false>, dim3((N + 63) / 64, (M + 63) / 64), dim3(NT), 0, s, slabs, n_slabs, stride, M, N, C, ldc,
                           bias, relu, relu_src, ld_relu, colsum_part, 0, 0.f, 0.f, 0.f);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

}  // namespace codae
