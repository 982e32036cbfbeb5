// The batch's way into the step: gather + input noise + slot corruption + slot presence in one pass (from the fp32 rows, or from
// the dataset's bf16 image), the casts, and the dense corrupt / mask expansion of the drop-in path.  All are single-pass, 16 B per
// lane where the row width allows, grid capped at 2048 blocks with a grid-stride loop.
#include "loss_sweep.h"

namespace codae {
namespace {

constexpr int NT = GRID_NT;

// zero_norm != null (the fused step whose loss finish rides in the bias-finish launch): the launch's first block clears the
// clip_grad_norm_ accumulators - what finish_loss_kernel does in front of the backward when it runs as a launch of its own
__device__ __forceinline__ void zero_norm_scalars(double* zero_norm) {
    if (zero_norm != nullptr && blockIdx.x == 0) {
        if (threadIdx.x == 0) zero_norm[CODAE_S_GRAD_SQ] = 0.0;
        if (threadIdx.x < CODAE_S_N_SLOTS) zero_norm[CODAE_S_GRAD_SQ_SLOTS + threadIdx.x] = 0.0;
    }
}

// ---- input noise (codae_noise, include/codae_hip.h) ---------------------------------------------------------------------------
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
// swap noise moves whole slots and does no arithmetic: the words' key and threshold travel in sw; sdata = the matrix the swapped
// slots are read from (the batch's own data unless the caller gathered the batch)
struct SwapGather {
    SwapArgs sw; const float* sdata;
};
// the kernel argument of one noise kind; the plain gather (CODAE_NOISE_NONE) keeps the argument block it always had
template <int KIND>
struct NoiseArgsOf : NoiseArgs {
    NoiseArgsOf(const NoiseArgs& a, const SwapGather&) : NoiseArgs(a) {}
};
template <>
struct NoiseArgsOf<CODAE_NOISE_NONE> {
    double* zero_norm;
    NoiseArgsOf(const NoiseArgs& a, const SwapGather&) : zero_norm(a.zero_norm) {}
};
template <>
struct NoiseArgsOf<CODAE_NOISE_SWAP> {
    uint32_t step; const double* step_dev; const int32_t* rows; double* zero_norm;
    SwapArgs sw; const float* sdata;
    NoiseArgsOf(const NoiseArgs& a, const SwapGather& g) : step(a.step), step_dev(a.step_dev), rows(a.rows), zero_norm(a.zero_norm), sw(g.sw), sdata(g.sdata) {}
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

// ---- the gather's steps, each for W = 8, 4 or 1 columns of one row ------------------------------------------------------------
template <int W>
__device__ __forceinline__ void load_cols(float* v, const float* __restrict__ src) {
    if constexpr (W == 1) {
        v[0] = src[0];
    } else {
#pragma unroll
        for (int q = 0; q < W / 4; ++q) {
            const float4 x = *reinterpret_cast<const float4*>(src + 4 * q);
            v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w;
        }
    }
}

// the same columns of batch row b (read from dataset row src_row) with their noise at `step`, one Philox call per group of four
// columns; returns the noise row.
// (The 4-wide form has its noise row and Philox rounds in front of its load and the other two behind theirs, as the separate kernels
// did: the compiler's register allocation follows the source order, and the register counts of DESIGN.md 5k hold only this way.)
template <int W, int KIND>
__device__ __forceinline__ uint32_t load_noised(float* v, const float* __restrict__ src, int c, int b, int64_t src_row, uint32_t step,
                                                const NoiseArgs& na) {
    const uint32_t g = (uint32_t)(c >> 2);
    if constexpr (W == 4) {
        const uint32_t nrow = na.rows ? (uint32_t)na.rows[b] : (uint32_t)src_row;
        const uint4 r = philox4x32_10(g, nrow, step, 0u, na.key0, na.key1);
        load_cols<4>(v, src);
        noise_apply4<KIND>(v, r, na);
        return nrow;
    } else {
        load_cols<W>(v, src);
        const uint32_t nrow = na.rows ? (uint32_t)na.rows[b] : (uint32_t)src_row;
        if constexpr (W == 1) v[0] = noise_apply1<KIND>(v[0], philox4x32_10(g, nrow, step, 0u, na.key0, na.key1), c & 3, na);
        else {
#pragma unroll
            for (int q = 0; q < W / 4; ++q) noise_apply4<KIND>(v + 4 * q, philox4x32_10(g + (uint32_t)q, nrow, step, 0u, na.key0, na.key1), na);
        }
        return nrow;
    }
}

// the same columns of batch row b under swap noise: each column comes from the row its slot's draw accepted (sdata[q]), else from
// `src`.  A group inside one slot - every group when E % W == 0 - is one Philox call and the vector load of one row; a group that
// straddles slots (E = 6, E = 12) forms a draw per slot it touches and loads by column.  Returns the noise row.
template <int W>
__device__ __forceinline__ uint32_t load_swapped(float* v, const float* __restrict__ src, int c, int b, int64_t src_row, int io,
                                                 uint32_t step, const NoiseArgsOf<CODAE_NOISE_SWAP>& na) {
    const uint32_t nrow = na.rows ? (uint32_t)na.rows[b] : (uint32_t)src_row;
    const int E = na.sw.E;
    const int s0 = c / E, rem = c - s0 * E;
    if (W == 1 || rem + W <= E) {
        const int64_t q = swap_source(na.sw, nrow, s0, step);
        load_cols<W>(v, q >= 0 ? na.sdata + q * io + c : src);
    } else {
        const float* __restrict__ from = src;
        int s_at = -1;
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const int sk = s0 + (rem + k) / E;
            if (sk != s_at) {
                const int64_t q = swap_source(na.sw, nrow, sk, step);
                from = q >= 0 ? na.sdata + q * io + c : src;
                s_at = sk;
            }
            v[k] = from[k];
        }
    }
    return nrow;
}

// the slot mask: v[k] survives where byte k of the mask row is not zero (the W bytes in one load)
template <int W>
__device__ __forceinline__ void mask_cols(float* v, const uint8_t* __restrict__ mrow) {
    uint32_t m[(W + 3) / 4];
    if constexpr (W == 8) { const uint2 t = *reinterpret_cast<const uint2*>(mrow); m[0] = t.x; m[1] = t.y; }
    else if constexpr (W == 4) m[0] = *reinterpret_cast<const uint32_t*>(mrow);
    else m[0] = mrow[0];
#pragma unroll
    for (int k = 0; k < W; ++k) v[k] = ((m[k >> 2] >> (8 * (k & 3))) & 0xff) ? v[k] : 0.f;
}

// the presence rule: exactly 0 in every column of an absent slot, behind the noise and the slot mask
template <int W>
__device__ __forceinline__ void zero_absent(float* v, const PresArgs& pa, int64_t row, int c) {
    int sl[W];
    slots_of<W>(c, pa.E, sl);
    const uint32_t pb = present_bits<W>(pa, row, sl);
#pragma unroll
    for (int k = 0; k < W; ++k) v[k] = ((pb >> k) & 1u) ? v[k] : 0.f;
}

// W = 8 (bf16 only: the training step's form) is one 16-B store; the 4-wide bf16 form stores 8 B per lane
template <int W, bool OUT_BF16>
__device__ __forceinline__ void store_cols(void* __restrict__ out, int64_t o, const float* v) {
    if constexpr (OUT_BF16) {
        bf16_t* op = reinterpret_cast<bf16_t*>(out) + o;
        if constexpr (W == 8)
            *reinterpret_cast<uint4*>(op) = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
        else if constexpr (W == 4) *reinterpret_cast<uint2*>(op) = pack_bf16x4(v[0], v[1], v[2], v[3]);
        else op[0] = f32_to_bf16(v[0]);
    } else {
        static_assert(W != 8, "the 8-wide gather writes bf16");
        float* op = reinterpret_cast<float*>(out) + o;
        if constexpr (W == 4) *reinterpret_cast<float4*>(op) = make_float4(v[0], v[1], v[2], v[3]);
        else op[0] = v[0];
    }
}

// ---- a2 + a10: out[b][:] = noise(data[row_idx[b]][:]) * mask_table[mask_id[b]][:], absent slots cleared -----------------------
// (collate_embedding data_tool.py:96-103 + corrupt embedding_...py:226-239 fused; the [B,io] fp32 mask of Corrupter.get_masks is
// never materialised.)  One kernel for every width W (columns per thread), output type, noise kind (CODAE_NOISE_NONE: the plain
// gather) and presence.  The presence table is keyed by the noise row when there is noise, else by the row read.
// (Measured and dropped for W = 8: whole rows per wave - 2 rows x up to 4 column chunks of 16-B loads in flight per lane, row index and
// mask id read once per row: 28.0 -> 27.1 us per launch on one box, 27.3 -> 27.8 on another: inside the noise)
template <int W, bool OUT_BF16, int KIND, bool PRES>
__global__ __launch_bounds__(NT) void gather_corrupt_kernel(const float* __restrict__ data, const int32_t* __restrict__ row_idx,
                                                            const int32_t* __restrict__ mask_id, const uint8_t* __restrict__ table, int B,
                                                            int io, void* __restrict__ out, const int32_t* __restrict__ mask_to_use,
                                                            int nb_run, int run, int64_t out_ld, NoiseArgsOf<KIND> na, PresArgs pa) {
    constexpr bool NOISE = KIND != CODAE_NOISE_NONE;
    zero_norm_scalars(na.zero_norm);
    const bool masked = (mask_id != nullptr) || (mask_to_use != nullptr);
    uint32_t step = 0u;
    if constexpr (NOISE) step = na.step_dev ? (uint32_t)*na.step_dev : na.step;
    const int cols = io / W;
    const int64_t total = (int64_t)B * cols;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < total; e += (int64_t)gridDim.x * NT) {
        const int b = (int)(e / cols);
        const int c = (int)(e - (int64_t)b * cols) * W;
        const int64_t src_row = row_idx ? row_idx[b] : b;
        const float* src = data + src_row * io + c;
        int64_t pres_row = src_row;
        float v[W];
        if constexpr (KIND == CODAE_NOISE_SWAP) pres_row = (int64_t)load_swapped<W>(v, src, c, b, src_row, io, step, na);
        else if constexpr (NOISE) pres_row = (int64_t)load_noised<W, KIND>(v, src, c, b, src_row, step, na);
        else load_cols<W>(v, src);
        if (masked) {
            const int id = mask_id ? mask_id[b] : mask_to_use[src_row * nb_run + run];
            mask_cols<W>(v, table + (int64_t)id * io + c);
        }
        if constexpr (PRES) zero_absent<W>(v, pa, pres_row, c);
        store_cols<W, OUT_BF16>(out, (int64_t)b * out_ld + c, v);
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
// SWAP (swap noise): a kept group reads the image row its slot's draw accepted - the bits of the fp32 route, which rounds the same
// fp32 row -; the draw is formed behind the blank test, so a wholly blanked group still costs neither a word nor a load.  A group
// that straddles slots (E % 8 != 0) loads by column.  The un-swapped instantiations keep their argument block and their code.
template <bool SWAP>
struct ImageHead {
    double* zero_norm;
};
template <>
struct ImageHead<true> {
    double* zero_norm;
    uint32_t step; const double* step_dev;
    SwapArgs sw;
};
template <bool PRES, bool SWAP>
__global__ __launch_bounds__(NT) void gather_corrupt_image_kernel(const bf16_t* __restrict__ image,
                                                                  const int32_t* __restrict__ row_idx,
                                                                  const int32_t* __restrict__ mask_id,
                                                                  const uint8_t* __restrict__ table, int B, int io,
                                                                  bf16_t* __restrict__ out,
                                                                  const int32_t* __restrict__ mask_to_use, int nb_run,
                                                                  int run, int64_t out_ld, ImageHead<SWAP> hd, PresArgs pa) {
    zero_norm_scalars(hd.zero_norm);
    const bool masked = (mask_id != nullptr) || (mask_to_use != nullptr);
    uint32_t step = 0u;
    if constexpr (SWAP) step = hd.step_dev ? (uint32_t)*hd.step_dev : hd.step;
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
            if constexpr (SWAP) {
                const int E = hd.sw.E;
                const int s0 = c / E, rem = c - s0 * E;
                uint4 x;
                if (rem + 8 <= E) {
                    const int64_t q = swap_source(hd.sw, (uint32_t)src_row, s0, step);
                    x = *reinterpret_cast<const uint4*>(image + (q >= 0 ? q : src_row) * io + c);
                } else {
                    const bf16_t* __restrict__ from = image + src_row * io + c;
                    int s_at = -1;
                    uint32_t h[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const int sk = s0 + (rem + k) / E;
                        if (sk != s_at) {
                            const int64_t q = swap_source(hd.sw, (uint32_t)src_row, sk, step);
                            from = image + (q >= 0 ? q : src_row) * io + c;
                            s_at = sk;
                        }
                        h[k] = from[k];
                    }
                    x = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
                }
                o = make_uint4(x.x & keep.x, x.y & keep.y, x.z & keep.z, x.w & keep.w);
            } else {
                const uint4 x = *reinterpret_cast<const uint4*>(image + src_row * io + c);
                o = make_uint4(x.x & keep.x, x.y & keep.y, x.z & keep.z, x.w & keep.w);
            }
        }
        *reinterpret_cast<uint4*>(out + (int64_t)b * out_ld + c) = o;
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

// the batch checks of every gather launcher, the error texts prefixed with `who`; src: where the rows come from
int check_gather(const char* who, const codae_batch* b, const void* src, const void* out, const uint8_t* present, int n_slots) {
    CODAE_REQUIRE(b && src && out && b->B > 0 && b->io > 0, "%s: bad batch", who);
    const int rc = check_presence(present, n_slots, b->io, who);
    if (rc) return rc;
    CODAE_REQUIRE(!(b->mask_id || b->mask_to_use) || b->mask_table, "%s: mask ids without mask_table", who);
    CODAE_REQUIRE(!b->mask_to_use || b->mask_id || (b->nb_run > 0 && b->run >= 0 && b->run < b->nb_run), "%s: run %d outside [0, %d)", who,
                  b->run, b->nb_run);
    return CODAE_OK;
}

// f(std::integral_constant<int, W>, std::bool_constant<OUT_BF16>, std::integral_constant<int, KIND>, std::bool_constant<PRES>) for
// the launch's instantiation (width 8 is bf16 only)
template <typename F>
void gather_dispatch(int width, bool out_bf16, int kind, bool pres, F&& f) {
    auto with_pres = [&](auto W, auto O, auto K) { if (pres) f(W, O, K, std::true_type{}); else f(W, O, K, std::false_type{}); };
    auto with_kind = [&](auto W, auto O) {
        if (kind == CODAE_NOISE_GAUSSIAN) with_pres(W, O, std::integral_constant<int, CODAE_NOISE_GAUSSIAN>{});
        else if (kind == CODAE_NOISE_MASKING) with_pres(W, O, std::integral_constant<int, CODAE_NOISE_MASKING>{});
        else if (kind == CODAE_NOISE_SALT_PEPPER) with_pres(W, O, std::integral_constant<int, CODAE_NOISE_SALT_PEPPER>{});
        else if (kind == CODAE_NOISE_SWAP) with_pres(W, O, std::integral_constant<int, CODAE_NOISE_SWAP>{});
        else with_pres(W, O, std::integral_constant<int, CODAE_NOISE_NONE>{});
    };
    auto with_out = [&](auto W) { if (out_bf16) with_kind(W, std::true_type{}); else with_kind(W, std::false_type{}); };
    if (width == 8) with_kind(std::integral_constant<int, 8>{}, std::true_type{});
    else if (width == 4) with_out(std::integral_constant<int, 4>{});
    else with_out(std::integral_constant<int, 1>{});
}

}  // namespace

int check_presence(const uint8_t* present, int n_slots, int io, const char* who) {
    if (present == nullptr) return CODAE_OK;
    CODAE_REQUIRE(n_slots >= 1 && n_slots <= 128, "%s: slot presence takes 1 .. 128 slots, got %d", who, n_slots);
    CODAE_REQUIRE(io > 0 && io % n_slots == 0, "%s: slot presence: n_slots %d does not divide io %d", who, n_slots, io);
    return CODAE_OK;
}

int check_swap(const codae_swap* sw, int io, const uint8_t* present, int pres_slots, const char* who) {
    CODAE_REQUIRE(sw != nullptr && sw->n_slots >= 1, "%s: swap noise needs its slot count (codae_set_swap_pool / codae_swap)", who);
    CODAE_REQUIRE(io > 0 && io % sw->n_slots == 0, "%s: swap noise: n_slots %d does not divide io %d", who, sw->n_slots, io);
    CODAE_REQUIRE(sw->n_pool >= 1, "%s: swap noise: a pool of %d rows", who, sw->n_pool);
    CODAE_REQUIRE(present == nullptr || pres_slots == sw->n_slots, "%s: swap noise: n_slots %d differs from the presence table's %d", who,
                  sw->n_slots, pres_slots);
    return CODAE_OK;
}

int check_noise(const codae_noise* n) {
    if (n == nullptr || n->kind == CODAE_NOISE_NONE) return CODAE_OK;
    CODAE_REQUIRE(n->kind == CODAE_NOISE_GAUSSIAN || n->kind == CODAE_NOISE_MASKING || n->kind == CODAE_NOISE_SALT_PEPPER ||
                      n->kind == CODAE_NOISE_SWAP,
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
                        hipStream_t s, int64_t out_ld, const int32_t* noise_rows, double* zero_norm, const uint8_t* present, int n_slots,
                        const codae_swap* swap, const float* swap_data) {
    const int kind = noise ? noise->kind : CODAE_NOISE_NONE;
    // (the plain gather keys the table by the row it reads: a batch gathered by the caller has lost its dataset rows)
    CODAE_REQUIRE(kind != CODAE_NOISE_NONE || present == nullptr || noise_rows == nullptr,
                  "gather_corrupt: a presence table with noise_rows needs an input noise kind");
    int rc = check_noise(noise);
    if (rc) return rc;
    rc = check_gather("gather_corrupt", b, b ? b->data : nullptr, out, present, n_slots);
    if (rc) return rc;
    SwapGather sg{};
    if (kind == CODAE_NOISE_SWAP) {
        rc = check_swap(swap, b->io, present, n_slots, "gather_corrupt");
        if (rc) return rc;
        CODAE_REQUIRE(noise_rows == nullptr || swap_data != nullptr, "gather_corrupt: swap noise on a gathered batch (noise_rows) needs the dataset");
        sg.sw = swap_args(noise, swap, b->io, present);
        sg.sdata = swap_data ? swap_data : b->data;
    }
    if (out_ld <= 0) out_ld = b->io;
    const PresArgs pa{present, n_slots, present ? b->io / n_slots : 0};
    NoiseArgs na{};
    na.zero_norm = zero_norm;
    if (kind != CODAE_NOISE_NONE) {
        na.key0 = (uint32_t)(noise->seed & 0xffffffffu); na.key1 = (uint32_t)(noise->seed >> 32);
        na.step = (uint32_t)step; na.step_dev = step_dev; na.rows = noise_rows;
        na.thresh = (uint64_t)floor((double)noise->p0 * 4294967296.0);      // (p <= 1: at most 2^32, above every word)
        na.p0 = noise->p0; na.p1 = noise->p1; na.p2 = noise->p2;
    }
    const bool masked = b->mask_id || b->mask_to_use;
    const bool vec = (b->io % 4 == 0) && (out_ld % 4 == 0) && a16(b->data) && (sg.sdata == nullptr || a16(sg.sdata)) && a16(out) && (!masked || (reinterpret_cast<uintptr_t>(b->mask_table) & 3) == 0);
    const int64_t items = (int64_t)b->B * (vec ? b->io / 4 : b->io);
    const bool x8 = vec && out_bf16 && b->io % 8 == 0 && (!masked || (reinterpret_cast<uintptr_t>(b->mask_table) & 7) == 0);
    const int grid = grid_for(x8 ? items / 2 : items);
    gather_dispatch(x8 ? 8 : (vec ? 4 : 1), out_bf16 != 0, kind, present != nullptr, [&](auto W, auto O, auto K, auto P) {
        hipLaunchKernelGGL((gather_corrupt_kernel<decltype(W)::value, decltype(O)::value, decltype(K)::value, decltype(P)::value>), dim3(grid),
                           dim3(NT), 0, s, b->data, b->row_idx, b->mask_id, b->mask_table, b->B, b->io, out, b->mask_to_use, b->nb_run, b->run,
                           out_ld, NoiseArgsOf<decltype(K)::value>(na, sg), pa);
    });
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
                        const uint8_t* present, int n_slots, const codae_noise* noise, int32_t step, const double* step_dev,
                        const codae_swap* swap) {
    int rc = check_gather("gather_image", b, image, out, present, n_slots);
    if (rc) return rc;
    const int kind = noise ? noise->kind : CODAE_NOISE_NONE;
    CODAE_REQUIRE(kind == CODAE_NOISE_NONE || kind == CODAE_NOISE_SWAP, "gather_image: noise kind %d needs the fp32 rows", kind);
    ImageHead<true> hs{};
    if (kind == CODAE_NOISE_SWAP) {
        rc = check_noise(noise);
        if (rc) return rc;
        rc = check_swap(swap, b->io, present, n_slots, "gather_image");
        if (rc) return rc;
        hs.zero_norm = zero_norm; hs.step = (uint32_t)step; hs.step_dev = step_dev;
        hs.sw = swap_args(noise, swap, b->io, present);
    }
    if (out_ld <= 0) out_ld = b->io;
    const PresArgs pa{present, n_slots, present ? b->io / n_slots : 0};
    CODAE_REQUIRE(gather_image_takes(b, image, out, out_ld),
                  "gather_image: io %d and out_ld %lld must be multiples of 8, image and out 16-byte and mask_table 8-byte aligned", b->io,
                  (long long)out_ld);
    const int grid = grid_for((int64_t)b->B * (b->io / 8));
#define GCI(P, W, HD) hipLaunchKernelGGL((gather_corrupt_image_kernel<P, W>), dim3(grid), dim3(NT), 0, s, image, b->row_idx, b->mask_id, b->mask_table, \
                                         b->B, b->io, out, b->mask_to_use, b->nb_run, b->run, out_ld, HD, pa)
    const ImageHead<false> hp{zero_norm};
    if (kind == CODAE_NOISE_SWAP) {
        if (present) GCI(true, true, hs);
        else GCI(false, true, hs);
    } else {
        if (present) GCI(true, false, hp);
        else GCI(false, false, hp);
    }
#undef GCI
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

}  // namespace codae
