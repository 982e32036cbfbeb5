// Training criterion other than the mean squared error (codae_recon_loss, include/codae_hip.h, "Training criterion"): the
// stand-alone loss kernels behind the last forward GEMM, on the seam emph_loss_kernel (elementwise.hip) uses - one block per
// LOSS_ROWS batch rows, dY + one partial column-sum row + three per-block sums, finished by finish_emph_loss_kernel.
//   recon_elem_kernel<KIND, ..>   L1 / SmoothL1 / Huber: emph_loss_kernel's block shape with rho as a template parameter
//   slot_cosine_kernel<..>        1 - cos per (row, slot): a wave reduces each pair, then the column-owner loop writes dY
// The emphasis weight w of an element is formed exactly as emph_loss_kernel forms it ("replaced" from the element's Philox word).
#include <math.h>

#include "codae_common.h"

namespace codae {
namespace {

constexpr int NT = 256;
constexpr int WAVES = NT / 64;
constexpr int LOSS_ROWS = 32;    // rows per block = rows per partial column-sum row (mse_loss_colsum_rows)
constexpr int LOSS_UNROLL = 8;   // rows in flight per thread
constexpr int MAX_SLOTS = 128;   // slot_cosine: the coefficient table is LOSS_ROWS * n_slots * 2 floats of LDS (32 KiB at most)

// keeps a sum / product a scalar VALU op of its own: the SLP vectorizer otherwise packs neighbouring columns' chains into
// v_pk_*_f32 with op_sel routing (tools/check_isa.py rule 4)
__device__ __forceinline__ float opaque(float x) { asm("" : "+v"(x)); return x; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// sum over the 256-thread block, the waves' sums added in wave order; result valid in thread 0
__device__ __forceinline__ float block_sum(float v, float* red /*[WAVES]*/) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = 0.f;
    if (threadIdx.x == 0) r = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return r;
}

__device__ __forceinline__ uint2 pack_bf16x4(float a, float b, float c, float d) {
    uint2 o;
    o.x = (uint32_t)f32_to_bf16(a) | ((uint32_t)f32_to_bf16(b) << 16);
    o.y = (uint32_t)f32_to_bf16(c) | ((uint32_t)f32_to_bf16(d) << 16);
    return o;
}

struct ReconArgs {
    // the emphasis weight (emph_loss_kernel's EmphArgs; alpha = beta = 1 and no column weights when emphasis is off)
    float alpha, beta;
    const float* col_weight;   // [io] or null (all ones)
    int replace;               // the input noise is MASKING or SALT_PEPPER: a word below thresh marks a replaced element
    uint64_t thresh;           // T = floor(p 2^32)
    uint32_t key0, key1;
    uint32_t step;             // counter word 2 ...
    const double* step_dev;    // ... or, when not null, *step_dev (graph replay)
    // the criterion
    float param, rparam;       // beta (SMOOTH_L1) / delta (HUBER) and its reciprocal
    float mse_weight;          // SLOT_COSINE
    int S, E;                  // SLOT_COSINE: slots per row, columns per slot
};

struct BatchArgs {
    const float* data; const int32_t* row_idx; const int32_t* mask_id; const uint8_t* table; const int32_t* mask_to_use;
    int nb_run, run, B, io;
};

// sign(d) with sign(0) = 0; a NaN d stays NaN
__device__ __forceinline__ float sign_or_self(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : d); }

// rho(d) and d rho / dd of an element-wise kind (the table of include/codae_hip.h); NaN in, NaN out (both)
template <int KIND>
__device__ __forceinline__ void rho_of(float d, const ReconArgs& a, float& rho, float& drho) {
    const float ad = fabsf(d);
    if constexpr (KIND == CODAE_LOSS_L1) {
        rho = ad;
        drho = sign_or_self(d);
    } else if constexpr (KIND == CODAE_LOSS_SMOOTH_L1) {
        const bool quad = ad < a.param;
        rho = quad ? opaque(0.5f * d) * opaque(d * a.rparam) : ad - 0.5f * a.param;
        drho = quad ? d * a.rparam : sign_or_self(d);
    } else {   // CODAE_LOSS_HUBER
        const bool quad = ad <= a.param;
        rho = quad ? opaque(0.5f * d) * d : a.param * opaque(ad - 0.5f * a.param);
        drho = quad ? d : a.param * sign_or_self(d);
    }
}

// which of the four columns c .. c + 3 of dataset row `row` the gather's noise replaced (c a multiple of 4: one Philox group)
__device__ __forceinline__ void hits4(bool* hit, int c, uint32_t row, uint32_t step, const ReconArgs& a) {
    const uint4 r = philox4x32_10((uint32_t)(c >> 2), row, step, 0u, a.key0, a.key1);
    hit[0] = (uint64_t)r.x < a.thresh; hit[1] = (uint64_t)r.y < a.thresh;
    hit[2] = (uint64_t)r.z < a.thresh; hit[3] = (uint64_t)r.w < a.thresh;
}
// the same for the single column c (word c % 4 of its group; selects, no indexed register array)
__device__ __forceinline__ bool hit1(int c, uint32_t row, uint32_t step, const ReconArgs& a) {
    const uint4 r = philox4x32_10((uint32_t)(c >> 2), row, step, 0u, a.key0, a.key1);
    const int k = c & 3;
    const uint32_t rk = (k & 2) ? ((k & 1) ? r.w : r.z) : ((k & 1) ? r.y : r.x);
    return (uint64_t)rk < a.thresh;
}

// sl[k] = slot of column c + k (E columns per slot): one division where the group sits inside one slot
template <int W>
__device__ __forceinline__ void slots_of(int c, int E, int* sl) {
    const int s0 = c / E, rem = c - s0 * E;
    if (rem + W <= E) {
#pragma unroll
        for (int k = 0; k < W; ++k) sl[k] = s0;
    } else {
#pragma unroll
        for (int k = 0; k < W; ++k) sl[k] = s0 + (rem + k) / E;
    }
}

// ---- L1 / SmoothL1 / Huber -----------------------------------------------------------------------------------------------------
//   dy = w rho'(d) (-1) inv_n, d = x - y;   parts[block] = { sum w rho(d), sum d^2, sum (1-fmask) d^2 }
// PRES (a presence table is set): an absent element's x and y are SELECTED to 0 as they are loaded (x may be NaN there): d = 0,
// rho = rho' = 0, exact zeros into every sum; its stored dy is +0.  Between the loads and the stores the text is the one without a table.
template <int KIND, bool VEC, bool DY_BF16, bool PRES>
__global__ __launch_bounds__(NT) void recon_elem_kernel(BatchArgs ba, const float* __restrict__ y, void* __restrict__ dy, float inv_n,
                                                        float* __restrict__ colsum_part, double* __restrict__ parts, int64_t dy_ld,
                                                        ReconArgs ea, PresArgs pa) {
    __shared__ float red[WAVES];
    const float* __restrict__ data = ba.data;
    const uint8_t* __restrict__ table = ba.table;
    const int B = ba.B, io = ba.io;
    const bool masked = (ba.mask_id != nullptr) || (ba.mask_to_use != nullptr);
    const uint32_t step = ea.step_dev ? (uint32_t)*ea.step_dev : ea.step;
    constexpr int W = VEC ? 4 : 1;
    const int cols = io / W;
    const int r_begin = blockIdx.x * LOSS_ROWS;
    float wr = 0.f, sq = 0.f, sqp = 0.f;
    for (int cv = threadIdx.x; cv < cols; cv += NT) {
        const int c = cv * W;
        int psl[W];
        if constexpr (PRES) slots_of<W>(c, pa.E, psl);
        float cw[4] = {1.f, 1.f, 1.f, 1.f};
        if (ea.col_weight != nullptr) {
            if constexpr (VEC) {
                const float4 w4 = *reinterpret_cast<const float4*>(ea.col_weight + c);
                cw[0] = w4.x; cw[1] = w4.y; cw[2] = w4.z; cw[3] = w4.w;
            } else {
                cw[0] = ea.col_weight[c];
            }
        }
        float cs[4] = {0.f, 0.f, 0.f, 0.f};
        // rows as in mse_loss_kernel: clamped (always valid) addresses, rows past the batch contribute nothing
        for (int r0 = 0; r0 < LOSS_ROWS; r0 += LOSS_UNROLL)
#pragma unroll
        for (int ru = 0; ru < LOSS_UNROLL; ++ru) {
            const int rr = r0 + ru;
            const bool live = r_begin + rr < B;
            const int b = live ? r_begin + rr : B - 1;
            const int64_t src_row = ba.row_idx ? ba.row_idx[b] : b;
            float xv[4], yv[4];
            uint32_t m = 0x01010101u;
            const int id = !masked ? 0 : (ba.mask_id ? ba.mask_id[b] : ba.mask_to_use[src_row * ba.nb_run + ba.run]);
            if constexpr (VEC) {
                const float4 x4 = *reinterpret_cast<const float4*>(data + src_row * io + c);
                const float4 y4 = *reinterpret_cast<const float4*>(y + (int64_t)b * io + c);
                xv[0] = x4.x; xv[1] = x4.y; xv[2] = x4.z; xv[3] = x4.w;
                yv[0] = y4.x; yv[1] = y4.y; yv[2] = y4.z; yv[3] = y4.w;
                if (masked) m = *reinterpret_cast<const uint32_t*>(table + (int64_t)id * io + c);
            } else {
                xv[0] = data[src_row * io + c];
                yv[0] = y[(int64_t)b * io + c];
                if (masked) m = table[(int64_t)id * io + c];
            }
            bool hit[4] = {false, false, false, false};
            if (ea.replace) {
                if constexpr (VEC) hits4(hit, c, (uint32_t)src_row, step, ea);
                else hit[0] = hit1(c, (uint32_t)src_row, step, ea);
            }
            uint32_t pb = 0xfu;
            if constexpr (PRES) {
                pb = present_bits<W>(pa, src_row, psl);
#pragma unroll
                for (int k = 0; k < W; ++k)
                    if (!((pb >> k) & 1u)) { xv[k] = 0.f; yv[k] = 0.f; }
            }
            float g[4];
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const bool blank = ((m >> (8 * k)) & 0xff) == 0;
                const float w = live ? cw[k] * ((blank || hit[k]) ? ea.alpha : ea.beta) : 0.f;
                const float d = live ? xv[k] - yv[k] : 0.f;
                const float se = d * d;
                float rho, drho;
                rho_of<KIND>(d, ea, rho, drho);
                wr = opaque(wr + w * rho);
                sq = opaque(sq + se);
                if (blank) sqp = opaque(sqp + se);
                g[k] = -drho * opaque(w * inv_n);
                cs[k] = opaque(cs[k] + g[k]);
            }
            if constexpr (PRES) {      // (the stored gradient of an absent element is +0, not the product's -0)
#pragma unroll
                for (int k = 0; k < W; ++k) g[k] = ((pb >> k) & 1u) ? g[k] : 0.f;
            }
            if (live) {
                const int64_t o = (int64_t)b * dy_ld + c;
                if constexpr (DY_BF16) {
                    bf16_t* op = reinterpret_cast<bf16_t*>(dy) + o;
                    if constexpr (VEC) *reinterpret_cast<uint2*>(op) = pack_bf16x4(g[0], g[1], g[2], g[3]);
                    else op[0] = f32_to_bf16(g[0]);
                } else {
                    float* op = reinterpret_cast<float*>(dy) + o;
                    if constexpr (VEC) *reinterpret_cast<float4*>(op) = make_float4(g[0], g[1], g[2], g[3]);
                    else op[0] = g[0];
                }
            }
        }
        if (colsum_part) {
#pragma unroll
            for (int k = 0; k < W; ++k) colsum_part[(int64_t)blockIdx.x * io + c + k] = cs[k];
        }
    }
    const float bwr = block_sum(wr, red);
    const float bsq = block_sum(sq, red);
    const float bsqp = block_sum(sqp, red);
    if (threadIdx.x == 0) {
        parts[3 * blockIdx.x] = (double)bwr;
        parts[3 * blockIdx.x + 1] = (double)bsq;
        parts[3 * blockIdx.x + 2] = masked ? (double)bsqp : 0.0;
    }
}

// ---- per-slot cosine -------------------------------------------------------------------------------------------------------------
// Phase 1: wave v of the block takes the (row, slot) pairs p = v, v + 4, .. of its LOSS_ROWS x S; lane l the pieces of four
// columns j = l, l + 64, .. of the slot (columns ascending inside a piece, explicit fma): the order a pair's E products are added in
// depends on E alone - not on B, the block, the row's place in the batch, the dY type or whether the loads are 16-B or scalar -,
// which is what makes a shard's dY rows the bits of the same rows of the full batch.  Four butterfly reductions per pair (dot,
// |x|^2, |y|^2, sum w), then the pair's two coefficients go to LDS:
//   a = k / (nx ny),  b = k [|y| > eps] cos / |y|^2,  k = W / (rows S) = W E inv_n,  W = sum w / E
// Phase 2 (after one barrier): emph_loss_kernel's column-owner loop: g = -(a x - b y) + mse_weight 2 w (y - x) inv_n, dY, the column
// sums in registers, the squared-error sums.  x and y are read again (from L2: a block's rows are 2 x 32 x io x 4 B).
//   parts[block] = { mse_weight sum w d^2 + E sum W (1 - cos), sum d^2, sum (1-fmask) d^2 }
template <bool VEC1>
__device__ __forceinline__ void slot_pair_sums(const BatchArgs& ba, const float* __restrict__ y, const ReconArgs& ea, int b, int s,
                                               uint32_t step, float& dot, float& nx2, float& ny2, float& sw) {
    const int E = ea.E, io = ba.io;
    const int lane = threadIdx.x & 63;
    const bool masked = (ba.mask_id != nullptr) || (ba.mask_to_use != nullptr);
    const int64_t src_row = ba.row_idx ? ba.row_idx[b] : b;
    const int id = !masked ? 0 : (ba.mask_id ? ba.mask_id[b] : ba.mask_to_use[src_row * ba.nb_run + ba.run]);
    const float* __restrict__ xr = ba.data + src_row * io;
    const float* __restrict__ yr = y + (int64_t)b * io;
    const uint8_t* __restrict__ tr = ba.table + (int64_t)id * io;
    const bool weighted = ea.col_weight != nullptr || ea.replace || ea.alpha != ea.beta;
    dot = 0.f; nx2 = 0.f; ny2 = 0.f; sw = 0.f;
    const int pieces = (E + 3) >> 2;
    for (int j = lane; j < pieces; j += 64) {
        const int e0 = j * 4;
        const int c = s * E + e0;
        float xv[4] = {0.f, 0.f, 0.f, 0.f}, yv[4] = {0.f, 0.f, 0.f, 0.f}, wv[4] = {0.f, 0.f, 0.f, 0.f};
        if constexpr (VEC1) {      // E % 4 == 0: every piece is whole and starts a Philox group
            const float4 x4 = *reinterpret_cast<const float4*>(xr + c);
            const float4 y4 = *reinterpret_cast<const float4*>(yr + c);
            xv[0] = x4.x; xv[1] = x4.y; xv[2] = x4.z; xv[3] = x4.w;
            yv[0] = y4.x; yv[1] = y4.y; yv[2] = y4.z; yv[3] = y4.w;
            if (weighted) {
                float cw[4] = {1.f, 1.f, 1.f, 1.f};
                if (ea.col_weight != nullptr) {
                    const float4 w4 = *reinterpret_cast<const float4*>(ea.col_weight + c);
                    cw[0] = w4.x; cw[1] = w4.y; cw[2] = w4.z; cw[3] = w4.w;
                }
                const uint32_t m = masked ? *reinterpret_cast<const uint32_t*>(tr + c) : 0x01010101u;
                bool hit[4] = {false, false, false, false};
                if (ea.replace) hits4(hit, c, (uint32_t)src_row, step, ea);
#pragma unroll
                for (int k = 0; k < 4; ++k) wv[k] = cw[k] * ((((m >> (8 * k)) & 0xff) == 0 || hit[k]) ? ea.alpha : ea.beta);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) wv[k] = ea.beta;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (e0 + k < E) {
                    xv[k] = xr[c + k];
                    yv[k] = yr[c + k];
                    const float cw = ea.col_weight != nullptr ? ea.col_weight[c + k] : 1.f;
                    const bool blank = masked && tr[c + k] == 0;
                    const bool hit = ea.replace ? hit1(c + k, (uint32_t)src_row, step, ea) : false;
                    wv[k] = cw * ((blank || hit) ? ea.alpha : ea.beta);
                }
            }
        }
        // (columns past the slot's end add x = y = w = 0: exact, so the ragged piece changes no sum)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            dot = opaque(__fmaf_rn(xv[k], yv[k], dot));
            nx2 = opaque(__fmaf_rn(xv[k], xv[k], nx2));
            ny2 = opaque(__fmaf_rn(yv[k], yv[k], ny2));
            sw = opaque(sw + wv[k]);
        }
    }
    dot = wave_sum(dot); nx2 = wave_sum(nx2); ny2 = wave_sum(ny2); sw = wave_sum(sw);
}

// PRES: an absent pair is skipped in phase 1 - coefficients 0, no term, its x never read -, and phase 2 selects x = y = 0 for its
// columns as they are loaded and stores +0 (the table's slots are the criterion's: pa.S == ea.S).
template <bool VEC1, bool VEC, bool DY_BF16, bool PRES>
__global__ __launch_bounds__(NT) void slot_cosine_kernel(BatchArgs ba, const float* __restrict__ y, void* __restrict__ dy, float inv_n,
                                                         float* __restrict__ colsum_part, double* __restrict__ parts, int64_t dy_ld,
                                                         ReconArgs ea, PresArgs pa) {
    extern __shared__ float coef[];      // [LOSS_ROWS][S][2]
    __shared__ float red[WAVES];
    const float* __restrict__ data = ba.data;
    const uint8_t* __restrict__ table = ba.table;
    const int B = ba.B, io = ba.io, S = ea.S, E = ea.E;
    const bool masked = (ba.mask_id != nullptr) || (ba.mask_to_use != nullptr);
    const uint32_t step = ea.step_dev ? (uint32_t)*ea.step_dev : ea.step;
    const int r_begin = blockIdx.x * LOSS_ROWS;
    const int wave = threadIdx.x >> 6;
    const float k_scale = (float)E * inv_n;     // 1 / (rows S)

    // ---- phase 1
    float cos_terms = 0.f;                       // this wave's sum of W (1 - cos), its pairs in ascending order
    for (int p = wave; p < LOSS_ROWS * S; p += WAVES) {
        const int rr = p / S, s = p - rr * S;
        float a = 0.f, bq = 0.f;
        bool pair_on = r_begin + rr < B;         // (wave-uniform)
        if constexpr (PRES) {
            if (pair_on) {
                const int64_t prow = ba.row_idx ? ba.row_idx[r_begin + rr] : r_begin + rr;
                pair_on = pa.tab[prow * pa.S + s] != 0;
            }
        }
        if (pair_on) {
            float dot, nx2, ny2, sw;
            slot_pair_sums<VEC1>(ba, y, ea, r_begin + rr, s, step, dot, nx2, ny2, sw);
            const float nxr = sqrtf(nx2), nyr = sqrtf(ny2);
            const float nx = nxr < CODAE_COS_EPS ? CODAE_COS_EPS : nxr;     // max(., eps) that keeps a NaN norm a NaN
            const float ny = nyr < CODAE_COS_EPS ? CODAE_COS_EPS : nyr;
            const float nn = nx * ny;
            const float cs = dot / nn;
            const float Wp = sw / (float)E;
            const float k = Wp * k_scale;
            a = k / nn;
            bq = nyr > CODAE_COS_EPS ? opaque(k * cs) / ny2 : 0.f;
            cos_terms = opaque(cos_terms + Wp * opaque(1.f - cs));
        }
        if ((threadIdx.x & 63) == 0) { coef[2 * p] = a; coef[2 * p + 1] = bq; }
    }
    __syncthreads();

    // ---- phase 2
    const float mw = ea.mse_weight;
    const float mwin = mw * inv_n;
    constexpr int W = VEC ? 4 : 1;
    const int cols = io / W;
    float wsq = 0.f, sq = 0.f, sqp = 0.f;
    for (int cv = threadIdx.x; cv < cols; cv += NT) {
        const int c = cv * W;
        float cw[4] = {1.f, 1.f, 1.f, 1.f};
        int sl[4];
#pragma unroll
        for (int k = 0; k < W; ++k) sl[k] = (c + k) / E;
        if (mw != 0.f && ea.col_weight != nullptr) {
            if constexpr (VEC) {
                const float4 w4 = *reinterpret_cast<const float4*>(ea.col_weight + c);
                cw[0] = w4.x; cw[1] = w4.y; cw[2] = w4.z; cw[3] = w4.w;
            } else {
                cw[0] = ea.col_weight[c];
            }
        }
        float cs[4] = {0.f, 0.f, 0.f, 0.f};
        for (int r0 = 0; r0 < LOSS_ROWS; r0 += LOSS_UNROLL)
#pragma unroll
        for (int ru = 0; ru < LOSS_UNROLL; ++ru) {
            const int rr = r0 + ru;
            const bool live = r_begin + rr < B;
            const int b = live ? r_begin + rr : B - 1;
            const int64_t src_row = ba.row_idx ? ba.row_idx[b] : b;
            float xv[4], yv[4];
            uint32_t m = 0x01010101u;
            const int id = !masked ? 0 : (ba.mask_id ? ba.mask_id[b] : ba.mask_to_use[src_row * ba.nb_run + ba.run]);
            if constexpr (VEC) {
                const float4 x4 = *reinterpret_cast<const float4*>(data + src_row * io + c);
                const float4 y4 = *reinterpret_cast<const float4*>(y + (int64_t)b * io + c);
                xv[0] = x4.x; xv[1] = x4.y; xv[2] = x4.z; xv[3] = x4.w;
                yv[0] = y4.x; yv[1] = y4.y; yv[2] = y4.z; yv[3] = y4.w;
                if (masked) m = *reinterpret_cast<const uint32_t*>(table + (int64_t)id * io + c);
            } else {
                xv[0] = data[src_row * io + c];
                yv[0] = y[(int64_t)b * io + c];
                if (masked) m = table[(int64_t)id * io + c];
            }
            bool hit[4] = {false, false, false, false};
            if (mw != 0.f && ea.replace) {
                if constexpr (VEC) hits4(hit, c, (uint32_t)src_row, step, ea);
                else hit[0] = hit1(c, (uint32_t)src_row, step, ea);
            }
            uint32_t pb = 0xfu;
            if constexpr (PRES) {
                pb = present_bits<W>(pa, src_row, sl);
#pragma unroll
                for (int k = 0; k < W; ++k)
                    if (!((pb >> k) & 1u)) { xv[k] = 0.f; yv[k] = 0.f; }
            }
            float g[4];
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const bool blank = ((m >> (8 * k)) & 0xff) == 0;
                const float d = live ? xv[k] - yv[k] : 0.f;
                const float se = d * d;
                sq = opaque(sq + se);
                if (blank) sqp = opaque(sqp + se);
                const float a = coef[2 * (rr * S + sl[k])], bq = coef[2 * (rr * S + sl[k]) + 1];
                float gk = __fmaf_rn(bq, yv[k], -opaque(a * xv[k]));
                if (mw != 0.f) {
                    const float w = cw[k] * ((blank || hit[k]) ? ea.alpha : ea.beta);
                    wsq = opaque(wsq + w * se);
                    gk = __fmaf_rn(opaque(-2.f * d), opaque(w * mwin), gk);
                }
                g[k] = live ? gk : 0.f;
                cs[k] = opaque(cs[k] + g[k]);
            }
            if constexpr (PRES) {      // (the stored gradient of an absent element is +0 whatever sign its zero came out with)
#pragma unroll
                for (int k = 0; k < W; ++k) g[k] = ((pb >> k) & 1u) ? g[k] : 0.f;
            }
            if (live) {
                const int64_t o = (int64_t)b * dy_ld + c;
                if constexpr (DY_BF16) {
                    bf16_t* op = reinterpret_cast<bf16_t*>(dy) + o;
                    if constexpr (VEC) *reinterpret_cast<uint2*>(op) = pack_bf16x4(g[0], g[1], g[2], g[3]);
                    else op[0] = f32_to_bf16(g[0]);
                } else {
                    float* op = reinterpret_cast<float*>(dy) + o;
                    if constexpr (VEC) *reinterpret_cast<float4*>(op) = make_float4(g[0], g[1], g[2], g[3]);
                    else op[0] = g[0];
                }
            }
        }
        if (colsum_part) {
#pragma unroll
            for (int k = 0; k < W; ++k) colsum_part[(int64_t)blockIdx.x * io + c + k] = cs[k];
        }
    }
    // every lane of a wave holds the same cos_terms: count it once per wave
    const float bcos = block_sum((threadIdx.x & 63) == 0 ? cos_terms : 0.f, red);
    const float bwsq = block_sum(wsq, red);
    const float bsq = block_sum(sq, red);
    const float bsqp = block_sum(sqp, red);
    if (threadIdx.x == 0) {
        const double cos_part = (double)E * (double)bcos;
        parts[3 * blockIdx.x] = mw != 0.f ? (double)mw * (double)bwsq + cos_part : cos_part;
        parts[3 * blockIdx.x + 1] = (double)bsq;
        parts[3 * blockIdx.x + 2] = masked ? (double)bsqp : 0.0;
    }
}

inline bool a16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
bool finite_f(float x) { return x == x && fabsf(x) <= 3.402823466e38f; }

}  // namespace

int check_recon_loss(const codae_recon_loss* l, int io) {
    if (l == nullptr || l->kind == CODAE_LOSS_MSE) {
        CODAE_REQUIRE(l == nullptr || l->mse_weight == 0.f, "training criterion: mse_weight %g goes with slot_cosine only", (double)l->mse_weight);
        return CODAE_OK;
    }
    CODAE_REQUIRE(l->kind == CODAE_LOSS_L1 || l->kind == CODAE_LOSS_SMOOTH_L1 || l->kind == CODAE_LOSS_HUBER || l->kind == CODAE_LOSS_SLOT_COSINE,
                  "training criterion: unknown kind %d", l->kind);
    if (l->kind == CODAE_LOSS_SMOOTH_L1)
        CODAE_REQUIRE(finite_f(l->param) && l->param > 0.f, "training criterion: smooth_l1 beta %g must be finite and > 0", (double)l->param);
    if (l->kind == CODAE_LOSS_HUBER)
        CODAE_REQUIRE(finite_f(l->param) && l->param > 0.f, "training criterion: huber delta %g must be finite and > 0", (double)l->param);
    CODAE_REQUIRE(finite_f(l->mse_weight) && l->mse_weight >= 0.f, "training criterion: mse_weight %g must be finite and >= 0", (double)l->mse_weight);
    if (l->kind != CODAE_LOSS_SLOT_COSINE) {
        CODAE_REQUIRE(l->mse_weight == 0.f, "training criterion: mse_weight %g goes with slot_cosine only", (double)l->mse_weight);
        return CODAE_OK;
    }
    CODAE_REQUIRE(l->n_slots >= 1, "training criterion: slot_cosine needs n_slots >= 1, got %d", l->n_slots);
    CODAE_REQUIRE(io <= 0 || io % l->n_slots == 0, "training criterion: n_slots %d does not divide io %d", l->n_slots, io);
    if (l->n_slots > MAX_SLOTS) {
        set_error("training criterion: slot_cosine takes at most %d slots, got %d", MAX_SLOTS, l->n_slots);
        return CODAE_E_UNSUPPORTED;
    }
    return CODAE_OK;
}

int launch_recon_loss(const codae_batch* b, const codae_noise* noise, int32_t step, const double* step_dev, const codae_emphasis* emph,
                      const codae_recon_loss* loss, const float* y, void* dy, int dy_bf16, int64_t dy_ld, float inv_n, float* colsum_part,
                      double* parts, hipStream_t s, const uint8_t* present, int n_slots) {
    if (dy_ld <= 0) dy_ld = b ? b->io : 0;
    CODAE_REQUIRE(b && b->data && y && dy && parts && loss && b->B > 0 && b->io > 0, "recon_loss: bad args");
    int prc = check_presence(present, n_slots, b->io, "recon_loss");
    if (prc) return prc;
    CODAE_REQUIRE(present == nullptr || loss->kind != CODAE_LOSS_SLOT_COSINE || loss->n_slots == n_slots,
                  "recon_loss: slot_cosine n_slots %d differs from the presence table's %d", loss->n_slots, n_slots);
    const PresArgs pa{present, n_slots, present ? b->io / n_slots : 0};
    CODAE_REQUIRE(dy_ld >= b->io, "recon_loss: dy_ld %lld below io %d", (long long)dy_ld, b->io);
    int rc = check_recon_loss(loss, b->io);
    if (rc) return rc;
    CODAE_REQUIRE(loss->kind != CODAE_LOSS_MSE, "recon_loss: kind MSE runs on the mean-squared-error kernels (codae_emph_loss)");
    rc = check_emphasis(emph);
    if (rc) return rc;
    rc = check_noise(noise);
    if (rc) return rc;
    const bool masked = b->mask_id || b->mask_to_use;
    CODAE_REQUIRE(!masked || b->mask_table, "recon_loss: mask ids without mask_table");
    CODAE_REQUIRE(!b->mask_to_use || b->mask_id || (b->nb_run > 0 && b->run >= 0 && b->run < b->nb_run),
                  "recon_loss: run %d outside [0, %d)", b->run, b->nb_run);
    ReconArgs ea{};
    ea.alpha = 1.f; ea.beta = 1.f;
    if (emph != nullptr) { ea.alpha = emph->alpha; ea.beta = emph->beta; ea.col_weight = emph->col_weight; }
    ea.step = (uint32_t)step; ea.step_dev = step_dev;
    const bool weighted = emph != nullptr;      // without emphasis no element's weight depends on what the noise replaced
    if (weighted && noise != nullptr && (noise->kind == CODAE_NOISE_MASKING || noise->kind == CODAE_NOISE_SALT_PEPPER)) {
        ea.replace = 1;
        ea.key0 = (uint32_t)(noise->seed & 0xffffffffu); ea.key1 = (uint32_t)(noise->seed >> 32);
        ea.thresh = (uint64_t)floor((double)noise->p0 * 4294967296.0);      // (the gather's T)
    }
    ea.param = loss->param; ea.rparam = (loss->kind == CODAE_LOSS_SMOOTH_L1) ? (float)(1.0 / (double)loss->param) : 0.f;
    BatchArgs ba{b->data, b->row_idx, b->mask_id, b->mask_table, b->mask_to_use, b->nb_run, b->run, b->B, b->io};
    const bool in16 = a16(b->data) && a16(y) && (!ea.col_weight || a16(ea.col_weight)) &&
                      (!masked || (reinterpret_cast<uintptr_t>(b->mask_table) & 3) == 0);
    const bool vec = (b->io % 4 == 0) && (dy_ld % 4 == 0) && in16 && a16(dy);
    const int grid = mse_loss_colsum_rows(b->B);
    if (loss->kind == CODAE_LOSS_SLOT_COSINE) {
        ea.mse_weight = loss->mse_weight; ea.S = loss->n_slots; ea.E = b->io / loss->n_slots;
        const bool vec1 = (ea.E % 4 == 0) && in16;
        const size_t lds = (size_t)LOSS_ROWS * ea.S * 2 * sizeof(float);
#define SCP(V1, V, O, P) hipLaunchKernelGGL((slot_cosine_kernel<V1, V, O, P>), dim3(grid), dim3(NT), lds, s, ba, y, dy, inv_n, colsum_part, parts, dy_ld, ea, pa)
#define SC(V1, V, O) do { if (present) SCP(V1, V, O, true); else SCP(V1, V, O, false); } while (0)
        if (vec1) {
            if (vec && dy_bf16) SC(true, true, true);
            else if (vec) SC(true, true, false);
            else if (dy_bf16) SC(true, false, true);
            else SC(true, false, false);
        } else {
            if (vec && dy_bf16) SC(false, true, true);
            else if (vec) SC(false, true, false);
            else if (dy_bf16) SC(false, false, true);
            else SC(false, false, false);
        }
#undef SC
#undef SCP
    } else {
#define RLP(K, V, O, P) hipLaunchKernelGGL((recon_elem_kernel<K, V, O, P>), dim3(grid), dim3(NT), 0, s, ba, y, dy, inv_n, colsum_part, parts, dy_ld, ea, pa)
#define RL(K, V, O) do { if (present) RLP(K, V, O, true); else RLP(K, V, O, false); } while (0)
#define RK(K) do { if (vec && dy_bf16) RL(K, true, true); else if (vec) RL(K, true, false); else if (dy_bf16) RL(K, false, true); \
                   else RL(K, false, false); } while (0)
        if (loss->kind == CODAE_LOSS_L1) RK(CODAE_LOSS_L1);
        else if (loss->kind == CODAE_LOSS_SMOOTH_L1) RK(CODAE_LOSS_SMOOTH_L1);
        else RK(CODAE_LOSS_HUBER);
#undef RK
#undef RL
#undef RLP
    }
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

}  // namespace codae
