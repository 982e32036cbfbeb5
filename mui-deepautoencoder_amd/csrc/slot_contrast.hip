// Sampled-softmax slot contrast (codae_slot_contrast, include/codae_hip.h, "Slot contrast"): an additional training term behind
// the criterion's stand-alone kernel.  Per (row, slot) pair a softmax over the target slot and K sampled candidates of the same
// slot, all as unit vectors; attention-shaped: queries = the y^ rows, keys = values = the candidate matrix C^ [K][E].
//   slot_contrast_prepare_kernel<T>   one wave per candidate: Philox draw, gather of the clean slot, normalisation, written to the
//                                     work space in BOTH orders ([K][E] for the logits, [E][K] for the weighted sum) + its id
//   slot_contrast_kernel<T, MAXT, NH> one block per 32 batch rows, one wave per 16 of them, the slots in turn; two passes over the
//                                     candidate tiles (DESIGN.md section 6 "Slot contrast" says why two passes and not a rescaled one)
// T = the operand type of the two products: bf16 (v_mfma_f32_16x16x32_bf16) or float (v_mfma_f32_16x16x4_f32, an exact fmaf chain).
// A wave owns its 16 rows from the first load to the last store, and every reduction runs over a register / lane pattern that is
// the same for every row of a tile: a row's bits do not depend on its neighbours, on B or on the block it lands in.
#include <math.h>

#include <mutex>

#include "loss_sweep.h"

namespace codae {
namespace {

constexpr int NT = 128;          // two waves
constexpr int WAVES = 2;
constexpr int WROWS = 16;        // rows per wave = the MFMA's N
constexpr int BROWS = 32;        // rows per block = rows per partial column-sum row (mse_loss_colsum_rows)
constexpr int MAX_E = 1024;
constexpr int MAX_NEG = 4096;
constexpr int MAX_SLOTS = 128;
constexpr int PAD = 32;          // K and E are padded to multiples of this in the work space (zeros; pad logits are masked)
constexpr int NSC = 8;           // per-row scalars in LDS
// id of a candidate whose slot is absent in its dataset row ("Slot presence"): never kept by any pair, its vector stored as zeros.
// (item ids and dataset rows are >= 0; the pad candidates' -1 is never read under the k < K test.)
constexpr int32_t ABSENT_ID = INT32_MIN;

// keeps the loads of an unrolled loop where they are written: hoisted as a whole, the operand loads of 64 column tiles need more
// registers than the 256 accumulators leave
__device__ __forceinline__ void load_fence() { asm volatile("" ::: "memory"); }

// sum over the 16 lanes that share lane >> 4 (the 16 columns of an accumulator row)
__device__ __forceinline__ float sum16(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

struct ContrastArgs {
    int S, K, E, Kpad, Epad;
    float inv_tau;
    int n_rows;
    const int32_t* item_id;       // [S][n_rows] or null
    const void* cn;               // [S][Kpad][Epad] T
    const void* ct;               // [S][Epad][Kpad] T
    const int32_t* ids;           // [S][Kpad]
    const uint8_t* present;       // [n_rows][S] or null: slot presence of the batch rows (a uniform null test, no instantiation of its own)
};

struct PrepArgs {
    const float* data; int io, n_rows;
    int S, K, E, Kpad, Epad;
    const int32_t* pool; int P;
    const int32_t* item_id;
    uint32_t key0, key1, step;
    const double* step_dev;
    void* cn; void* ct; int32_t* ids;
    const uint8_t* present;       // [n_rows][S] or null
};

template <typename T> __device__ __forceinline__ T to_op(float v);
template <> __device__ __forceinline__ float to_op<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16_t to_op<bf16_t>(float v) { return f32_to_bf16(v); }
// v as the product will see it: rounded to the operand type
template <typename T> __device__ __forceinline__ float as_operand(float v) {
    if constexpr (sizeof(T) == 2) return bf16_to_f32(f32_to_bf16(v)); else return v;
}

// ---- prepare ---------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(64) void slot_contrast_prepare_kernel(PrepArgs a) {
    const int k = blockIdx.x, s = blockIdx.y, lane = threadIdx.x;
    T* __restrict__ cn = reinterpret_cast<T*>(a.cn) + ((int64_t)s * a.Kpad + k) * a.Epad;
    T* __restrict__ ct = reinterpret_cast<T*>(a.ct) + (int64_t)s * a.Epad * a.Kpad + k;
    if (k >= a.K) {       // pad candidates: zeros (never a NaN under the mask), id unused
        for (int e = lane; e < a.Epad; e += 64) { cn[e] = to_op<T>(0.f); ct[(int64_t)e * a.Kpad] = to_op<T>(0.f); }
        if (lane == 0) a.ids[s * a.Kpad + k] = -1;
        return;
    }
    const uint32_t step = a.step_dev ? (uint32_t)*a.step_dev : a.step;
    const uint4 r4 = philox4x32_10((uint32_t)(k >> 2), (uint32_t)s, step, 256u, a.key0, a.key1);
    const int w = k & 3;
    const uint32_t r = (w & 2) ? ((w & 1) ? r4.w : r4.z) : ((w & 1) ? r4.y : r4.x);
    const int j = (int)(((uint64_t)r * (uint64_t)a.P) >> 32);
    int row = a.pool ? a.pool[j] : j;
    row = row < 0 ? 0 : (row >= a.n_rows ? a.n_rows - 1 : row);      // (the host checks the pool; never read out of bounds)
    if (a.present != nullptr && a.present[(int64_t)row * a.S + s] == 0) {
        // an absent candidate: zeros in both orders - whatever data holds there (a NaN included) reaches no product - and the id
        // that no pair keeps.  The draw itself is the one a step without a table makes.
        for (int e = lane; e < a.Epad; e += 64) { cn[e] = to_op<T>(0.f); ct[(int64_t)e * a.Kpad] = to_op<T>(0.f); }
        if (lane == 0) a.ids[s * a.Kpad + k] = ABSENT_ID;
        return;
    }
    const float* __restrict__ src = a.data + (int64_t)row * a.io + s * a.E;
    float n2 = 0.f;
    for (int e = lane; e < a.E; e += 64) { const float v = src[e]; n2 = opaque(__fmaf_rn(v, v, n2)); }
    n2 = wave_sum(n2);
    const float nr = sqrtf(n2);
    const float nn = nr < CODAE_COS_EPS ? CODAE_COS_EPS : nr;
    for (int e = lane; e < a.Epad; e += 64) {
        const T v = to_op<T>(e < a.E ? src[e] / nn : 0.f);
        cn[e] = v;
        ct[(int64_t)e * a.Kpad] = v;
    }
    if (lane == 0) a.ids[s * a.Kpad + k] = a.item_id ? a.item_id[(int64_t)s * a.n_rows + row] : row;
}

// ---- the two products --------------------------------------------------------------------------------------------------------------
// logits_tile: Z^T tile = C^[c0 .. c0+15][:] . Q[16 rows][:]^T; lane l, register j: candidate c0 + 4 (l >> 4) + j, row l & 15.
// accumulate: G[16 rows][:] += P[16 rows][32 candidates] . C^[c0 .. c0+31][:], P handed over in the registers logits_tile left it
// in: the MFMA's k slots are numbered to fit (any numbering is right as long as A and B agree), so nothing crosses lanes.
template <typename T> struct Ops;

template <> struct Ops<bf16_t> {
    typedef bf16_t elem;
    static __device__ __forceinline__ f32x4 logits_tile(const bf16_t* __restrict__ cn, const bf16_t* q, int Epad, int qld, int c0, int lane) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const bf16_t* ap = cn + (int64_t)(c0 + (lane & 15)) * Epad + 8 * (lane >> 4);
        const bf16_t* bp = q + (lane & 15) * qld + 8 * (lane >> 4);
        for (int e0 = 0; e0 < Epad; e0 += 32) {
            const bf16x8 av = *reinterpret_cast<const bf16x8*>(ap + e0);
            const bf16x8 bv = *reinterpret_cast<const bf16x8*>(bp + e0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, acc, 0, 0, 0);
        }
        return acc;
    }
    template <int MAXT>
    static __device__ __forceinline__ void accumulate(f32x4 (&acc)[MAXT], const float* pa, const float* pb, const bf16_t* __restrict__ ct,
                                                      int Kpad, int nt, int c0, int lane) {
        // k slot (g, i): candidate c0 + 4 g + i for i < 4, c0 + 16 + 4 g + (i - 4) for i >= 4
        const u32x4 pw = {pack_bf16x2(pa[0], pa[1]), pack_bf16x2(pa[2], pa[3]), pack_bf16x2(pb[0], pb[1]), pack_bf16x2(pb[2], pb[3])};
        const bf16x8 av = __builtin_bit_cast(bf16x8, pw);
        const bf16_t* bp = ct + (int64_t)(lane & 15) * Kpad + c0 + 4 * (lane >> 4);
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
            if (t < nt) {
                const u32x2 lo = *reinterpret_cast<const u32x2*>(bp + (int64_t)t * 16 * Kpad);
                const u32x2 hi = *reinterpret_cast<const u32x2*>(bp + (int64_t)t * 16 * Kpad + 16);
                const u32x4 bw = {lo.x, lo.y, hi.x, hi.y};
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, __builtin_bit_cast(bf16x8, bw), acc[t], 0, 0, 0);
            }
            if ((t & 3) == 3) load_fence();
        }
    }
};

template <> struct Ops<float> {
    typedef float elem;
    static __device__ __forceinline__ f32x4 logits_tile(const float* __restrict__ cn, const float* q, int Epad, int qld, int c0, int lane) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const float* ap = cn + (int64_t)(c0 + (lane & 15)) * Epad + 4 * (lane >> 4);
        const float* bp = q + (lane & 15) * qld + 4 * (lane >> 4);
        for (int e0 = 0; e0 < Epad; e0 += 16) {      // k slot g of product i: column e0 + 4 g + i
            const float4 av = *reinterpret_cast<const float4*>(ap + e0);
            const float4 bv = *reinterpret_cast<const float4*>(bp + e0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc, 0, 0, 0);
        }
        return acc;
    }
    template <int MAXT>
    static __device__ __forceinline__ void accumulate(f32x4 (&acc)[MAXT], const float* pa, const float* pb, const float* __restrict__ ct,
                                                      int Kpad, int nt, int c0, int lane) {
        const float* bp = ct + (int64_t)(lane & 15) * Kpad + c0 + 4 * (lane >> 4);
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
            if (t < nt) {      // k slot g of product j: candidate c0 + 4 g + j, then the second 16 candidates
                const float4 b0 = *reinterpret_cast<const float4*>(bp + (int64_t)t * 16 * Kpad);
                const float4 b1 = *reinterpret_cast<const float4*>(bp + (int64_t)t * 16 * Kpad + 16);
                f32x4 c = acc[t];
                c = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[0], b0.x, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[1], b0.y, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[2], b0.z, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[3], b0.w, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x4f32(pb[0], b1.x, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x4f32(pb[1], b1.y, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x4f32(pb[2], b1.z, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x4f32(pb[3], b1.w, c, 0, 0, 0);
                acc[t] = c;
            }
            if ((t & 3) == 3) load_fence();
        }
    }
};

__device__ __forceinline__ float ex(float v) { return __expf(v); }

// ---- the contrast ----------------------------------------------------------------------------------------------------------------
// per-row scalars (LDS, one set per wave): 0 cos(x, y), 1 1 / max(|x|, eps), 2 1 / max(|y|, eps), 3 [|y| > eps] / (tau |y|), 4 W, 5 flags
// (1 = bad: a NaN or Inf in the y slot, 2 = no positive: |x| <= eps, 4 = a row of the batch, 8 = the slot is absent in this row:
// its x is never used - selected to 0, which makes it a pair without a positive), 6 1 - p0, 7 g . y^
template <typename T, int MAXT, int NH, bool SWAP = false>
__global__ __launch_bounds__(NT) void slot_contrast_kernel(BatchArgs ba, const float* __restrict__ y, T* __restrict__ dy, int64_t dy_ld,
                                                           float scale, float* __restrict__ colsum_part, double* __restrict__ parts,
                                                           ContrastArgs ca, WeightArgsOf<SWAP> ew) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int B = ba.B, io = ba.io, S = ca.S, K = ca.K, E = ca.E, Epad = ca.Epad, Kpad = ca.Kpad;
    const int qld = Epad + 16 / (int)sizeof(T);
    T* q = reinterpret_cast<T*>(smem) + wave * WROWS * qld;
    float* sc_base = reinterpret_cast<float*>(smem + (size_t)WAVES * WROWS * qld * sizeof(T));
    float* sc = sc_base + wave * WROWS * NSC;
    float* xch = sc_base + WAVES * WROWS * NSC;       // [WAVES][Epad] column sums of a slot, [WAVES] loss sums behind them
    float* lsum = xch + WAVES * Epad;
    const bool masked = (ba.mask_id != nullptr) || (ba.mask_to_use != nullptr);
    const bool weighted = ew.col_weight != nullptr || ew.replace || ew.alpha != ew.beta;
    const uint32_t step = ew.step_dev ? (uint32_t)*ew.step_dev : ew.step;
    const int r_begin = blockIdx.x * BROWS + wave * WROWS;
    const bool wave_live = r_begin < B;
    const int nt = (E + 15) >> 4;
    const float inv_tau = ca.inv_tau;
    // this lane's row as a logit column (r16), and its dataset row
    const bool my_live = r_begin + r16 < B;
    const int my_b = my_live ? r_begin + r16 : B - 1;
    const int my_src = ba.row_idx ? ba.row_idx[my_b] : my_b;
    float wave_loss = 0.f;

    for (int s = 0; s < S; ++s) {
        if (wave_live) {
            const int my_id = ca.item_id ? ca.item_id[(int64_t)s * ca.n_rows + my_src] : my_src;
            // ---- per-row sums, y^ into LDS: the whole wave on one row at a time, columns lane, lane + 64, .. (order: E alone)
            for (int rr = 0; rr < WROWS; ++rr) {
                const bool live = r_begin + rr < B;
                const int b = live ? r_begin + rr : B - 1;
                const int64_t src_row = ba.row_idx ? ba.row_idx[b] : b;
                const int id = !masked ? 0 : (ba.mask_id ? ba.mask_id[b] : ba.mask_to_use[src_row * ba.nb_run + ba.run]);
                const float* __restrict__ xr = ba.data + src_row * io + s * E;
                const float* __restrict__ yr = y + (int64_t)b * io + s * E;
                const bool absent = ca.present != nullptr && ca.present[src_row * S + s] == 0;     // (wave-uniform)
                float dot = 0.f, nx2 = 0.f, ny2 = 0.f, sw = 0.f;
                // swap noise: the pair's own draw when the swap's slots are the contrast's, else a draw per column
                bool swap_pair = false, pair_hit = false;
                if constexpr (SWAP) {
                    swap_pair = ew.sw.E == E;
                    pair_hit = weighted && swap_pair && swap_source(ew.sw, (uint32_t)src_row, s, step) >= 0;
                }
                for (int e = lane; e < E; e += 64) {
                    const float xv = absent ? 0.f : xr[e], yv = yr[e];
                    float w = ew.beta;
                    if (weighted) {
                        const int c = s * E + e;
                        const float cw = ew.col_weight != nullptr ? ew.col_weight[c] : 1.f;
                        const bool blank = masked && ba.table[(int64_t)id * io + c] == 0;
                        bool hit;
                        if constexpr (SWAP) hit = swap_pair ? pair_hit : swap_hit1(c, (uint32_t)src_row, step, ew.sw);
                        else hit = ew.replace ? hit1(c, (uint32_t)src_row, step, ew) : false;
                        w = cw * ((blank || hit) ? ew.alpha : ew.beta);
                    }
                    dot = opaque(__fmaf_rn(xv, yv, dot));
                    nx2 = opaque(__fmaf_rn(xv, xv, nx2));
                    ny2 = opaque(__fmaf_rn(yv, yv, ny2));
                    sw = opaque(sw + w);
                }
                dot = wave_sum(dot); nx2 = wave_sum(nx2); ny2 = wave_sum(ny2); sw = wave_sum(sw);
                const float nxr = sqrtf(nx2), nyr = sqrtf(ny2);
                const float nx = nxr < CODAE_COS_EPS ? CODAE_COS_EPS : nxr;
                const float ny = nyr < CODAE_COS_EPS ? CODAE_COS_EPS : nyr;
                const bool bad = !(ny2 - ny2 == 0.f);          // NaN or Inf somewhere in the slot (or squares past fp32)
                const bool nopos = !(nxr > CODAE_COS_EPS);
                const float iny = 1.f / ny;
                for (int e = lane; e < Epad; e += 64) q[rr * qld + e] = to_op<T>((e < E && !bad) ? yr[e] * iny : 0.f);
                if (lane == 0) {
                    sc[rr * NSC + 0] = dot / (nx * ny);
                    sc[rr * NSC + 1] = 1.f / nx;
                    sc[rr * NSC + 2] = iny;
                    sc[rr * NSC + 3] = nyr > CODAE_COS_EPS ? inv_tau / nyr : 0.f;
                    sc[rr * NSC + 4] = live ? sw / (float)E : 0.f;
                    sc[rr * NSC + 5] = __int_as_float((bad ? 1 : 0) | (nopos ? 2 : 0) | (live ? 4 : 0) | (absent ? 8 : 0));
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const float cos0 = sc[r16 * NSC + 0];
            const float z0 = cos0 * inv_tau;
            const int my_flags = __float_as_int(sc[r16 * NSC + 5]);
            const T* __restrict__ cn = reinterpret_cast<const T*>(ca.cn) + (int64_t)s * Kpad * Epad;
            const T* __restrict__ ct = reinterpret_cast<const T*>(ca.ct) + (int64_t)s * Epad * Kpad;
            const int32_t* __restrict__ ids = ca.ids + s * Kpad;

            // ---- pass 1: running maximum and sum of the kept logits, per lane, then over the four lanes of the row.
            // (compares and selects, never fmaxf: a NaN logit cannot hide; a bad row is made NaN explicitly below anyway)
            float m = -INFINITY, sum = 0.f;
            for (int c0 = 0; c0 < Kpad; c0 += 16) {
                const f32x4 z = Ops<T>::logits_tile(cn, q, Epad, qld, c0, lane);
                const int4 id4 = *reinterpret_cast<const int4*>(ids + c0 + 4 * g);
                const int idv[4] = {id4.x, id4.y, id4.z, id4.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool keep = (c0 + 4 * g + j < K) && idv[j] != my_id && idv[j] != ABSENT_ID;
                    const float zz = z[j] * inv_tau;
                    if (keep) {
                        if (zz > m) { sum = opaque(sum * ex(m - zz)) + 1.f; m = zz; }     // (m = -inf, sum = 0: 0 * 0 + 1)
                        else sum = sum + ex(zz - m);
                    }
                }
            }
#pragma unroll
            for (int o = 16; o <= 32; o <<= 1) {
                const float m1 = __shfl_xor(m, o), s1 = __shfl_xor(sum, o);
                const float M = m1 > m ? m1 : m;
                const float ta = sum > 0.f ? sum * ex(m - M) : 0.f, tb = s1 > 0.f ? s1 * ex(m1 - M) : 0.f;
                sum = ta + tb;      // (commutative: both partners get the same bits)
                m = M;
            }
            const float M = z0 > m ? z0 : m;           // (a NaN z0 fails the compare: M = m, and lse below is NaN through z0)
            const float rest = sum > 0.f ? sum * ex(m - M) : 0.f;
            const float total = rest + ex(z0 - M);
            float lse = M + __logf(total);
            float l = lse - z0;
            // 1 - p_0 as the kept share of the total, not as 1 - exp(z_0 - lse): a pair that is already ranked first has p_0 within
            // an ulp of 1 and the difference would keep no bits of what its gradient is proportional to
            float omp0 = rest / total;
            if (my_flags & 2) { l = 0.f; omp0 = 0.f; lse = INFINITY; }       // no positive: every p_k = 0, g = 0
            if (my_flags & 1) l = __int_as_float(0x7fc00000);
            if (g == 0) sc[r16 * NSC + 6] = omp0;

            // ---- pass 2: p_k from the logits again, G = P C^; NH > 1: the slot's columns in NH ranges of MAXT tiles, the logits formed
            // once per range (the accumulators of 64 tiles and everything else do not fit 512 registers).
            // g . y^ = sum_kept p_k cos_k - (1 - p_0) cos_0 comes from the logits themselves, with the p_k as the product sees them.
            float* xw = xch + wave * Epad;
#pragma unroll 1
            for (int h = 0; h < NH; ++h) {
                const int t0 = h * MAXT;
                const int nth = nt - t0 < MAXT ? nt - t0 : MAXT;
                if (nth <= 0) break;
                f32x4 acc[MAXT];
#pragma unroll
                for (int t = 0; t < MAXT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
                float pz = 0.f;
                const T* __restrict__ cth = ct + (int64_t)t0 * 16 * Kpad;
                for (int c0 = 0; c0 < Kpad; c0 += 32) {
                    const f32x4 za = Ops<T>::logits_tile(cn, q, Epad, qld, c0, lane);
                    const f32x4 zb = Ops<T>::logits_tile(cn, q, Epad, qld, c0 + 16, lane);
                    const int4 ia = *reinterpret_cast<const int4*>(ids + c0 + 4 * g);
                    const int4 ib = *reinterpret_cast<const int4*>(ids + c0 + 16 + 4 * g);
                    const int iav[4] = {ia.x, ia.y, ia.z, ia.w}, ibv[4] = {ib.x, ib.y, ib.z, ib.w};
                    float pa[4], pb[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool ka = (c0 + 4 * g + j < K) && iav[j] != my_id && iav[j] != ABSENT_ID;
                        const bool kb = (c0 + 16 + 4 * g + j < K) && ibv[j] != my_id && ibv[j] != ABSENT_ID;
                        pa[j] = as_operand<T>(ka ? ex(za[j] * inv_tau - lse) : 0.f);
                        pb[j] = as_operand<T>(kb ? ex(zb[j] * inv_tau - lse) : 0.f);
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) pz = opaque(__fmaf_rn(pa[j], za[j], pz));
#pragma unroll
                    for (int j = 0; j < 4; ++j) pz = opaque(__fmaf_rn(pb[j], zb[j], pz));
                    Ops<T>::template accumulate<MAXT>(acc, pa, pb, cth, Kpad, nth, c0, lane);
                }
                if (h == 0) {
                    pz += __shfl_xor(pz, 16);
                    pz += __shfl_xor(pz, 32);
                    if (g == 0) sc[r16 * NSC + 7] = __fmaf_rn(-omp0, cos0, pz);
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }

                // ---- epilogue: lane (r16, g), register j of tile t = row 4 g + j, column 16 (t0 + t) + r16
                float inx[4], iny[4], dls[4], kw[4], omp0r[4], gy[4];
                int fl[4]; int64_t xoff[4], yoff[4], doff[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int rr = 4 * g + j;
                    inx[j] = sc[rr * NSC + 1]; iny[j] = sc[rr * NSC + 2]; dls[j] = sc[rr * NSC + 3];
                    kw[j] = scale * sc[rr * NSC + 4];
                    fl[j] = __float_as_int(sc[rr * NSC + 5]);
                    omp0r[j] = sc[rr * NSC + 6];
                    gy[j] = sc[rr * NSC + 7];
                    const int b = (fl[j] & 4) ? r_begin + rr : B - 1;
                    const int64_t src_row = ba.row_idx ? ba.row_idx[b] : b;
                    xoff[j] = src_row * io + s * E; yoff[j] = (int64_t)b * io + s * E; doff[j] = (int64_t)b * dy_ld + s * E;
                }
#pragma unroll
                for (int t = 0; t < MAXT; ++t) {
                    if (t < nth) {
                        const int e = 16 * (t0 + t) + r16;
                        const int ec = e < E ? e : E - 1;
                        float cs = 0.f;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const bool live = (fl[j] & 4) && e < E;
                            const float xh = (fl[j] & 8) ? 0.f : ba.data[xoff[j] + ec] * inx[j];
                            const float yh = y[yoff[j] + ec] * iny[j];
                            const float ge = opaque(__fmaf_rn(-omp0r[j], xh, acc[t][j]));
                            const float dl = opaque(__fmaf_rn(-gy[j], yh, ge)) * dls[j];
                            float stored = 0.f;
                            if (live) {
                                T* op = dy + doff[j] + e;
                                float v;
                                if constexpr (sizeof(T) == 2) v = bf16_to_f32(*op); else v = *op;
                                v = __fmaf_rn(kw[j], dl, v);
                                if (fl[j] & 1) v = __int_as_float(0x7fc00000);
                                const T o = to_op<T>(v);
                                *op = o;
                                if constexpr (sizeof(T) == 2) stored = bf16_to_f32(o); else stored = o;
                            }
                            cs = opaque(cs + stored);
                        }
                        cs += __shfl_xor(cs, 16);
                        cs += __shfl_xor(cs, 32);
                        if (g == 0 && e < E) xw[e] = cs;
                    }
                    load_fence();
                }
            }
            // the wave's share of sum W l: its 16 rows added by a butterfly over the lanes that hold them (a fixed order)
            float wl = 0.f;
            if (g == 0) {
                const float Wr = sc[r16 * NSC + 4];
                wl = (my_flags & 4) ? ((my_flags & 1) ? l : Wr * l) : 0.f;
            }
            wl = sum16(wl);
            wave_loss = opaque(wave_loss + __shfl(wl, 0));
        } else if (g == 0) {
            for (int e = r16; e < E; e += 16) xch[wave * Epad + e] = 0.f;
        }
        __syncthreads();
        if (colsum_part != nullptr)
            for (int e = threadIdx.x; e < E; e += NT) colsum_part[(int64_t)blockIdx.x * io + s * E + e] = xch[e] + xch[Epad + e];
        __syncthreads();
    }
    if (lane == 0) lsum[wave] = wave_loss;
    __syncthreads();
    if (threadIdx.x == 0) parts[blockIdx.x] = (double)lsum[0] + (double)lsum[1];
}

// LAST_LOSS += scale * sum parts, in index order (one thread: a few hundred doubles)
__global__ void slot_contrast_finish_kernel(double* __restrict__ scalars, double scale, const double* __restrict__ parts, int n) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double t = 0.0;
    for (int i = 0; i < n; ++i) t += parts[i];
    scalars[CODAE_S_LAST_LOSS] += scale * t;
}

struct WsLayout { int Kpad, Epad; int64_t cn_off, ct_off, ids_off, bytes; };
WsLayout ws_layout(int S, int K, int E, int bf16) {
    WsLayout w;
    w.Kpad = (int)round_up(K, PAD); w.Epad = (int)round_up(E, PAD);
    const int64_t mat = (int64_t)S * w.Kpad * w.Epad * (bf16 ? 2 : 4);
    w.cn_off = 0; w.ct_off = mat; w.ids_off = 2 * mat;
    w.bytes = 2 * mat + (int64_t)S * w.Kpad * 4;
    return w;
}

// more than the default 64 KiB of dynamic LDS (fp32 operands, E = 1024: 134 KiB).  The attribute belongs to the CURRENT device's copy
// of a kernel: asked for once per device, for every instantiation, under a lock (engines on several GPUs, or set up from several
// host threads, share this table)
int raise_lds() {
    constexpr int MAX_DEV = 64;
    static std::mutex lock;
    static bool raised[MAX_DEV] = {};
    int dev = 0;
    CODAE_HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> hold(lock);
    if (dev >= 0 && dev < MAX_DEV && raised[dev]) return CODAE_OK;
#define RAISE1(T, M, H, W) CODAE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&slot_contrast_kernel<T, M, H, W>), \
                                                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024))
#define RAISE(T, M, H) RAISE1(T, M, H, false); RAISE1(T, M, H, true)
    RAISE(bf16_t, 8, 1); RAISE(bf16_t, 32, 1); RAISE(bf16_t, 32, 2); RAISE(float, 8, 1); RAISE(float, 32, 1); RAISE(float, 32, 2);
#undef RAISE
#undef RAISE1
    if (dev >= 0 && dev < MAX_DEV) raised[dev] = true;
    return CODAE_OK;
}

template <typename T, int MAXT, int NH>
int launch_one(int grid, size_t lds, hipStream_t s, const BatchArgs& ba, const float* y, void* dy, int64_t dy_ld, float scale,
               float* colsum_part, double* parts, const ContrastArgs& ca, const SwapWeightArgs& ew) {
    swap_dispatch(ew, [&](auto W) {
        hipLaunchKernelGGL((slot_contrast_kernel<T, MAXT, NH, decltype(W)::value>), dim3(grid), dim3(NT), lds, s, ba, y, reinterpret_cast<T*>(dy),
                           dy_ld, scale, colsum_part, parts, ca, weight_args_of<decltype(W)::value>(ew));
    });
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

}  // namespace

int64_t slot_contrast_ws_bytes(int S, int K, int E, int bf16) {
    if (S < 1 || S > MAX_SLOTS || K < 1 || K > MAX_NEG || E < 1 || E > MAX_E) return -1;
    return ws_layout(S, K, E, bf16).bytes;
}

int check_slot_contrast(const codae_slot_contrast* c, int io, int bf16) {
    if (c == nullptr) return CODAE_OK;
    CODAE_REQUIRE(finite_f(c->weight) && c->weight >= 0.f, "slot contrast: weight %g must be finite and >= 0", (double)c->weight);
    if (c->weight == 0.f) return CODAE_OK;          // off: nothing else is read
    CODAE_REQUIRE(c->n_neg >= 1 && c->n_neg <= MAX_NEG, "slot contrast: n_neg %d outside [1, %d]", c->n_neg, MAX_NEG);
    CODAE_REQUIRE(finite_f(c->tau) && c->tau >= 0.01f, "slot contrast: tau %g must be finite and >= 0.01", (double)c->tau);
    CODAE_REQUIRE(c->n_slots >= 1 && c->n_slots <= MAX_SLOTS, "slot contrast: n_slots %d outside [1, %d]", c->n_slots, MAX_SLOTS);
    CODAE_REQUIRE(io <= 0 || io % c->n_slots == 0, "slot contrast: n_slots %d does not divide io %d", c->n_slots, io);
    CODAE_REQUIRE(c->n_rows >= 1, "slot contrast: n_rows %d must be >= 1", c->n_rows);
    CODAE_REQUIRE(c->pool == nullptr ? c->n_pool == 0 || c->n_pool == c->n_rows : c->n_pool >= 1,
                  "slot contrast: n_pool %d (a pool needs at least one row; without one it is 0 or n_rows)", c->n_pool);
    if (io > 0) {
        const int E = io / c->n_slots;
        if (E > MAX_E) {
            set_error("slot contrast: E = %d columns per slot, at most %d are supported", E, MAX_E);
            return CODAE_E_UNSUPPORTED;
        }
        const int64_t need = ws_layout(c->n_slots, c->n_neg, E, bf16).bytes;
        CODAE_REQUIRE(c->ws != nullptr && a16(c->ws), "slot contrast: ws missing or not 16-byte aligned");
        CODAE_REQUIRE(c->ws_bytes >= need, "slot contrast: ws of %lld bytes, %lld needed", (long long)c->ws_bytes, (long long)need);
    }
    return CODAE_OK;
}

int slot_contrast_warm() { return raise_lds(); }

int launch_slot_contrast_prepare(const float* data, int io, const codae_slot_contrast* c, int32_t step, const double* step_dev, int bf16,
                                 hipStream_t s, const uint8_t* present, int n_slots) {
    CODAE_REQUIRE(data != nullptr && c != nullptr && io > 0 && c->weight != 0.f, "slot contrast prepare: bad args");
    int rc = check_slot_contrast(c, io, bf16);
    if (rc) return rc;
    rc = check_presence(present, n_slots, io, "slot contrast prepare");
    if (rc) return rc;
    CODAE_REQUIRE(present == nullptr || n_slots == c->n_slots, "slot contrast prepare: n_slots %d differs from the presence table's %d",
                  c->n_slots, n_slots);
    const int E = io / c->n_slots;
    const WsLayout w = ws_layout(c->n_slots, c->n_neg, E, bf16);
    PrepArgs a{};
    a.data = data; a.io = io; a.n_rows = c->n_rows; a.S = c->n_slots; a.K = c->n_neg; a.E = E; a.Kpad = w.Kpad; a.Epad = w.Epad;
    a.pool = c->pool; a.P = c->pool ? c->n_pool : c->n_rows; a.item_id = c->item_id;
    a.key0 = (uint32_t)(c->seed & 0xffffffffu); a.key1 = (uint32_t)(c->seed >> 32); a.step = (uint32_t)step; a.step_dev = step_dev;
    unsigned char* base = reinterpret_cast<unsigned char*>(c->ws);
    a.cn = base + w.cn_off; a.ct = base + w.ct_off; a.ids = reinterpret_cast<int32_t*>(base + w.ids_off);
    a.present = present;
    if (bf16) hipLaunchKernelGGL(slot_contrast_prepare_kernel<bf16_t>, dim3(w.Kpad, a.S), dim3(64), 0, s, a);
    else hipLaunchKernelGGL(slot_contrast_prepare_kernel<float>, dim3(w.Kpad, a.S), dim3(64), 0, s, a);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_slot_contrast(const LossLaunch& ll, const codae_slot_contrast* c, hipStream_t s) {
    CODAE_REQUIRE(c && c->weight != 0.f, "slot contrast: bad args");
    int rc = check_loss_launch("slot contrast", ll, true);
    if (rc) return rc;
    const codae_batch* b = ll.batch;
    const float* y = ll.y;
    void* dy = ll.dy;
    const int dy_bf16 = ll.dy_bf16;
    const int64_t dy_ld = loss_dy_ld(ll);
    CODAE_REQUIRE(ll.present == nullptr || ll.n_slots == c->n_slots, "slot contrast: n_slots %d differs from the presence table's %d",
                  c->n_slots, ll.n_slots);
    CODAE_REQUIRE(finite_f(ll.scale), "slot contrast: scale %g is not finite", (double)ll.scale);
    rc = check_slot_contrast(c, b->io, dy_bf16);
    if (rc) return rc;
    const SwapWeightArgs ew = weight_args(ll, ll.emph != nullptr);
    const int E = b->io / c->n_slots;
    const WsLayout w = ws_layout(c->n_slots, c->n_neg, E, dy_bf16);
    ContrastArgs ca{};
    ca.S = c->n_slots; ca.K = c->n_neg; ca.E = E; ca.Kpad = w.Kpad; ca.Epad = w.Epad;
    ca.inv_tau = (float)(1.0 / (double)c->tau); ca.n_rows = c->n_rows; ca.item_id = c->item_id;
    const unsigned char* base = reinterpret_cast<const unsigned char*>(c->ws);
    ca.cn = base + w.cn_off; ca.ct = base + w.ct_off; ca.ids = reinterpret_cast<const int32_t*>(base + w.ids_off);
    ca.present = ll.present;
    const BatchArgs ba = batch_args(b);
    const int es = dy_bf16 ? 2 : 4;
    const size_t lds = (size_t)WAVES * WROWS * (w.Epad + 16 / es) * es + (size_t)(WAVES * WROWS * NSC + WAVES * w.Epad + WAVES) * 4;
    rc = raise_lds();
    if (rc) return rc;
    const int grid = slot_contrast_blocks(b->B);
    const int nt = (E + 15) / 16;
#define SCK(T, M, H) return launch_one<T, M, H>(grid, lds, s, ba, y, dy, dy_ld, ll.scale, ll.colsum_part, ll.parts, ca, ew)
    if (dy_bf16) { if (nt <= 8) SCK(bf16_t, 8, 1); if (nt <= 32) SCK(bf16_t, 32, 1); SCK(bf16_t, 32, 2); }
    if (nt <= 8) SCK(float, 8, 1);
    if (nt <= 32) SCK(float, 32, 1);
    SCK(float, 32, 2);
#undef SCK
}

int launch_slot_contrast_finish(double* scalars, double scale, const double* parts, int n_parts, hipStream_t s) {
    hipLaunchKernelGGL(slot_contrast_finish_kernel, dim3(1), dim3(64), 0, s, scalars, scale, parts, n_parts);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

}  // namespace codae
