// What the stand-alone loss kernels share (elementwise.hip: mse_loss_kernel, emph_loss_kernel; recon_loss.hip: recon_elem_kernel,
// slot_cosine_kernel; slot_contrast.hip takes the helpers): the block reductions, the argument structs, the Philox "replaced" test,
// and loss_sweep - the column-owner row sweep that forms dY from y - with the per-element arithmetic as a policy (a "term").
//   new arithmetic (a criterion, a weight rule)   -> a term
//   anything that touches the loads or the stores -> loss_sweep, once for every kernel
#pragma once
#include <math.h>

#include "codae_common.h"

namespace codae {

constexpr int LOSS_NT = 256;    // threads per block of the sweeping kernels
constexpr int LOSS_ROWS = 32;   // rows per block = rows per partial column-sum row (mse_loss_colsum_rows)
constexpr int LOSS_UNROLL = 8;  // rows in flight per thread

inline bool a16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool finite_f(float x) { return x == x && fabsf(x) <= 3.402823466e38f; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// sum over a 256-thread block, the waves' sums added in wave order; result valid in thread 0
__device__ __forceinline__ float block_sum(float v, float* red /*[4]*/) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[w] = v;
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

struct BatchArgs {
    const float* data; const int32_t* row_idx; const int32_t* mask_id; const uint8_t* table; const int32_t* mask_to_use;
    int nb_run, run, B, io;
};

// The emphasis weight of an element (codae_emphasis, include/codae_hip.h; Vincent et al. 2010, section 4.3):
//   w = col_weight[c] * (corrupted ? alpha : beta),  corrupted = blanked by the slot mask OR replaced by the input noise
// alpha = beta = 1 and no column weights when emphasis is off.  "replaced" is recomputed from the element's Philox word (the
// gather's counter: column / 4, DATASET row, step), one call per four columns; nothing is read back from the noised input.
struct WeightArgs {
    float alpha, beta;
    const float* col_weight;   // [io] or null (all ones)
    int replace;               // 1: the input noise is MASKING or SALT_PEPPER: a word below thresh marks a replaced element
                               // 2: SWAP: every element of a slot whose swap was accepted (SwapWeightArgs::sw; one word per (row, slot))
    uint64_t thresh;           // T = floor(p 2^32)
    uint32_t key0, key1;
    uint32_t step;             // counter word 2 ...
    const double* step_dev;    // ... or, when not null, *step_dev (graph replay)
};
constexpr int REPLACE_ELEMS = 1, REPLACE_SWAP = 2;
// the SWAP instantiations take the draw's arguments behind the weights; every other instantiation keeps the argument block it had
struct SwapWeightArgs : WeightArgs {
    SwapArgs sw;               // replace == REPLACE_SWAP
};
template <bool SWAP>
using WeightArgsOf = std::conditional_t<SWAP, SwapWeightArgs, WeightArgs>;
template <bool SWAP>
inline WeightArgsOf<SWAP> weight_args_of(const SwapWeightArgs& a) { return a; }

// which of the four columns c .. c + 3 of dataset row `row` the gather's noise replaced (c a multiple of 4: one Philox group)
__device__ __forceinline__ void hits4(bool* hit, int c, uint32_t row, uint32_t step, const WeightArgs& a) {
    const uint4 r = philox4x32_10((uint32_t)(c >> 2), row, step, 0u, a.key0, a.key1);
    hit[0] = (uint64_t)r.x < a.thresh; hit[1] = (uint64_t)r.y < a.thresh;
    hit[2] = (uint64_t)r.z < a.thresh; hit[3] = (uint64_t)r.w < a.thresh;
}
// the same for the single column c (word c % 4 of its group; selects, no indexed register array)
__device__ __forceinline__ bool hit1(int c, uint32_t row, uint32_t step, const WeightArgs& a) {
    const uint4 r = philox4x32_10((uint32_t)(c >> 2), row, step, 0u, a.key0, a.key1);
    const int k = c & 3;
    const uint32_t rk = (k & 2) ? ((k & 1) ? r.w : r.z) : ((k & 1) ? r.y : r.x);
    return (uint64_t)rk < a.thresh;
}

// Swap noise: which of the W columns whose swap slots are ssl[0 .. W) (slots_of with the swap's E, formed once per thread) sit in a
// slot of dataset row `row` that took an accepted swap: one Philox call per slot the group touches
template <int W>
__device__ __forceinline__ void swap_hits(bool* hit, const int* ssl, uint32_t row, uint32_t step, const SwapArgs& sw) {
    hit[0] = swap_source(sw, row, ssl[0], step) >= 0;
#pragma unroll
    for (int k = 1; k < W; ++k) hit[k] = ssl[k] == ssl[k - 1] ? hit[k - 1] : swap_source(sw, row, ssl[k], step) >= 0;
}
// the same for the single column c of a kernel that walks a slot's columns (slot_cosine's phase 1, the slot contrast)
__device__ __forceinline__ bool swap_hit1(int c, uint32_t row, uint32_t step, const SwapArgs& sw) {
    return swap_source(sw, row, c / sw.E, step) >= 0;
}

// ---- host side: what the launchers make of a LossLaunch ----------------------------------------------------------------------------
inline BatchArgs batch_args(const codae_batch* b) {
    return BatchArgs{b->data, b->row_idx, b->mask_id, b->mask_table, b->mask_to_use, b->nb_run, b->run, b->B, b->io};
}
inline PresArgs pres_args(const LossLaunch& ll) {
    return PresArgs{ll.present, ll.n_slots, ll.present ? ll.batch->io / ll.n_slots : 0};
}
// weighted: an element's weight may depend on what the input noise replaced (without emphasis no weight does)
inline SwapWeightArgs weight_args(const LossLaunch& ll, bool weighted) {
    SwapWeightArgs wa{};
    wa.alpha = 1.f; wa.beta = 1.f;
    if (ll.emph != nullptr) { wa.alpha = ll.emph->alpha; wa.beta = ll.emph->beta; wa.col_weight = ll.emph->col_weight; }
    wa.step = (uint32_t)ll.step; wa.step_dev = ll.step_dev;
    const codae_noise* n = ll.noise;
    if (weighted && n != nullptr && n->kind == CODAE_NOISE_SWAP) {      // (check_loss_launch has seen ll.swap)
        wa.replace = REPLACE_SWAP;
        wa.sw = swap_args(n, ll.swap, ll.batch->io, ll.present);
    }
    if (weighted && n != nullptr && (n->kind == CODAE_NOISE_MASKING || n->kind == CODAE_NOISE_SALT_PEPPER)) {
        wa.replace = REPLACE_ELEMS;
        wa.key0 = (uint32_t)(n->seed & 0xffffffffu); wa.key1 = (uint32_t)(n->seed >> 32);
        wa.thresh = (uint64_t)floor((double)n->p0 * 4294967296.0);      // (the gather's T)
    }
    return wa;
}
// x, y and the mask rows can be read 16 (4) bytes at a time; each launcher adds dy and the column weights on its own terms
inline bool loss_inputs_a16(const LossLaunch& ll) {
    const codae_batch* b = ll.batch;
    const bool masked = b->mask_id || b->mask_to_use;
    return a16(b->data) && a16(ll.y) && (!masked || (reinterpret_cast<uintptr_t>(b->mask_table) & 3) == 0);
}
// g(std::bool_constant<SWAP>) for the launch's instantiation of the "replaced" test
template <typename G>
inline void swap_dispatch(const SwapWeightArgs& wa, G&& g) {
    if (wa.replace == REPLACE_SWAP) g(std::true_type{}); else g(std::false_type{});
}
// f(std::bool_constant<VEC>, std::bool_constant<DY_BF16>, std::bool_constant<PRES>) for the launch's instantiation
template <typename F>
inline void loss_dispatch(bool vec, bool dy_bf16, bool pres, F&& f) {
    auto with_pres = [&](auto V, auto O) { if (pres) f(V, O, std::true_type{}); else f(V, O, std::false_type{}); };
    if (vec && dy_bf16) with_pres(std::true_type{}, std::true_type{});
    else if (vec) with_pres(std::true_type{}, std::false_type{});
    else if (dy_bf16) with_pres(std::false_type{}, std::true_type{});
    else with_pres(std::false_type{}, std::false_type{});
}

// ---- the sweep -------------------------------------------------------------------------------------------------------------------
// One block owns LOSS_ROWS consecutive batch rows and sweeps all columns, a thread keeping its W = 4 (VEC) or 1 columns while it
// walks the rows; the bias gradient of the last Linear (column sums of dy) leaves as one partial-sum row per block (plain stores,
// added up in block order by bias_finish_kernel: deterministic).
// PRES (a presence table is set): an absent element's x and y are SELECTED to 0 as they are loaded - x may be NaN there -, so it
// adds exact zeros to every sum, and its stored dy is +0 (selection, not a weight of 0).  Between the loads and the stores the
// text is the one without a table: an all-ones table gives its bits.
// A term carries its own running sums and is called once per element:
//   g = term(live, rr, slot, x, y, blank, hit, cw, cs)     -> the element's dy; adds g to the column sum cs in its own form
//     live   the row is inside the batch (rows past it run on row B - 1's addresses and must contribute nothing)
//     rr     the row's place in the block;  slot: the column's slot (Term::PER_SLOT or PRES, else 0)
//     blank  the slot mask blanks the element;  hit: the noise replaced it;  cw: its column weight
//   term.weighted()   false: no column weight is loaded and no Philox word formed (hit = false, cw = 1)
//   term.stores()     false: the sums alone - nothing is written to dy or colsum_part
//   Term::PER_SLOT    the term reads a value per (row, slot): every column's slot is formed, with the term's E
// Whether a sum is wrapped in opaque() is the term's: it decides whether neighbouring columns' chains are packed (DESIGN.md
// section 5d), and it is part of the bits tests/test_gpu_loss_kernel_bits.py pins.
// SWAP (the input noise is CODAE_NOISE_SWAP, wa.replace == REPLACE_SWAP): "replaced" is the swap form - one Philox call per (row,
// slot) the thread's columns touch.  A template flag, so that the instantiations of every other setting stay the code they were
// (tests/test_gpu_loss_kernel_bits.py pins their bits; whether a sum is contracted into an fma is decided per instantiation).
template <bool VEC, bool DY_BF16, bool PRES, bool SWAP = false, typename Term>
__device__ __forceinline__ void loss_sweep(const BatchArgs& ba, const float* __restrict__ y, void* __restrict__ dy, int64_t dy_ld,
                                           float* __restrict__ colsum_part, const PresArgs& pa, const WeightArgsOf<SWAP>& wa, Term& term) {
    const float* __restrict__ data = ba.data;
    const uint8_t* __restrict__ table = ba.table;
    const int B = ba.B, io = ba.io;
    const bool masked = (ba.mask_id != nullptr) || (ba.mask_to_use != nullptr);
    const uint32_t step = wa.step_dev ? (uint32_t)*wa.step_dev : wa.step;
    constexpr int W = VEC ? 4 : 1;
    const int cols = io / W;
    const int r_begin = blockIdx.x * LOSS_ROWS;
    for (int cv = threadIdx.x; cv < cols; cv += LOSS_NT) {
        const int c = cv * W;
        int sl[4] = {0, 0, 0, 0};
        if constexpr (Term::PER_SLOT) {
#pragma unroll
            for (int k = 0; k < W; ++k) sl[k] = (c + k) / term.E;
        } else if constexpr (PRES) {
            slots_of<W>(c, pa.E, sl);
        }
        int ssl[4] = {0, 0, 0, 0};
        if constexpr (SWAP) {
            if (term.weighted()) slots_of<W>(c, wa.sw.E, ssl);
        }
        float cw[4] = {1.f, 1.f, 1.f, 1.f};
        if (term.weighted() && wa.col_weight != nullptr) {
            if constexpr (VEC) {
                const float4 w4 = *reinterpret_cast<const float4*>(wa.col_weight + c);
                cw[0] = w4.x; cw[1] = w4.y; cw[2] = w4.z; cw[3] = w4.w;
            } else {
                cw[0] = wa.col_weight[c];
            }
        }
        float cs[4] = {0.f, 0.f, 0.f, 0.f};
        // rows are independent: unrolled with clamped (always valid) addresses so that the loads of
        // all LOSS_ROWS rows are in flight together; rows past the batch contribute nothing
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
            if constexpr (SWAP) {
                if (term.weighted()) swap_hits<W>(hit, ssl, (uint32_t)src_row, step, wa.sw);
            } else if (term.weighted() && wa.replace) {
                if constexpr (VEC) hits4(hit, c, (uint32_t)src_row, step, wa);
                else hit[0] = hit1(c, (uint32_t)src_row, step, wa);
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
            for (int k = 0; k < W; ++k) g[k] = term(live, rr, sl[k], xv[k], yv[k], ((m >> (8 * k)) & 0xff) == 0, hit[k], cw[k], cs[k]);
            if constexpr (PRES) {      // (the stored gradient of an absent element is +0 whatever sign its zero came out with)
#pragma unroll
                for (int k = 0; k < W; ++k) g[k] = ((pb >> k) & 1u) ? g[k] : 0.f;
            }
            if (term.stores() && live) {
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
        if (term.stores() && colsum_part) {
#pragma unroll
            for (int k = 0; k < W; ++k) colsum_part[(int64_t)blockIdx.x * io + c + k] = cs[k];
        }
    }
}

// ---- the terms -------------------------------------------------------------------------------------------------------------------
// MSELoss(mean) + the per-step metric sums:  dy = 2 (y - x) inv_n,  sq = sum (x-y)^2,  sqp = sum (1-fmask)(x-y)^2
// (-2 * 0 is -0 under an absent element: the column sum does not see the sign, the stored gradient is +0)
struct MseTerm {
    static constexpr bool PER_SLOT = false;
    float inv_n;
    int want_grad;
    float sq = 0.f, sqp = 0.f;
    __device__ __forceinline__ MseTerm(float inv_n_, int want_grad_) : inv_n(inv_n_), want_grad(want_grad_) {}
    __device__ __forceinline__ static constexpr bool weighted() { return false; }
    __device__ __forceinline__ bool stores() const { return want_grad != 0; }
    __device__ __forceinline__ float operator()(bool live, int, int, float x, float y, bool blank, bool, float, float& cs) {
        const float d = live ? x - y : 0.f;
        const float se = d * d;
        sq += se;
        if (blank) sqp += se;
        const float g = -2.f * d * inv_n;
        cs += g;
        return g;
    }
};

// The emphasised MSE:  dy = 2 w (y - x) inv_n, written as (-2 d) (w inv_n): with w == 1 the product MseTerm forms, bit for bit;
// wsq = sum w (x-y)^2, the metric sums stay unweighted
struct EmphTerm {
    static constexpr bool PER_SLOT = false;
    float alpha, beta, inv_n;
    float wsq = 0.f, sq = 0.f, sqp = 0.f;
    __device__ __forceinline__ EmphTerm(const WeightArgs& wa, float inv_n_) : alpha(wa.alpha), beta(wa.beta), inv_n(inv_n_) {}
    __device__ __forceinline__ static constexpr bool weighted() { return true; }
    __device__ __forceinline__ static constexpr bool stores() { return true; }
    __device__ __forceinline__ float operator()(bool live, int, int, float x, float y, bool blank, bool hit, float cw, float& cs) {
        const float w = live ? cw * ((blank || hit) ? alpha : beta) : 0.f;
        const float d = live ? x - y : 0.f;
        const float se = d * d;
        wsq += w * se;
        sq += se;
        if (blank) sqp += se;
        const float g = -2.f * d * (w * inv_n);
        cs += g;
        return g;
    }
};

// the criterion's own arguments (codae_recon_loss, include/codae_hip.h)
struct ReconArgs {
    float param, rparam;       // beta (SMOOTH_L1) / delta (HUBER) and its reciprocal
    float mse_weight;          // SLOT_COSINE
    int S, E;                  // SLOT_COSINE: slots per row, columns per slot
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

// L1 / SmoothL1 / Huber:  dy = w rho'(d) (-1) inv_n, d = x - y;  wr = sum w rho(d); an absent element has d = 0, rho = rho' = 0
template <int KIND>
struct RhoTerm {
    static constexpr bool PER_SLOT = false;
    float alpha, beta, inv_n;
    const ReconArgs& ra;
    float wr = 0.f, sq = 0.f, sqp = 0.f;
    __device__ __forceinline__ RhoTerm(const WeightArgs& wa, const ReconArgs& ra_, float inv_n_)
        : alpha(wa.alpha), beta(wa.beta), inv_n(inv_n_), ra(ra_) {}
    __device__ __forceinline__ static constexpr bool weighted() { return true; }
    __device__ __forceinline__ static constexpr bool stores() { return true; }
    __device__ __forceinline__ float operator()(bool live, int, int, float x, float y, bool blank, bool hit, float cw, float& cs) {
        const float w = live ? cw * ((blank || hit) ? alpha : beta) : 0.f;
        const float d = live ? x - y : 0.f;
        const float se = d * d;
        float rho, drho;
        rho_of<KIND>(d, ra, rho, drho);
        wr = opaque(wr + w * rho);
        sq = opaque(sq + se);
        if (blank) sqp = opaque(sqp + se);
        const float g = -drho * opaque(w * inv_n);
        cs = opaque(cs + g);
        return g;
    }
};

// Phase 2 of the per-slot cosine:  g = -(a x - b y) + mse_weight 2 w (y - x) inv_n with the pair's coefficients (a, b) read from
// coef [LOSS_ROWS][S][2] in LDS (slot_cosine_kernel's phase 1); weights and hits only under mse_weight != 0
struct CosineTerm {
    static constexpr bool PER_SLOT = true;
    const float* coef;
    int S, E;
    float alpha, beta, mw, mwin;
    float wsq = 0.f, sq = 0.f, sqp = 0.f;
    __device__ __forceinline__ CosineTerm(const float* coef_, const WeightArgs& wa, const ReconArgs& ra, float inv_n)
        : coef(coef_), S(ra.S), E(ra.E), alpha(wa.alpha), beta(wa.beta), mw(ra.mse_weight), mwin(ra.mse_weight * inv_n) {}
    __device__ __forceinline__ bool weighted() const { return mw != 0.f; }
    __device__ __forceinline__ static constexpr bool stores() { return true; }
    __device__ __forceinline__ float operator()(bool live, int rr, int slot, float x, float y, bool blank, bool hit, float cw, float& cs) {
        const float d = live ? x - y : 0.f;
        const float se = d * d;
        sq = opaque(sq + se);
        if (blank) sqp = opaque(sqp + se);
        const float a = coef[2 * (rr * S + slot)], bq = coef[2 * (rr * S + slot) + 1];
        float gk = __fmaf_rn(bq, y, -opaque(a * x));
        if (mw != 0.f) {
            const float w = cw * ((blank || hit) ? alpha : beta);
            wsq = opaque(wsq + w * se);
            gk = __fmaf_rn(opaque(-2.f * d), opaque(w * mwin), gk);
        }
        const float g = live ? gk : 0.f;
        cs = opaque(cs + g);
        return g;
    }
};

}  // namespace codae
