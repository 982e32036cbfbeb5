// Shared declarations for libcodae_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <type_traits>

#include "codae_hip.h"

namespace codae {

void set_error(const char* fmt, ...);

#define CODAE_HIP_CHECK(expr)                                                              \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            codae::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return CODAE_E_HIP;                                                            \
        }                                                                                  \
    } while (0)

#define CODAE_LAUNCH_CHECK()                                                               \
    do {                                                                                   \
        hipError_t e_ = hipGetLastError();                                                 \
        if (e_ != hipSuccess) {                                                            \
            codae::set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), __FILE__, __LINE__); \
            return CODAE_E_HIP;                                                            \
        }                                                                                  \
    } while (0)

#define CODAE_REQUIRE(cond, ...)                                                           \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            codae::set_error(__VA_ARGS__);                                                 \
            return CODAE_E_INVALID;                                                        \
        }                                                                                  \
    } while (0)

typedef uint16_t bf16_t;  // raw bf16 storage

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

__device__ __forceinline__ float bf16_to_f32(bf16_t v) { return __uint_as_float(((uint32_t)v) << 16); }
// round-to-nearest-even through the hardware convert (keeps NaN a NaN)
__device__ __forceinline__ bf16_t f32_to_bf16(float f) {
    __bf16 b = (__bf16)f;
    return __builtin_bit_cast(bf16_t, b);
}

// two fp32 -> one packed bf16 pair with a single v_cvt_pk_bf16_f32 (round-to-nearest-even)
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    const f32x2_t v = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
}
// max(x, floor) that keeps a NaN x a NaN, as torch.relu does (include/codae_hip.h, "Non-finite values"), in ONE VALU op:
// gfx950's v_maximum3_f32 is IEEE 754-2019 maximum (NaN-propagating).  v_max_f32 and fmaxf() return the OTHER operand for a
// NaN - 0 under ReLU, -inf under the identity; a compare + select keeps it but costs a second op per element (measured: +0.4 %
// of the C3 step, about +1 % of C2).
// The GEMM epilogues clamp at `floor` = 0 (ReLU) or -inf (identity), so the ReLU switch costs no branch.
// Every ReLU site of the library goes through this one form, so that they agree bit for bit.
__device__ __forceinline__ float clamp_below(float x, float floor) {
    float r;
    asm("v_maximum3_f32 %0, %1, %2, %2" : "=v"(r) : "v"(x), "v"(floor));
    return r;
}

// bias[j .. j+3] (or zeros when there is no bias / j is past N) as ONE unconditional 16-B load from a clamped address:
// with a branch around it the compiler waits for each of an epilogue's 6 bias loads before issuing the next one
// (~0.5 us of L2 latency apiece).  `valid`: any readable 16-B aligned address.
__device__ __forceinline__ float4 load_bias4(const float* __restrict__ bias, const void* valid, int j, int N) {
    const bool ok = bias != nullptr && j < N;
    const float4 v = *reinterpret_cast<const float4*>(ok ? bias + j : reinterpret_cast<const float*>(valid));
    return make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
}

// ---- activations other than ReLU (CODAE_ACT_*; include/codae_hip.h has the parameter table) -----------------------------
// Only the generic-activation instantiations of the GEMM epilogues (template flag ACT) call these; the ReLU / identity
// instantiations keep clamp_below and the sign / bit masks.  Every supported activation is monotone, so its derivative is a
// function of the saved OUTPUT y: the data gradient multiplies by act_dy_from_y(saved activation) where ReLU masks by y > 0.
// Formulas as torch's CPU kernels write them (elu / softplus / hardsigmoid and their is_result backwards).
// The empty asm statements keep each element's arithmetic a scalar chain: left alone, the SLP vectorizer packs neighbouring
// elements - and the double-float steps inside the device library's expm1f / log1pf - into v_pk_*_f32 with op_sel routing
// (tools/check_isa.py rule 4 rejects that form).  So exp / log are the hardware v_exp_f32 / v_log_f32
// and expm1 / log1p Kahan's identities on top of them (a few fp32 ulps; the fp32 engine's bar is rtol 1e-3).
__device__ __forceinline__ float opaque(float x) { asm("" : "+v"(x)); return x; }
__device__ __forceinline__ float act_exp(float x) { return __builtin_amdgcn_exp2f(opaque(x * 1.44269504f)); }
__device__ __forceinline__ float act_log(float x) { return opaque(__builtin_amdgcn_logf(x)) * 0.693147181f; }
__device__ __forceinline__ float act_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float act_expm1(float x) {     // (u - 1) x / log u: the rounding of u cancels
    const float u = opaque(act_exp(x));
    const float um1 = opaque(u - 1.f);
    if (u == 1.f) return x;
    if (um1 == -1.f) return -1.f;
    return opaque(um1 * x) * act_rcp(act_log(u));
}
__device__ __forceinline__ float act_log1p(float t) {     // t log(1 + t) / ((1 + t) - 1)
    const float u = opaque(1.f + t);
    if (u == 1.f) return t;
    return opaque(act_log(u) * t) * act_rcp(opaque(u - 1.f));
}
__device__ __forceinline__ float act_fwd_(int kind, const float* p, float v) {
    switch (kind) {
        case CODAE_ACT_RELU: return clamp_below(v, 0.f);              // (NaN stays NaN: every kind, as torch.nn's modules)
        case CODAE_ACT_LEAKY: return v > 0.f ? v : v * p[0];
        case CODAE_ACT_RELU6: return v <= 0.f ? 0.f : (v >= 6.f ? 6.f : v);
        case CODAE_ACT_ELU: return v > 0.f ? v * p[0] : act_expm1(v * p[2]) * opaque(p[1] * p[0]);
        case CODAE_ACT_SOFTPLUS: return v * p[0] > p[1] ? v : act_log1p(act_exp(v * p[0])) * act_rcp(p[0]);
        case CODAE_ACT_HARDSIGMOID: { const float t = clamp_below(v + 3.f, 0.f); return (t > 6.f ? 6.f : t) * (1.f / 6.f); }
        default: return v;
    }
}
__device__ __forceinline__ float act_fwd(int kind, const float* p, float v) {
    asm("" : "+v"(v));
    float r = act_fwd_(kind, p, v);
    asm("" : "+v"(r));
    return r;
}
__device__ __forceinline__ float act_dy_from_y_(int kind, const float* p, float y) {
    switch (kind) {
        case CODAE_ACT_RELU: return y > 0.f ? 1.f : 0.f;
        case CODAE_ACT_LEAKY: return y > 0.f ? 1.f : p[0];
        case CODAE_ACT_RELU6: return (y > 0.f && y < 6.f) ? 1.f : 0.f;
        case CODAE_ACT_ELU: return y > 0.f ? p[0] : p[2] * opaque(y + opaque(p[1] * p[0]));
        case CODAE_ACT_SOFTPLUS: return y * p[0] > p[1] ? 1.f : -act_expm1(-y * p[0]);
        case CODAE_ACT_HARDSIGMOID: return (y > 0.f && y < 1.f) ? 1.f / 6.f : 0.f;
        default: return 1.f;
    }
}
__device__ __forceinline__ float act_dy_from_y(int kind, const float* p, float y) {
    asm("" : "+v"(y));
    float r = act_dy_from_y_(kind, p, y);
    asm("" : "+v"(r));
    return r;
}

// g * act'(y) as torch's backward forms it: ReLU, ReLU6 and Hardsigmoid SELECT (0 where the derivative is 0, whatever g is - a
// NaN or Inf gradient does not leak through a dead unit), every other kind multiplies (NaN * 0 = NaN there, in torch too)
__device__ __forceinline__ float act_bwd(int kind, const float* p, float g, float y) {
    const float d = act_dy_from_y(kind, p, y);
    const bool selects = kind == CODAE_ACT_RELU || kind == CODAE_ACT_RELU6 || kind == CODAE_ACT_HARDSIGMOID;
    return (selects && d == 0.f) ? 0.f : g * d;
}

// f(std::integral_constant<int, kind>): one switch per thread around a whole epilogue instead of one per element (a loop body
// small enough to unroll fully - the accumulators stay in registers)
template <typename F>
__device__ __forceinline__ void act_dispatch(int kind, F&& f) {
    switch (kind) {
        case CODAE_ACT_RELU: f(std::integral_constant<int, CODAE_ACT_RELU>{}); break;
        case CODAE_ACT_LEAKY: f(std::integral_constant<int, CODAE_ACT_LEAKY>{}); break;
        case CODAE_ACT_RELU6: f(std::integral_constant<int, CODAE_ACT_RELU6>{}); break;
        case CODAE_ACT_ELU: f(std::integral_constant<int, CODAE_ACT_ELU>{}); break;
        case CODAE_ACT_SOFTPLUS: f(std::integral_constant<int, CODAE_ACT_SOFTPLUS>{}); break;
        case CODAE_ACT_HARDSIGMOID: f(std::integral_constant<int, CODAE_ACT_HARDSIGMOID>{}); break;
        default: f(std::integral_constant<int, CODAE_ACT_NONE>{}); break;
    }
}

// data gradient of a bf16 pair: (g_lo, g_hi) * act'(saved pair (h_lo, h_hi)), rounded to bf16 again (the ReLU code masks instead)
__device__ __forceinline__ uint32_t act_dgrad_bf16x2(int kind, const float* p, uint32_t g2, uint32_t h2) {
    const float lo = act_bwd(kind, p, bf16_to_f32((bf16_t)(g2 & 0xffffu)), bf16_to_f32((bf16_t)(h2 & 0xffffu)));
    const float hi = act_bwd(kind, p, bf16_to_f32((bf16_t)(g2 >> 16)), bf16_to_f32((bf16_t)(h2 >> 16)));
    return pack_bf16x2(lo, hi);
}

// Philox4x32-10 (Salmon et al. 2011): the counter-based generator of the input noise (gather.hip) and of the hidden dropout
// (dropout.hip); include/codae_hip.h says which counter words each uses
__device__ __forceinline__ uint4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return make_uint4(c0, c1, c2, c3);
}

// Per-row slot presence ("Slot presence", include/codae_hip.h): tab[row * S + slot] == 0 says that DATASET row `row` has no item in
// that slot.  Kernels take it behind a template flag, so the instantiations of a step without a table stay the ones they were.
struct PresArgs {
    const uint8_t* tab;   // device [n_rows][S]; null = every slot present
    int S, E;             // slots per row, columns per slot
};
// Which of the W columns c .. c + W - 1 of dataset row `row` are present, as bit k of the result.  sl[k] = (c + k) / E, formed
// once by the caller (a loss kernel's thread keeps its columns while it walks the rows: no division in the row loop).  One byte per
// (row, slot): a group inside one slot reads one byte, a group that straddles slots (E = 6, E = 12) decides per column.
template <int W>
__device__ __forceinline__ uint32_t present_bits(const PresArgs& p, int64_t row, const int* sl) {
    const uint8_t* __restrict__ t = p.tab + row * p.S;
    const uint32_t p0 = t[sl[0]] != 0 ? 1u : 0u;
    if (sl[W - 1] == sl[0]) return p0 ? ((1u << W) - 1u) : 0u;
    uint32_t bits = p0;
#pragma unroll
    for (int k = 1; k < W; ++k) bits |= (t[sl[k]] != 0 ? 1u : 0u) << k;
    return bits;
}
int check_presence(const uint8_t* present, int n_slots, int io, const char* who);

// Swap noise ("Swap noise", include/codae_hip.h): whether slot `slot` of DATASET row `row` takes another row's item at `step`, and
// which row's.  One Philox call per (row, slot), counter (slot, row, step, 512); pres (null: none) is the presence table [.][S].
struct SwapArgs {
    const int32_t* pool;   // device [P], or null = the row itself
    uint32_t P;
    int S, E;              // slots per row, columns per slot
    uint64_t thresh;       // T = floor(p 2^32)
    uint32_t key0, key1;
    const uint8_t* pres;
};
constexpr uint32_t SWAP_STREAM = 512u;
// the source row q of an accepted swap, or -1: not hit, q == row, or a side absent
__device__ __forceinline__ int64_t swap_source(const SwapArgs& a, uint32_t row, int slot, uint32_t step) {
    const uint4 r = philox4x32_10((uint32_t)slot, row, step, SWAP_STREAM, a.key0, a.key1);
    if (!((uint64_t)r.x < a.thresh)) return -1;
    const uint32_t j = (uint32_t)(((uint64_t)r.y * a.P) >> 32);
    const uint32_t q = a.pool ? (uint32_t)a.pool[j] : j;
    if (q == row) return -1;
    if (a.pres != nullptr && (a.pres[(int64_t)row * a.S + slot] == 0 || a.pres[(int64_t)q * a.S + slot] == 0)) return -1;
    return (int64_t)q;
}
// host side: the kernel argument of a validated (noise, swap) pair; check_swap: CODAE_E_INVALID with the offending argument named
int check_swap(const codae_swap* swap, int io, const uint8_t* present, int pres_slots, const char* who);
inline SwapArgs swap_args(const codae_noise* n, const codae_swap* sw, int io, const uint8_t* present) {
    SwapArgs a{};
    a.pool = sw->pool; a.P = (uint32_t)sw->n_pool; a.S = sw->n_slots; a.E = io / sw->n_slots;
    a.thresh = (uint64_t)floor((double)n->p0 * 4294967296.0);
    a.key0 = (uint32_t)(n->seed & 0xffffffffu); a.key1 = (uint32_t)(n->seed >> 32);
    a.pres = present;
    return a;
}

static inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// the launch shape of the single-pass kernels: GRID_NT threads per block, a grid-stride loop over at most 2048 blocks
constexpr int GRID_NT = 256;
inline int grid_for(int64_t work_items) {
    int64_t b = (work_items + GRID_NT - 1) / GRID_NT;
    if (b < 1) b = 1;
    if (b > 2048) b = 2048;
    return (int)b;
}

// ---- output store policy (GemmBf16::store_policy) ------------------------------------------------------
// PLAIN: ordinary stores - the lines stay dirty in the writing XCD's L2 and are written back at the kernel's end, when no workgroup
// computes any more.  WT: write-through stores (sc1) - every line leaves for memory as its store is issued, under the rest of the
// epilogue and the K-loop tails of slower workgroups.  Same bytes, same addresses: a cache policy changes no value.
// (sc0 sc1 measured the same as sc1 - 1.2043 against 1.2063 ms per C3 step over three alternating runs - and is not built.)
enum { STORE_PLAIN = 0, STORE_WT = 1 };
// policy of a launch that writes out_bytes: CODAE_STORE_POLICY when set, else by the output's size against the L2s (gemm_bf16.hip)
int store_policy_for(int64_t out_bytes);

// 16-byte-per-lane stores into one output tile under a policy fixed at COMPILE time (the cache-policy bits are instruction
// immediates; a run-time choice per store - a scalar branch in front of each - ended the write-out loops' basic blocks at every
// store and cost the plain path 1 us per C3 launch).  PLAIN: the ordinary pointer store this code always had.  WT: a raw buffer
// descriptor over the tile's first row (wave-uniform base) + a 32-bit byte offset per lane (the launchers keep a tile's span under
// 2 GiB or fall back to PLAIN).
template <int POL>
struct TileStore {
    __amdgpu_buffer_rsrc_t rsrc;
    __device__ __forceinline__ explicit TileStore(void* tile_base) {
        if constexpr (POL != STORE_PLAIN) rsrc = __builtin_amdgcn_make_buffer_rsrc(tile_base, 0, 0x7fffffff, 0x00020000);
    }
    // p: the element's address; byte_off: the same place relative to tile_base
    __device__ __forceinline__ void store16(void* p, uint32_t byte_off, u32x4 v) const {
        if constexpr (POL == STORE_PLAIN) *reinterpret_cast<u32x4*>(p) = v;
        else __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, (int)byte_off, 0, 16);      // aux 16: sc1
    }
};

// CODAE_* tuning variables, read ONCE (library load, codae_create, codae_reload_env): nothing on the
// launch path calls getenv (round 1 did, ~30 times per step)
struct EnvToggles {
    int gemm_tile = -1;          // CODAE_GEMM_TILE: s = 128 x 128 (0), q = 256 x 192 pipelined, every wave loads (3),
                                 // x = 256 x 192 pipelined, LDS-DMA on one wave per SIMD (6); -1 = automatic
    int wgrad_splitk = 0;        // CODAE_WGRAD_SPLITK > 0 forces the split
    int small_tile_max = 200;    // CODAE_SMALL_TILE_MAX: forward-form launches of up to this many 128 x 128 tiles run on 64 x 64 tiles
    int small_stages = 4;        // CODAE_SMALL_STAGES=2: launches that cannot fill the chip keep the 2-stage double buffer
    int f32_gemm = 0;            // CODAE_F32_GEMM: native = v_mfma_f32_32x32x2_f32 always (1); default (0) and x3 (2) = three bf16 planes / six bf16
                                 // MFMA products wherever the shape is legal (gemm_f32.hip)
    int group_tile = -1;         // CODAE_GROUP_TILE: grouped weight gradients on 128 x 128 (0), 64 x 128 (1), 64 x 64 (2); -1 = automatic
    bool side_priority_set = false; int side_priority = 0;   // CODAE_SIDE_PRIORITY
    bool no_wt = false, single_stream = false, tail_on_side = false, no_fused_loss = false, flat_adam = false,
         no_fused_norm = false, no_chain = false, no_deep_small = false,      // CODAE_NO_DEEP_SMALL: 2-stage small GEMMs
         no_relu_bits = false,        // CODAE_NO_RELU_BITS: the data gradient reads the saved activation for its ReLU mask
         no_prefetch = false,         // CODAE_NO_PREFETCH: no touch of the next launch's weights under the epilogue
         no_defer_wgrad = false;      // CODAE_NO_DEFER_WGRAD: per-layer split-K weight gradients beside the data-gradient chain (round 2's backward)
    bool no_folded_loss_finish = false;      // CODAE_NO_FOLDED_LOSS_FINISH: the fused step's loss finish as a launch of its own
    bool no_folded_bias_finish = false;      // CODAE_NO_FOLDED_BIAS_FINISH: the bias finish behind the pipelined grouped weight gradients as a launch of its own
    bool no_dataset_image = false;           // CODAE_NO_DATASET_IMAGE: the gather reads the fp32 rows although a bf16 image is registered
    int store_policy = -1;       // CODAE_STORE_POLICY: plain (0), wt = sc1 write-through (1); -1 = by output size
};
const EnvToggles& env();
void env_reload();

// ---- generic exact-fp32 GEMM (gemm_f32.hip) --------------------------------
// C[i][j] = epilogue( sum_k A(i,k) * B(j,k) ), A(i,k) = A[i*a_rs + k*a_ks], B(j,k) = B[j*b_rs + k*b_ks]
struct GemmF32 {
    const float* A; int64_t a_rs, a_ks;
    const float* B; int64_t b_rs, b_ks;
    float* C; int64_t ldc;
    int M, N, K;
    const float* bias;       // [N] added before activation, or null
    int relu;                // max(v, 0)
    const float* relu_src;   // [M][ld_relu] multiply by (src > 0), or null
    int64_t ld_relu;
    float* colsum_part;      // [ceil(M / 64)][N] column sums of the stored values per 64-row block (plain stores, summed in
                             // a fixed order by launch_bias_finish: deterministic bias gradients), or null
    const int* m_dev;        // not null: the row count is min(M, *m_dev), read on the device (row tiles past it exit at once);
                             // the grid is still sized for M
    int split_k;             // > 1: K is cut into split_k ranges of whole 32-deep tiles (grid.z); range z writes its partial
                             // product to C + z * M * ldc (fp32 slabs, reduced in slab order by reduce_slabs_kernel); no
                             // bias / ReLU / column sums then
    int act;                 // != CODAE_ACT_NONE: the generic-activation instantiation (gemm_f32_kernel / gemm_f32x3_kernel <.., ACT>):
                             // stored value = act_fwd(act, act_p, v) when relu_src is null, else v * act_dy_from_y(act, act_p, relu_src);
                             // `relu` is ignored then.  CODAE_ACT_NONE: the ReLU / identity code above
    float act_p[3];
};
int gemm_f32(const GemmF32& g, hipStream_t s);
int gemm_f32x3(const GemmF32& g, hipStream_t s);      // gemm_f32x3.hip: the same product from three bf16 planes per operand
bool gemm_f32x3_takes(const GemmF32& g);              // its shape / alignment conditions (everything else stays on gemm_f32_kernel)
inline int gemm_f32_colsum_rows(int M) { return (M + 63) / 64; }

// several independent exact-fp32 GEMMs in one launch of the bf16-plane kernel (gemm_f32x3.hip): the fp32 engine's weight gradients
constexpr int CODAE_GROUP_MAX = 16;
struct GemmF32Group {
    int n;
    GemmF32 g[CODAE_GROUP_MAX];
    int wg_begin[CODAE_GROUP_MAX + 1];     // prefix sum of workgroups per GEMM (filled by the launcher)
};
int gemm_f32x3_grouped(GemmF32Group& grp, hipStream_t s);

// ---- bf16 MFMA GEMM (gemm_bf16.hip) ----------------------------------------
enum { OP_KC = 0,  // operand stored [rows][k] (k contiguous)
       OP_KS = 1   // operand stored [k][rows] (rows contiguous; transposed LDS reads)
};
// MSE loss folded into the epilogue of the last forward GEMM (train_dae_on_embedding.py:206-223):
// the kernel then writes dL/dy (bf16) instead of y and accumulates the metric sums.
struct LossFuse {
    int enabled;
    const float* data;            // dataset [n][io] fp32
    const int32_t* row_idx;       // [rows] or null
    const int32_t* mask_id;       // [rows] or null
    const int32_t* mask_to_use;   // [n][nb_run] or null
    int nb_run, run;
    const uint8_t* table;         // [n_masks][io]
    int io;
    int B;                        // valid batch rows; rows in [B, M) get dy = 0
    float inv_n;                  // 1 / (global rows * io)
    double* parts;                // [workgroups][2]: each workgroup's {sum (x-y)^2, sum (1-m)(x-y)^2}, plain stores; added up
                                  // in index order by launch_finish_loss (256 same-address double atomics cost the
                                  // kernel ~10 us of serialised tail, and their order is not reproducible)
};

struct GemmBf16 {
    const bf16_t* A; int64_t lda; int a_mode;   // output row index i
    const bf16_t* B; int64_t ldb; int b_mode;   // output col index j
    void* C; int64_t ldc; int c_f32;            // bf16 or fp32 output [M][N]
    int M, N, K;
    const float* bias;
    int relu;
    const bf16_t* relu_src; int64_t ld_relu;
    float* colsum_part;      // [tiles_m][N] per-tile column sums of the stored values (plain stores; see GemmF32), or null
    int split_k;             // >1: fp32 partial slabs C + z*M*ldc, K range split evenly in BK units
    LossFuse loss;           // enabled: C receives dy (bf16), colsum_part the last bias gradient's partial sums
    int : 32;                // pad: keeps the kernel-argument offsets behind it, and with them eight EPI 5 kernels' code, as they were
    // ReLU mask as one bit per element, [rows][ld_bits] bytes, bit k of byte (i, j / 8) = (stored value (i, j + k) > 0): written by a
    // forward launch (relu_bits_out), read by the data-gradient launch INSTEAD of the saved activation (relu_bits; relu_src stays
    // set for the kernels that do not take bits).  Pipelined kernels only: gemm_bf16_takes_relu_bits() says whether a launch
    // of this shape will write / read them.
    uint8_t* relu_bits_out; const uint8_t* relu_bits; int64_t ld_bits;
    const void* prefetch; int64_t prefetch_bytes;   // pipelined 256 x 192 kernel only: touched (one 4-B load per 128-B line, spread
                             // over the launch's workgroups) while the epilogue runs - the NEXT launch's weight matrix, which
                             // would otherwise come from HBM under its first K-tiles; null = nothing
    int coscheduled;         // this launch shares the chip with another stream's kernels (the data-gradient chain beside the per-layer
                             // weight gradients of the data-parallel / bucketed backward): the pipelined kernel keeps the COMPILER's
                             // instruction schedule - its pinned, hand-ordered phases (gemm_bf16_halftile.h) win 1.3 % when the launch
                             // has the chip to itself and lose 7.5 % of the step in that company (tools/abl/ab_dp.sh)
    double* sumsq_slots;     // fp32 output, 128 x 128 tile only: += sum of the stored values' squares, scattered over the
                             // CODAE_S_N_SLOTS clip_grad_norm_ slots (what sumsq_kernel would add in a pass of its own), or null
    int act;                 // as GemmF32::act: != CODAE_ACT_NONE picks the generic-activation instantiation (forward form: act_fwd on
                             // the stored values; data-gradient form: times act_dy_from_y of relu_src); no 1-bit masks, no fused loss,
                             // no k-strided A operand there
    float act_p[3];
    int store_policy;        // STORE_*: how the pipelined kernels' epilogues store the output tile (bf16 rows, fused-loss dy, fp32 half
                             // tiles; the mask dwords and column-sum rows stay plain).  Other kernels ignore it.
};
bool gemm_bf16_supported(int M, int N, int K);

// The workgroup tiles of the GEMM kernels, and how many of one cover an M x N output: the one form of this arithmetic in the host
// code (the plan below, the split-K choices, the engine's grouped weight-gradient modes, the grouped launchers)
struct GemmTile { int bm, bn; };
constexpr GemmTile TILE_256x192{256, 192}, TILE_128x192{128, 192}, TILE_128x128{128, 128}, TILE_64x128{64, 128}, TILE_64x64{64, 64};
inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline int tile_count(int M, int N, GemmTile t) { return ceil_div(M, t.bm) * ceil_div(N, t.bn); }

// What gemm_bf16(g) launches, decided ONCE by gemm_bf16_plan (gemm_bf16.hip): the launchers switch on these fields and
// nothing else, and whoever must know a launch's tile in advance (the engine's partial-sum row counts, the 1-bit ReLU masks)
// reads them from the same plan.
enum { BF16_ONE_BARRIER = 0,      // gemm_bf16_kernel: one-barrier double buffer, or four stages (gemm_bf16.hip)
       BF16_PIPELINED = 1         // gemm_bf16_pipe_kernel: phase-pipelined (gemm_bf16_pipe.hip)
};
// instruction schedule of the pipelined kernel's K loop (its SCHED template argument; the values are part of the kernels' symbol names)
enum { SCHED_PINNED = 0,          // the phases pinned and ordered by hand (gemm_bf16_halftile.h)
       SCHED_COMPILER = 64        // the compiler's own schedule (GemmBf16::coscheduled)
};
struct Bf16Plan {
    int family;              // BF16_*
    int bm, bn;              // workgroup tile: 64 x 64, 128 x 128 (one-barrier); 128 x 192, 256 x 192 (pipelined)
    int stages;              // one-barrier: operand stages in LDS, 2 or 4; pipelined: 0
    int loader;              // pipelined: 1 = 256 x 192, every wave loads (B halves by 6 of the 8); 6 = 256 x 192, LDS-DMA on one wave per
                             // SIMD; 7 = 128 x 192 (forward form only); one-barrier: 0
    int epi;                 // 3 = fused loss (either family); pipelined bf16 output: 1 = forward, 2 = data-gradient epilogue; else 0
    int sched;               // pipelined: SCHED_PINNED, or SCHED_COMPILER for a GemmBf16::coscheduled launch; one-barrier: 0
    int act;                 // the generic-activation instantiation (one-barrier only)
    int store_policy;        // STORE_* the launch really stores with: the descriptor's, after the ldc fallback; PLAIN wherever the
                             // kernel takes no policy
    int tiles_m, tiles_n;
    int64_t workgroups;      // tiles_m * tiles_n * split_k = the grid
};
Bf16Plan gemm_bf16_plan(const GemmBf16& g);
bool gemm_bf16_takes_relu_bits(int M, int N);    // forward-form bf16 launch of this output shape runs on a pipelined kernel
int gemm_bf16_colsum_rows(const GemmBf16& g);   // rows of colsum_part this launch writes (= its plan's tiles along M)
int gemm_bf16_loss_parts(const GemmBf16& g);    // workgroups of the fused-loss launch = rows of LossFuse::parts
int gemm_bf16(const GemmBf16& g, hipStream_t s);
int gemm_bf16_pipe(const GemmBf16& g, const Bf16Plan& plan, hipStream_t s);   // gemm_bf16_pipe.hip: the pipelined family of a plan
int choose_split_k(int N, int K, int rows);     // gemm_bf16.hip: split-K factor of the weight gradient dW[N][K] over `rows` batch rows

// several independent GEMMs (here: the weight gradients of every layer of a narrow stack) in ONE launch; tile
// configuration 128 x 128 for all of them
struct GemmBf16Group {
    int n;
    GemmBf16 g[CODAE_GROUP_MAX];
    int wg_begin[CODAE_GROUP_MAX + 1];     // prefix sum of workgroups per GEMM (filled by the launcher)
};
int gemm_bf16_grouped(GemmBf16Group& grp, hipStream_t s);
// 256 x 192 pipelined tiles, unsplit K (gemm_bf16_pipe.hip); fold != null: the step's bias finish rides in the same launch (BiasFold, below)
struct BiasFold;
int gemm_bf16_pipe_grouped(GemmBf16Group& grp, hipStream_t s, const BiasFold* fold = nullptr);

// ---- persistent fused chain for narrow stacks (chain_bf16.hip) ----------------
constexpr int CODAE_CHAIN_MAX_WIDTH = 512;
constexpr int CODAE_CHAIN_MAX_LAYERS = 16;
constexpr int CODAE_CHAIN_MAX_BIAS = 6144;          // floats: all layers' biases are staged in LDS
struct ChainArgs {
    int L, rows, B;                                  // rows: batch padded to a multiple of 64
    int width[CODAE_CHAIN_MAX_LAYERS + 1];           // width[l] = input of layer l, width[L] = output of the last
    uint32_t relu_flags;                             // bit l: layer l ends in a ReLU
    double* scalars;                                 // not null: workgroup 0 zeroes CODAE_S_GRAD_SQ and the norm slots
    const bf16_t* W[CODAE_CHAIN_MAX_LAYERS];         // bf16 weight shadow   [out][in]
    const bf16_t* Wt[CODAE_CHAIN_MAX_LAYERS];        // transposed shadow    [in][out]
    const float* bias[CODAE_CHAIN_MAX_LAYERS];
    bf16_t* act[CODAE_CHAIN_MAX_LAYERS];             // act[l] [rows][width[l]]: input of layer l (saved for the backward)
    bf16_t* dact[CODAE_CHAIN_MAX_LAYERS];            // dact[l] [rows][width[l+1]]: gradient of layer l's output
    float* colsum_part[CODAE_CHAIN_MAX_LAYERS];      // [rows / 16][width[l+1]] partial bias gradients
    const float* data; const int32_t* row_idx; const int32_t* mask_id; const uint8_t* mask_table;
    const int32_t* mask_to_use; int nb_run, run;
    float inv_n;                                     // 1 / (global rows * io)
    double* loss_parts;                              // [rows / 16][2]
    int do_backward;
};
bool chain_supported(int L, const int* in, const int* out);
int chain_rows_per_workgroup();
int launch_chain_step(const ChainArgs& a, hipStream_t s);

// ---- the batch gather (gather.hip) -----------------------------------------
// out[b] = the batch's row b: gathered, then the input noise of `noise` (codae_noise, include/codae_hip.h; null or
// CODAE_NOISE_NONE = the plain gather), then the slot mask, then the presence rule.  One launcher for every instantiation.
// out_ld: row stride of `out` in elements (0 = b->io: contiguous rows)
// step: the noise counter's step word; step_dev != null: read it from that device scalar instead (graph replay: kernel arguments
// are frozen at capture); noise_rows: see codae_corrupt_batch.  check_noise: CODAE_E_INVALID with the offending argument named.
// zero_norm != null: the scalars block - the launch also clears CODAE_S_GRAD_SQ and its slots (the fused step that folds its loss
// finish into the bias finish: nothing else runs between the previous update and the first weight gradient)
// present != null (every launcher below that takes it): the presence table [n_rows][n_slots] of "Slot presence" - the PRES
// instantiations; null launches exactly what it launched before.
int check_noise(const codae_noise* noise);
int launch_gather_noise(const codae_batch* b, const codae_noise* noise, int32_t step, const double* step_dev, void* out,
                        int out_bf16, hipStream_t s, int64_t out_ld = 0, const int32_t* noise_rows = nullptr, double* zero_norm = nullptr,
                        const uint8_t* present = nullptr, int n_slots = 0, const codae_swap* swap = nullptr, const float* swap_data = nullptr);
// (swap: required by CODAE_NOISE_SWAP; swap_data: the matrix the swapped slots are read from, null = b->data)
// The plain gather (bf16 out, no noise) from the dataset's bf16 image instead of its fp32 rows (codae_set_dataset_image): the same
// bits as launch_gather_noise(b, nullptr, .., out, 1, ...) on the data the image was cast from.  gather_image_takes: the shape / alignment
// conditions of its 16-byte accesses (io and out_ld multiples of 8, image and out 16-byte, the mask table 8-byte aligned).
bool gather_image_takes(const codae_batch* b, const void* image, const void* out, int64_t out_ld);
// noise (null, NONE or SWAP) with step / step_dev / swap as launch_gather_noise: the swapped slots come from the image too.
int launch_gather_image(const codae_batch* b, const bf16_t* image, bf16_t* out, hipStream_t s, int64_t out_ld = 0, double* zero_norm = nullptr,
                        const uint8_t* present = nullptr, int n_slots = 0, const codae_noise* noise = nullptr, int32_t step = 0,
                        const double* step_dev = nullptr, const codae_swap* swap = nullptr);
int launch_noise_box_muller(const uint32_t* ra, const uint32_t* rb, float* rho, float* c, float* sn, int64_t n, hipStream_t s);
int launch_cast_bf16(const float* src, bf16_t* dst, int64_t n, hipStream_t s);
int launch_corrupt(const float* x, const float* mask, float* out, int64_t n, hipStream_t s);
int launch_expand_masks(const int32_t* mask_id, const uint8_t* table, const int32_t* k_of_mask, int B, int io,
                        int k_max, float* masks_out, float* fmask_out, hipStream_t s);
// ---- assembled outfits and compatibility (compat.hip; include/codae_hip.h, "Assembled outfits and compatibility") ----
// assemble: out rows [Q] (blank [Q] or null) or [Q S] (leave_one_out) from src = the fp32 rows or, src_bf16, their bf16 image (bf16 out
// only); out_ld 0 = io.  outfit_scores: Y [Q S][y_ld] fp32, the leave-one-out reconstruction.  auc_counts: parts_ws auc_blocks(M) * S * 3
// 64-bit words, counts int64 [S + 1][4].  Every argument error is CODAE_E_INVALID with the offending value named.
int launch_assemble_outfits(const void* src, int src_bf16, int64_t n_rows, int io, int n_slots, const int32_t* items, int Q,
                            const int32_t* blank, int leave_one_out, const uint8_t* present, void* out, int out_bf16, int64_t out_ld,
                            hipStream_t s);
int launch_outfit_scores(const float* data, int64_t n_rows, int io, int n_slots, const int32_t* items, int Q, const uint8_t* present,
                         const float* Y, int64_t y_ld, float* cos_out, float* sq_out, float* score, int32_t* n_present, hipStream_t s);
int auc_blocks(int M);
int launch_auc_counts(const float* pos, const uint8_t* pos_on, int P, const float* neg, const int32_t* neg_slot, const int32_t* neg_parent,
                      int M, int n_slots, void* parts_ws, int64_t* counts, hipStream_t s);
// ---- stand-alone losses and reductions (elementwise.hip and the files named below); the update (optimizer.hip) ----
// One stand-alone loss launch: y fp32 [B][io], x gathered from `batch`; writes dy (fp32 or bf16, row stride dy_ld; 0 = io), one
// colsum_part row per block (partial sums of the last bias gradient; may be null) and the per-block sums `parts`.
// noise / step / step_dev as launch_gather_noise (which elements the gather replaced is recomputed from the same words); emph may
// be null (all weights 1); present != null: the presence table [n_rows][n_slots] - the PRES instantiations.
struct LossLaunch {
    const codae_batch* batch; const codae_noise* noise; int32_t step; const double* step_dev;
    const codae_emphasis* emph; const uint8_t* present; int n_slots;
    const float* y; void* dy; int dy_bf16; int64_t dy_ld; float scale /* inv_n, or the contrast's scale */;
    float* colsum_part; double* parts;
    const codae_swap* swap;      // with noise->kind == CODAE_NOISE_SWAP: its slots and pool
};
inline int64_t loss_dy_ld(const LossLaunch& ll) { return ll.dy_ld > 0 ? ll.dy_ld : (ll.batch ? ll.batch->io : 0); }
// the argument checks every loss launcher makes, the error texts prefixed with `who`; needs_dy: dy must be there
int check_loss_launch(const char* who, const LossLaunch& ll, bool needs_dy);
// parts [mse_loss_colsum_rows(B)][2]: per-block metric sums (see LossFuse::parts); want_grad 0: the sums alone (dy may be null)
int launch_mse_loss(const LossLaunch& ll, int want_grad, hipStream_t s);
int mse_loss_colsum_rows(int B);
// The emphasised denoising loss (codae_emphasis, include/codae_hip.h): launch_mse_loss's block shape - mse_loss_colsum_rows(B)
// blocks, one colsum_part row each - with a weight per element; `noise` / step / step_dev as launch_gather_noise (which elements
// the gather replaced is recomputed from the same words).  parts [mse_loss_colsum_rows(B)][3]: weighted sum, sum (x-y)^2,
// sum (1-fmask)(x-y)^2; launch_finish_emph_loss adds them up in block order: LAST_LOSS = weighted sum * inv_n, the epoch
// accumulators take the unweighted two.  check_emphasis: CODAE_E_INVALID for a negative or non-finite alpha / beta.
int check_emphasis(const codae_emphasis* emph);
int launch_emph_loss(const LossLaunch& ll, hipStream_t s);
int launch_finish_emph_loss(double* scalars, double inv_n, hipStream_t s, const double* parts, int n_parts);
// A training criterion other than the MSE (codae_recon_loss, include/codae_hip.h; recon_loss.hip): launch_emph_loss's block shape,
// arguments and outputs, `emph` may be null (all weights 1); parts[.][0] is the criterion's sum, so launch_finish_emph_loss
// finishes it.  check_recon_loss: CODAE_E_INVALID / CODAE_E_UNSUPPORTED as codae_set_recon_loss documents (io <= 0: not checked
// against n_slots).
int check_recon_loss(const codae_recon_loss* loss, int io);
int launch_recon_loss(const LossLaunch& ll, const codae_recon_loss* loss, hipStream_t s);
// The mixed-variable criterion (codae_variable_loss, include/codae_hip.h; variable_loss.hip): three launches on the seam of the
// other stand-alone losses.  ws: the setting's work space (the table's device image at its head, written by variable_loss_upload);
// partials leaves the per-block sums there, finish forms the coefficients and writes the scalars (LAST_LOSS, the epoch sums, the
// norm accumulators zeroed), grad writes ll.dy and one ll.colsum_part row per mse_loss_colsum_rows block.  check_variable_loss:
// CODAE_E_INVALID as codae_set_variable_loss documents (io <= 0: not checked against io; max_B < 1: ws_bytes not checked).
int check_variable_loss(const codae_variable_loss* v, int io, int max_B);
int64_t variable_loss_ws_bytes(int n_var, int B);
int variable_loss_upload(const codae_variable_loss* v);
int launch_variable_partials(const LossLaunch& ll, const void* ws, int n_var, hipStream_t s);
int launch_variable_finish(const LossLaunch& ll, const void* ws, int n_var, double* scalars, hipStream_t s);
int launch_variable_grad(const LossLaunch& ll, const void* ws, int n_var, hipStream_t s);
// Sampled-softmax slot contrast (codae_slot_contrast, include/codae_hip.h; slot_contrast.hip): an additional term on top of the
// criterion.  prepare fills the work space with the step's S x K normalised candidates; launch_slot_contrast adds the term's
// gradient to the dy the criterion's kernel left (operand type of the products = dy's type), leaves slot_contrast_blocks(B) rows of
// colsum_part (column sums of the final dy) and as many doubles of parts (sum W l); the finish adds scale * sum parts to LAST_LOSS.
// check_slot_contrast: CODAE_E_INVALID / CODAE_E_UNSUPPORTED as codae_set_slot_contrast documents (io <= 0: the struct's own ranges only).
int check_slot_contrast(const codae_slot_contrast* c, int io, int bf16);
int64_t slot_contrast_ws_bytes(int S, int K, int E, int bf16);
inline int slot_contrast_blocks(int B) { return (B + 31) / 32; }
int slot_contrast_warm();     // one-time kernel attributes, outside any stream capture
int launch_slot_contrast_prepare(const float* data, int io, const codae_slot_contrast* c, int32_t step, const double* step_dev, int bf16,
                                 hipStream_t s, const uint8_t* present = nullptr, int n_slots = 0);
int launch_slot_contrast(const LossLaunch& ll, const codae_slot_contrast* c, hipStream_t s);
int launch_slot_contrast_finish(double* scalars, double scale, const double* parts, int n_parts, hipStream_t s);
// The streaming kernels between a step's GEMMs (dropout.hip, residual.hip, norm.hip).  Their backward forms share one sweep
// (row_sweep.h): row_sweep_blocks(B) blocks of 64 batch rows, each leaving one row of colsum_part [blocks][width] (column sums of
// the STORED values; may be null).
inline int row_sweep_blocks(int B) { return (B + 63) / 64; }
// Hidden dropout (codae_dropout, include/codae_hip.h; dropout.hip): a <- a * f in place on rows < B, columns < width of a [B][ld]
// matrix (fp32 or bf16), f from the Philox words of counter (column / 4, dataset row, step, 1 + layer); step_dev as
// launch_gather_noise.  check_dropout_p: CODAE_E_INVALID for p outside [0, 1) or not finite.
int check_dropout_p(float p, const char* who);
int launch_dropout_fwd(void* a, int bf16, int64_t ld, int B, int width, const int32_t* row_idx, int layer, int32_t step,
                       const double* step_dev, float p, uint64_t seed, hipStream_t s);
int launch_dropout_bwd(void* d, int bf16, int64_t ld, int B, int width, const int32_t* row_idx, int layer, int32_t step,
                       const double* step_dev, float p, uint64_t seed, float* colsum_part, hipStream_t s);
// What the residual and the norm backward kernels share, behind the UNMASKED data-gradient GEMM that left U in d: the gradient
// carried past skips - Gh = U + g_in (one fp32 add; g_in may be null), g_out <- the kernel's G (may be null, may be g_in), rows ld_g
// apart - and the derivative from a 1-bit mask: d <- D = G * act' rounded to the working type, act_kind RELU selects, LEAKY
// multiplies by slope; bits null = the kernel's other source of act', or 1.
struct StreamBwd {
    const float* g_in;
    float* g_out;
    int64_t ld_g;
    const uint8_t* bits;
    int64_t ld_bits;
    int act_kind;
    float slope;
};
// Residual connections (codae_residual, include/codae_hip.h; residual.hip): the two streaming kernels of a skipped layer.
// forward: y <- rne(y + x) in place on rows < B, columns < width (fp32 or bf16); bits != null: first the 1-bit mask "stored y > 0" of
// the value BEFORE the add, 8 columns per byte, column 8 j + k in bit k of byte j (the layout of the forward GEMM's masks).
// backward: G = Gh; act' from `bits`, from the saved activation `src` (any CODAE_ACT_* kind, parameters act_p) or 1 (both null).
struct ResidualBwd : StreamBwd {
    const void* src;
    int64_t ld_src;
    float act_p[3];
};
int launch_residual_fwd(void* y, const void* x, int bf16, int64_t ldy, int64_t ldx, int B, int width, uint8_t* bits, int64_t ld_bits,
                        hipStream_t s);
int launch_residual_bwd(void* d, int bf16, int64_t ld, int B, int width, const ResidualBwd& r, float* colsum_part, hipStream_t s);
// Normalisation (codae_norm, include/codae_hip.h; norm.hip): the two streaming kernels of a normalised layer, a wave per row.
// forward: bits != null: first the 1-bit mask "stored y > 0" (layout of the residual masks); then y <- xhat in place on rows < B,
// columns < width, rstd[b] <- r.  backward: G = Gs = r (Gh - c1 - xhat c2) (LAYER) / r (Gh - xhat c2) (RMS); act' from `bits` or 1.
struct NormBwd : StreamBwd {
    const void* xhat;
    int64_t ld_x;
    const float* rstd;
};
int launch_norm_fwd(void* y, int bf16, int64_t ld, int B, int width, int kind, float eps, float* rstd, uint8_t* bits, int64_t ld_bits,
                    hipStream_t s);
int launch_norm_bwd(void* d, int bf16, int64_t ld, int B, int width, int kind, const NormBwd& n, float* colsum_part, hipStream_t s);
// Sparse code (codae_sparse_code, include/codae_hip.h; sparse_code.hip): the two streaming kernels of the layer that produces the
// code.  forward: per row < B the `keep` columns < width that rank first by (key descending, column ascending) keep their bits, the
// others are stored as +0; bits != null: the 1-bit keep mask (layout of the residual masks).  backward: d <- kept ? d : +0 and the
// column sums of the stored values, the sweep of row_sweep.h.
int launch_sparse_code_fwd(void* y, int bf16, int64_t ld, int B, int width, int keep, uint8_t* bits, int64_t ld_bits, hipStream_t s);
int launch_sparse_code_bwd(void* d, int bf16, int64_t ld, int B, int width, const uint8_t* bits, int64_t ld_bits, float* colsum_part,
                           hipStream_t s);
// Outfit codes (codae_export_rows, include/codae_hip.h; codes.hip): dst [B][ld_dst] fp32 <- the stored rows of src (fp32 or bf16)
// widened exactly, columns < width; norm [B] (may be null) <- the fp32 row norms, a wave per row, no atomics.
int launch_export_rows(const void* src, int bf16, int64_t ld_src, int B, int width, float* dst, int64_t ld_dst, float* norm, hipStream_t s);
int launch_mse_dense(const float* x, const float* y, const float* fmask, float* dy, int64_t n, float inv_n,
                     double* scalars, hipStream_t s);
// optimizer.hip: the gradient norm, the clip coefficient, the update
int launch_sumsq(const float* g, int64_t n, double* out, hipStream_t s);
int launch_sumsq_to(const float* g, int64_t n, double* acc, hipStream_t s);      // *acc += sum g^2 (one address, <= 64 blocks)
int launch_clip_coef(const double* total_sq, float max_norm, double* coef_out, hipStream_t s);
// clip_grad_norm_'s sum g^2 of a flat gradient vector into scalars[CODAE_S_GRAD_SQ] (+ its slots); clear: zero them first (a caller
// whose step's loss finish has not already done so)
int launch_grad_sumsq(const float* g, int64_t n, double* scalars, bool clear, hipStream_t s);
// The vectors one update launch walks, element for element: parameters, gradients, the moments, AMSGrad's running maximum, the
// weight average, the bf16 shadow (each of the last three null when its feature is off).  at(lo): the same vectors from element lo on.
struct ParamVectors {
    float *p, *g, *m, *v, *vmax, *avg;
    bf16_t* shadow;
    ParamVectors at(int64_t lo) const {
        return {p ? p + lo : p, g ? g + lo : g, m ? m + lo : m, v ? v + lo : v, vmax ? vmax + lo : vmax, avg ? avg + lo : avg,
                shadow ? shadow + lo : shadow};
    }
};
// One update launch over x[0, n).  grad_sq: the sum g^2 scalar the clip coefficient is folded from (with its slots); coef_in != null:
// use that precomputed coefficient instead; step_dev != null: take the step count (bias corrections) from that device scalar instead
// of hp->step; opt: the optimizer setting (codae_optimizer; null or the default = Adam with L2 decay and a constant lr, the
// instantiation the launchers always ran); wa: the weight-average setting (null or kind OFF = the instantiations without it; the
// average itself is x.avg - wa->avg is not read here)
struct UpdateLaunch {
    ParamVectors x; int64_t n;
    const codae_hyper* hp; const double* grad_sq; const double* coef_in; const double* step_dev;
    const codae_optimizer* opt; const codae_weight_average* wa;
    int trust_mat;           // LAMB / LARS, the flat kernel: the matrix x[0, n) is (its ratio), -1 = the bias block (ratio 1)
};
// the argument checks both update launchers make, the error texts prefixed with `who`
int check_update_launch(const char* who, const UpdateLaunch& u);
int launch_update(const UpdateLaunch& u, hipStream_t s);      // the flat kernel over x[0, u.n)
// CODAE_E_INVALID as codae_set_weight_average documents (need_avg: the avg pointer is checked too); canonical: only the fields the
// kind reads; launch_weight_average: the stand-alone kernel, nothing launched on a step that does not sample
bool weight_average_is_off(const codae_weight_average* w);
int check_weight_average(const codae_weight_average* w, bool need_avg);
codae_weight_average weight_average_canonical(const codae_weight_average* w);
int launch_weight_average(float* avg, const float* p, int64_t n, const codae_weight_average* wa, int32_t step, hipStream_t s);
// CODAE_E_INVALID as codae_set_optimizer documents; is_default: null, or {ADAM, amsgrad 0, CONSTANT, warmup 0};
// canonical: only the fields the kind and the schedule read, all else zero (the graph key compares bytes)
int check_optimizer(const codae_optimizer* o);
bool optimizer_is_default(const codae_optimizer* o);
codae_optimizer optimizer_canonical(const codae_optimizer* o);
inline bool is_trust_kind(const codae_optimizer* o) { return o != nullptr && (o->kind == CODAE_OPT_LAMB || o->kind == CODAE_OPT_LARS); }
// LAMB / LARS ("Layer-wise trust ratios"): the norms pass over n_mats matrices x[off[l], off[l] + len[l]) and the finish, which leaves
// the fp32 ratios at the head of u.opt->trust_ws - in front of the update launches, on their stream.  The partial pairs a matrix
// leaves behind the ratios: trust_parts_flat(len) from the flat pass, trust_parts_tiled(rows, cols) from the tiled one.
int64_t trust_parts_flat(int64_t n);
int64_t trust_parts_tiled(int rows, int cols);
int launch_trust_norms(const UpdateLaunch& u, int n_mats, const int64_t* off, const int64_t* len, hipStream_t s);
int launch_set_scalar(double* dst, double value, hipStream_t s);
// bf16 engine: Adam over the weight matrices in tiles, writing the bf16 shadow AND (layers >= transposed_from) the
// transposed shadow in the same pass; the flat bias block [bias_off, bias_off + bias_n) rides along (u.n: the whole vector's length; u.coef_in stays null: the kernel takes none)
struct UpdateTiles {
    bf16_t* shadow_t;
    int n_layers; const int64_t* w_off; const int* rows; const int* cols;     // the layer table: element offset and shape of each matrix
    int transposed_from;
    int64_t bias_off, bias_n;
};
int launch_update_tiled(const UpdateLaunch& u, const UpdateTiles& t, hipStream_t s);
int launch_trust_norms_tiled(const UpdateLaunch& u, const UpdateTiles& t, hipStream_t s);      // the same over the update's tile table
// dst[c][r] = src[r][c] for n bf16 matrices (element offsets off[i], shapes rows[i] x cols[i]) in one launch
// tied weights (tied.hip; include/codae_hip.h, "Tied weights"): the fold of the decoder gradients into the encoder's, and the mirror of
// the encoder matrices into the decoder's fp32 image and (when given) its two bf16 shadows
int launch_tie_fold(float* g, const codae_tie_pair* pairs, int n, hipStream_t s);
int launch_tie_mirror(float* p, bf16_t* shadow, bf16_t* shadow_t, const codae_tie_pair* pairs, int n, hipStream_t s);
int launch_transpose_bf16(const bf16_t* src, bf16_t* dst, int n, const int64_t* off, const int* rows, const int* cols,
                          hipStream_t s);
// sumsq != null: += sum out^2 (slot-scattered)
// act != CODAE_ACT_NONE: the generic-activation epilogue (see GemmF32::act; relu is ignored then)
int launch_reduce_slabs_epi(const float* slabs, int n_slabs, int64_t stride, int M, int N, float* C, int64_t ldc, const float* bias,
                            int relu, const float* relu_src, int64_t ld_relu, float* colsum_part, hipStream_t s,
                            int act = CODAE_ACT_NONE, const float* act_p = nullptr);
int launch_reduce_slabs(const float* slabs, int n_slabs, int64_t slab_stride, float* out, int64_t n, double* sumsq,
                        hipStream_t s);
// parts != null: SQ_FULL += sum parts[i][0], SQ_PARTIAL += sum parts[i][1] (fixed order) and the step's loss from
// them; parts == null: the step's sum was accumulated in scalars[STEP_SQ] (dense stand-alone loss)
int launch_finish_loss(double* scalars, double inv_n, hipStream_t s, const double* parts = nullptr, int n_parts = 0);
int launch_cast_f32(const bf16_t* src, float* dst, int64_t n, hipStream_t s);
// out[n] = sum_m src[m][n], rows added in index order (deterministic; stand-alone primitive)
int launch_colsum_f32(const float* src, int M, int N, float* out, hipStream_t s);
// parts[p][n] = sum of rows [64 p, 64 p + 64) of src (first stage of the engine's bias gradient of a dense dy)
int launch_colsum_parts_f32(const float* src, int M, int N, float* parts, hipStream_t s);
// Second stage of every bias gradient: out_j[c] = sum_p parts_j[p][c] (p ascending), up to 64 jobs per launch;
// sumsq != null: += sum out^2 (slot-scattered, clip_grad_norm_)
struct BiasFinishJobs {
    int n;
    const float* parts[64];
    float* out[64];
    int rows[64], cols[64];
    int col_begin[65];       // prefix sum of cols: block -> job lookup
};
// optional last block of the same launch: what finish_loss_kernel does with per-workgroup metric sums, WITHOUT resetting the
// norm accumulators (the chain kernel zeroed them before the weight gradients started adding to them)
struct LossFinish { double* scalars; double inv_n; const double* parts; int n_parts; };
int launch_bias_finish(const BiasFinishJobs& jobs, double* sumsq, hipStream_t s, const LossFinish* loss = nullptr);
// The same finish as TRAILING workgroups of gemm_bf16_pipe_grouped's launch (the fused bf16 step's deferred weight gradients: 480
// tiles on 256 CUs at C3, 32 CUs idle through the second round) instead of a launch of its own behind it: what it reads - the
// partial rows, the loss kernel's sums - was complete before the weight gradients started.  The same bits as launch_bias_finish:
// every column's rows in row order, one float sum of squares per 256 columns added as a double to slot (that block's index & 63),
// the loss sums added by 256 threads in the same order.  At most CODAE_GROUP_MAX jobs: the table travels in the kernel-argument
// block beside the GEMM descriptors (BiasFinishJobs' 64 slots would not fit there).
struct BiasFold {
    int n;
    int rows[CODAE_GROUP_MAX], cols[CODAE_GROUP_MAX];
    int col_begin[CODAE_GROUP_MAX + 1];      // prefix sum of cols
    const float* parts[CODAE_GROUP_MAX];
    float* out[CODAE_GROUP_MAX];
    double* sumsq;                           // as launch_bias_finish's; null = no norm
    LossFinish loss;                         // scalars null = no loss finish
};

}  // namespace codae
