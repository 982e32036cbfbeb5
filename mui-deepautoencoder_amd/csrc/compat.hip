// Assembled outfits and compatibility (include/codae_hip.h, "Assembled outfits and compatibility"): a gather whose source row is chosen
// per (outfit, slot), the per-slot cosine / squared error of a leave-one-out reconstruction against the items it left out, and the
// win / tie counts of an AUC.  Single-pass kernels in gather.hip's discipline: 16 B per lane where the widths allow, a scalar form for
// the rest, grid-stride over a capped grid; no float atomics anywhere.
#include "loss_sweep.h"

namespace codae {
namespace {

constexpr int NT = GRID_NT;
constexpr int WAVES = NT / 64;

// ---- assemble ----------------------------------------------------------------------------------------------------------------------
struct AssembleArgs {
    const void* src;            // [n_rows][io] fp32, or its bf16 image
    const int32_t* items;       // [Q][S]
    const int32_t* blank;       // [Q] or null (single-blank form)
    const uint8_t* present;     // [n_rows][S] (PRES)
    void* out;                  // [rows][out_ld], rows = Q, or Q S in the leave-one-out form
    int64_t n_rows, out_ld;
    int Q, S, E;
};

// X[row][s E + e] = src[items[q][s]][s E + e], +0 where the pair (q, s) is absent or slot s is blanked for this row.  One thread per
// group of W columns (W divides E: a group sits inside one slot); a group that is blanked or absent is stored as zeros and never
// loaded.  An entry outside [0, n_rows) is absent, so no index reaches memory unchecked.
template <int W, bool SRC_BF16, bool OUT_BF16, bool PRES, bool LOO>
__global__ __launch_bounds__(NT) void assemble_outfits_kernel(AssembleArgs a) {
    static_assert(!SRC_BF16 || OUT_BF16, "the bf16 image assembles into bf16 rows");
    static_assert(W != 8 || OUT_BF16, "the 8-wide form writes bf16");
    const int io = a.S * a.E;
    const int cols = io / W;
    const int64_t rows = LOO ? (int64_t)a.Q * a.S : (int64_t)a.Q;
    const int64_t total = rows * cols;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < total; e += (int64_t)gridDim.x * NT) {
        const int64_t row = e / cols;
        const int c = (int)(e - row * cols) * W;
        const int s = c / a.E;
        int q, v;
        if constexpr (LOO) { q = (int)(row / a.S); v = (int)(row - (int64_t)q * a.S); }
        else { q = (int)row; v = a.blank ? a.blank[q] : -1; }
        const int64_t r = a.items[(int64_t)q * a.S + s];
        bool on = r >= 0 && r < a.n_rows && s != v;
        if constexpr (PRES) on = on && a.present[r * a.S + s] != 0;
        const int64_t o = row * a.out_ld + c;
        if constexpr (SRC_BF16) {
            const bf16_t* sp = reinterpret_cast<const bf16_t*>(a.src) + r * io + c;
            bf16_t* op = reinterpret_cast<bf16_t*>(a.out) + o;
            if constexpr (W == 8) *reinterpret_cast<uint4*>(op) = on ? *reinterpret_cast<const uint4*>(sp) : make_uint4(0u, 0u, 0u, 0u);
            else if constexpr (W == 4) *reinterpret_cast<uint2*>(op) = on ? *reinterpret_cast<const uint2*>(sp) : make_uint2(0u, 0u);
            else op[0] = on ? sp[0] : (bf16_t)0;
        } else {
            const float* sp = reinterpret_cast<const float*>(a.src) + r * io + c;
            float x[W];
#pragma unroll
            for (int k = 0; k < W; ++k) x[k] = 0.f;
            if (on) {
                if constexpr (W == 1) x[0] = sp[0];
                else {
#pragma unroll
                    for (int g = 0; g < W / 4; ++g) {
                        const float4 t = *reinterpret_cast<const float4*>(sp + 4 * g);
                        x[4 * g] = t.x; x[4 * g + 1] = t.y; x[4 * g + 2] = t.z; x[4 * g + 3] = t.w;
                    }
                }
            }
            if constexpr (OUT_BF16) {
                bf16_t* op = reinterpret_cast<bf16_t*>(a.out) + o;
                if constexpr (W == 8)
                    *reinterpret_cast<uint4*>(op) = make_uint4(pack_bf16x2(x[0], x[1]), pack_bf16x2(x[2], x[3]), pack_bf16x2(x[4], x[5]), pack_bf16x2(x[6], x[7]));
                else if constexpr (W == 4) *reinterpret_cast<uint2*>(op) = pack_bf16x4(x[0], x[1], x[2], x[3]);
                else op[0] = f32_to_bf16(x[0]);
            } else {
                float* op = reinterpret_cast<float*>(a.out) + o;
                if constexpr (W == 4) *reinterpret_cast<float4*>(op) = make_float4(x[0], x[1], x[2], x[3]);
                else op[0] = x[0];
            }
        }
    }
}

// ---- slot scores -------------------------------------------------------------------------------------------------------------------
// One workgroup per outfit, its waves striding over the slots.  Pair (q, s): x = data[items[q][s]][slot s], y = Y[q S + s][slot s].
// A lane adds its columns in ascending order (4 per 16-byte load in the VEC form), then the wave's xor-shuffle tree: the order depends on
// E and the form alone, never on Q or on where the outfit sits.  Thread 0 then adds the present cosines in ascending slot order.
template <bool VEC, bool PRES>
__global__ __launch_bounds__(NT) void outfit_score_kernel(const float* __restrict__ data, int64_t n_rows, int S, int E,
                                                          const int32_t* __restrict__ items, const uint8_t* __restrict__ present,
                                                          const float* __restrict__ Y, int64_t y_ld, float* __restrict__ cos_out,
                                                          float* __restrict__ sq_out, float* __restrict__ score,
                                                          int32_t* __restrict__ n_present) {
    __shared__ float s_cos[128];
    __shared__ int s_on[128];
    const int q = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int io = S * E;
    for (int s = wave; s < S; s += WAVES) {
        const int64_t r = items[(int64_t)q * S + s];
        bool on = r >= 0 && r < n_rows;                     // (wave-uniform)
        if constexpr (PRES) on = on && present[r * S + s] != 0;
        float cs = 0.f, sqv = 0.f;
        if (on) {
            const float* __restrict__ xp = data + r * io + (int64_t)s * E;
            const float* __restrict__ yp = Y + ((int64_t)q * S + s) * y_ld + (int64_t)s * E;
            float dot = 0.f, nx2 = 0.f, ny2 = 0.f, d2 = 0.f;
            if constexpr (VEC) {
                for (int c = lane * 4; c < E; c += 256) {
                    const float4 xv = *reinterpret_cast<const float4*>(xp + c);
                    const float4 yv = *reinterpret_cast<const float4*>(yp + c);
                    const float xa[4] = {xv.x, xv.y, xv.z, xv.w}, ya[4] = {yv.x, yv.y, yv.z, yv.w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float d = opaque(xa[k] - ya[k]);
                        dot = opaque(__fmaf_rn(xa[k], ya[k], dot));
                        nx2 = opaque(__fmaf_rn(xa[k], xa[k], nx2));
                        ny2 = opaque(__fmaf_rn(ya[k], ya[k], ny2));
                        d2 = opaque(__fmaf_rn(d, d, d2));
                    }
                }
            } else {
                for (int c = lane; c < E; c += 64) {
                    const float xk = xp[c], yk = yp[c];
                    const float d = opaque(xk - yk);
                    dot = opaque(__fmaf_rn(xk, yk, dot));
                    nx2 = opaque(__fmaf_rn(xk, xk, nx2));
                    ny2 = opaque(__fmaf_rn(yk, yk, ny2));
                    d2 = opaque(__fmaf_rn(d, d, d2));
                }
            }
            dot = wave_sum(dot); nx2 = wave_sum(nx2); ny2 = wave_sum(ny2); d2 = wave_sum(d2);
            const float nxr = sqrtf(nx2), nyr = sqrtf(ny2);
            const float nx = nxr < CODAE_COS_EPS ? CODAE_COS_EPS : nxr;     // max(., eps) that keeps a NaN norm a NaN (SLOT_COSINE's form)
            const float ny = nyr < CODAE_COS_EPS ? CODAE_COS_EPS : nyr;
            cs = dot / (nx * ny);
            sqv = d2;
        }
        if (lane == 0) {
            cos_out[(int64_t)q * S + s] = cs;
            sq_out[(int64_t)q * S + s] = sqv;
            s_cos[s] = cs;
            s_on[s] = on ? 1 : 0;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float acc = 0.f;
        int n = 0;
        for (int s = 0; s < S; ++s)
            if (s_on[s]) { acc = opaque(acc + s_cos[s]); ++n; }
        score[q] = n >= 2 ? acc / (float)n : __uint_as_float(0x7fc00000u);
        n_present[q] = n;
    }
}

// ---- AUC counts --------------------------------------------------------------------------------------------------------------------
constexpr int AUC_CHUNK = 4 * NT;       // positives staged per pass: one 16-byte load per lane
constexpr int AUC_MAX_BLOCKS = 2048;

struct AucArgs {
    const float* pos; const uint8_t* pos_on; int P;
    const float* neg; const int32_t* neg_slot; const int32_t* neg_parent; int M;
    int S;
};

// negative j counts iff its slot lies in [0, S) and, when it names a parent and the positives carry flags, that parent is on
__device__ __forceinline__ int auc_live_slot(const AucArgs& a, int slot, int parent) {
    bool on = slot >= 0 && slot < a.S;
    if (a.neg_parent != nullptr && a.pos_on != nullptr) on = on && parent >= 0 && parent < a.P && a.pos_on[parent] != 0;
    return on ? slot : -1;
}

// Every positive against every negative.  A thread owns one NEGATIVE at a time (grid-stride over blocks of NT negatives) - its slot is
// then fixed, so its wins and ties are two registers - and the positives pass through LDS in chunks of AUC_CHUNK: 16-byte loads for a
// whole chunk, scalar loads for the ragged last one; a positive that is off is staged as NaN, which neither wins nor ties.  The inner
// loop is one broadcast 16-byte LDS read and eight compares per four positives, nothing else.  A thread then adds its two counts and
// its paired win to the workgroup's LDS counters [slot][wins, ties, paired wins] with integer LDS atomics (exact in any order).
// parts [gridDim.x][S][3]: plain stores.
// (The first form of this kernel had the roles the other way round - a thread per positive, the negatives staged, one ballot per
// outcome and a read-modify-write of the wave's LDS counters per negative: 16.5 ms for 65 536 x 65 536 against DESIGN.md section 6's
// figure for this one; the dependent LDS round trips per negative were the whole cost.)
template <bool VEC>
__global__ __launch_bounds__(NT) void auc_count_kernel(AucArgs a, unsigned long long* __restrict__ parts) {
    __shared__ __attribute__((aligned(16))) float s_pos[AUC_CHUNK];
    extern __shared__ unsigned long long s_cnt[];      // [S][3]
    const int S = a.S;
    const float nan = __uint_as_float(0x7fc00000u);
    for (int i = threadIdx.x; i < S * 3; i += NT) s_cnt[i] = 0ull;
    const int n_nblocks = (a.M + NT - 1) / NT;
    for (int nb = blockIdx.x; nb < n_nblocks; nb += gridDim.x) {
        const int j = nb * NT + threadIdx.x;
        int sl = -1, par = -1;
        float v = nan;
        if (j < a.M) {
            par = a.neg_parent != nullptr ? a.neg_parent[j] : -1;
            sl = auc_live_slot(a, a.neg_slot[j], par);
            v = a.neg[j];
        }
        uint32_t w = 0u, t = 0u;                           // (at most P < 2^31 each)
        for (int i0 = 0; i0 < a.P; i0 += AUC_CHUNK) {
            const int n = a.P - i0 < AUC_CHUNK ? a.P - i0 : AUC_CHUNK;
            __syncthreads();                               // the previous chunk is consumed (and the counters are cleared)
            if (VEC && n == AUC_CHUNK) {
                const int i = i0 + 4 * threadIdx.x;
                const float4 p = *reinterpret_cast<const float4*>(a.pos + i);
                uint32_t on = 0x01010101u;
                if (a.pos_on != nullptr) on = *reinterpret_cast<const uint32_t*>(a.pos_on + i);
                *reinterpret_cast<float4*>(s_pos + 4 * threadIdx.x) =
                    make_float4((on & 0xffu) ? p.x : nan, (on & 0xff00u) ? p.y : nan, (on & 0xff0000u) ? p.z : nan, (on & 0xff000000u) ? p.w : nan);
            } else {
                for (int k = threadIdx.x; k < n; k += NT) s_pos[k] = (a.pos_on == nullptr || a.pos_on[i0 + k] != 0) ? a.pos[i0 + k] : nan;
            }
            __syncthreads();
            int k = 0;
            for (; k + 4 <= n; k += 4) {
                const float4 p = *reinterpret_cast<const float4*>(s_pos + k);      // (one address for the whole wave: a broadcast)
                w += (p.x > v ? 1u : 0u) + (p.y > v ? 1u : 0u) + (p.z > v ? 1u : 0u) + (p.w > v ? 1u : 0u);
                t += (p.x == v ? 1u : 0u) + (p.y == v ? 1u : 0u) + (p.z == v ? 1u : 0u) + (p.w == v ? 1u : 0u);
            }
            for (; k < n; ++k) {
                const float p = s_pos[k];
                w += p > v ? 1u : 0u;
                t += p == v ? 1u : 0u;
            }
        }
        if (sl >= 0) {
            if (w) atomicAdd(&s_cnt[sl * 3], (unsigned long long)w);
            if (t) atomicAdd(&s_cnt[sl * 3 + 1], (unsigned long long)t);
            if (par >= 0 && par < a.P && (a.pos_on == nullptr || a.pos_on[par] != 0) && a.pos[par] > v) atomicAdd(&s_cnt[sl * 3 + 2], 1ull);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < S * 3; i += NT) parts[(int64_t)blockIdx.x * S * 3 + i] = s_cnt[i];
}

// One workgroup: counts[s] = {wins, ties, pairs, paired wins} from the partial rows in row order, pairs = live positives x live
// negatives of the slot; counts[S] = {live positives, live negatives, 0, 0}.  (Integer LDS atomics count the negatives: exact.)
__global__ __launch_bounds__(NT) void auc_finish_kernel(AucArgs a, const unsigned long long* __restrict__ parts, int n_parts,
                                                        int64_t* __restrict__ counts) {
    extern __shared__ unsigned int s_n[];      // [S] live negatives per slot, [S] = live positives
    const int S = a.S;
    for (int i = threadIdx.x; i <= S; i += NT) s_n[i] = 0u;
    __syncthreads();
    for (int j = threadIdx.x; j < a.M; j += NT) {
        const int sl = auc_live_slot(a, a.neg_slot[j], a.neg_parent != nullptr ? a.neg_parent[j] : -1);
        if (sl >= 0) atomicAdd(&s_n[sl], 1u);
    }
    unsigned int np = 0u;
    for (int i = threadIdx.x; i < a.P; i += NT) np += (a.pos_on == nullptr || a.pos_on[i] != 0) ? 1u : 0u;
    if (np) atomicAdd(&s_n[S], np);
    __syncthreads();
    for (int s = threadIdx.x; s < S; s += NT) {
        unsigned long long w = 0ull, t = 0ull, pw = 0ull;
        for (int b = 0; b < n_parts; ++b) {
            const unsigned long long* row = parts + ((int64_t)b * S + s) * 3;
            w += row[0]; t += row[1]; pw += row[2];
        }
        counts[s * 4] = (int64_t)w;
        counts[s * 4 + 1] = (int64_t)t;
        counts[s * 4 + 2] = (int64_t)s_n[S] * (int64_t)s_n[s];
        counts[s * 4 + 3] = (int64_t)pw;
    }
    if (threadIdx.x == 0) {
        unsigned long long nn = 0ull;
        for (int s = 0; s < S; ++s) nn += s_n[s];
        counts[S * 4] = (int64_t)s_n[S];
        counts[S * 4 + 1] = (int64_t)nn;
        counts[S * 4 + 2] = 0;
        counts[S * 4 + 3] = 0;
    }
}

int check_outfit_shape(const char* who, int io, int n_slots, int Q) {
    CODAE_REQUIRE(n_slots >= 1 && n_slots <= 128, "%s: 1 .. 128 slots, got %d", who, n_slots);
    CODAE_REQUIRE(io > 0 && io % n_slots == 0, "%s: n_slots %d does not divide io %d", who, n_slots, io);
    CODAE_REQUIRE(Q >= 1, "%s: Q %d must be at least 1", who, Q);
    return CODAE_OK;
}

}  // namespace

int auc_blocks(int M) {
    const int b = (M + NT - 1) / NT;
    return b < 1 ? 1 : (b > AUC_MAX_BLOCKS ? AUC_MAX_BLOCKS : b);
}

int launch_assemble_outfits(const void* src, int src_bf16, int64_t n_rows, int io, int n_slots, const int32_t* items, int Q,
                            const int32_t* blank, int leave_one_out, const uint8_t* present, void* out, int out_bf16, int64_t out_ld,
                            hipStream_t s) {
    const int rc = check_outfit_shape("assemble_outfits", io, n_slots, Q);
    if (rc) return rc;
    CODAE_REQUIRE(src && items && out && n_rows > 0, "assemble_outfits: null source, items or output, or no rows");
    CODAE_REQUIRE(!src_bf16 || out_bf16, "assemble_outfits: the bf16 image assembles into bf16 rows only");
    CODAE_REQUIRE(!(leave_one_out && blank), "assemble_outfits: the leave-one-out form takes no blank vector");
    if (out_ld <= 0) out_ld = io;
    CODAE_REQUIRE(out_ld >= io, "assemble_outfits: out_ld %lld below io %d", (long long)out_ld, io);
    const int S = n_slots, E = io / S;
    const int64_t rows = leave_one_out ? (int64_t)Q * S : (int64_t)Q;
    CODAE_REQUIRE(rows <= 0x7fffffff, "assemble_outfits: %lld output rows", (long long)rows);
    // the widest group that sits inside one slot and keeps every access aligned: 16 B on the narrower side
    const int src_es = src_bf16 ? 2 : 4, out_es = out_bf16 ? 2 : 4;
    int W = 1;
    const int widths[2] = {8, 4};
    for (int w : widths) {
        if (w == 8 && !out_bf16) continue;
        const int64_t src_al = w * src_es > 16 ? 16 : w * src_es, out_al = w * out_es > 16 ? 16 : w * out_es;     // bytes per access
        const bool src_ok = reinterpret_cast<uintptr_t>(src) % (uintptr_t)src_al == 0 && ((int64_t)io * src_es) % src_al == 0;
        const bool out_ok = reinterpret_cast<uintptr_t>(out) % (uintptr_t)out_al == 0 && (out_ld * out_es) % out_al == 0;
        if (E % w == 0 && src_ok && out_ok) { W = w; break; }
    }
    const AssembleArgs a{src, items, blank, present, out, n_rows, out_ld, Q, S, E};
    const int grid = grid_for(rows * (io / W));
    auto go = [&](auto Wc, auto SB, auto OB) {
        constexpr int W_ = decltype(Wc)::value;
        constexpr bool SB_ = decltype(SB)::value, OB_ = decltype(OB)::value;
#define ASM(P, L) hipLaunchKernelGGL((assemble_outfits_kernel<W_, SB_, OB_, P, L>), dim3(grid), dim3(NT), 0, s, a)
        if (present) { if (leave_one_out) ASM(true, true); else ASM(true, false); }
        else { if (leave_one_out) ASM(false, true); else ASM(false, false); }
#undef ASM
    };
    auto with_types = [&](auto Wc) {
        if (src_bf16) go(Wc, std::true_type{}, std::true_type{});
        else if (out_bf16) go(Wc, std::false_type{}, std::true_type{});
        else if constexpr (decltype(Wc)::value != 8) go(Wc, std::false_type{}, std::false_type{});
    };
    if (W == 8) with_types(std::integral_constant<int, 8>{});
    else if (W == 4) with_types(std::integral_constant<int, 4>{});
    else with_types(std::integral_constant<int, 1>{});
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_outfit_scores(const float* data, int64_t n_rows, int io, int n_slots, const int32_t* items, int Q, const uint8_t* present,
                         const float* Y, int64_t y_ld, float* cos_out, float* sq_out, float* score, int32_t* n_present, hipStream_t s) {
    const int rc = check_outfit_shape("outfit_scores", io, n_slots, Q);
    if (rc) return rc;
    CODAE_REQUIRE(data && items && Y && cos_out && sq_out && score && n_present && n_rows > 0, "outfit_scores: null argument, or no rows");
    if (y_ld <= 0) y_ld = io;
    CODAE_REQUIRE(y_ld >= io, "outfit_scores: y_ld %lld below io %d", (long long)y_ld, io);
    const int S = n_slots, E = io / S;
    const bool vec = E % 4 == 0 && y_ld % 4 == 0 && a16(data) && a16(Y);
#define OSK(V, P) hipLaunchKernelGGL((outfit_score_kernel<V, P>), dim3(Q), dim3(NT), 0, s, data, n_rows, S, E, items, present, Y, y_ld, cos_out, \
                                     sq_out, score, n_present)
    if (vec) { if (present) OSK(true, true); else OSK(true, false); }
    else { if (present) OSK(false, true); else OSK(false, false); }
#undef OSK
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_auc_counts(const float* pos, const uint8_t* pos_on, int P, const float* neg, const int32_t* neg_slot, const int32_t* neg_parent,
                      int M, int n_slots, void* parts_ws, int64_t* counts, hipStream_t s) {
    CODAE_REQUIRE(n_slots >= 1 && n_slots <= 128, "auc_counts: 1 .. 128 slots, got %d", n_slots);
    CODAE_REQUIRE(P >= 1 && M >= 1, "auc_counts: P %d and M %d must be at least 1", P, M);
    CODAE_REQUIRE(pos && neg && neg_slot && parts_ws && counts, "auc_counts: null argument");
    CODAE_REQUIRE((reinterpret_cast<uintptr_t>(parts_ws) & 7) == 0 && (reinterpret_cast<uintptr_t>(counts) & 7) == 0,
                  "auc_counts: the work space and counts must be 8-byte aligned");
    const AucArgs a{pos, pos_on, P, neg, neg_slot, neg_parent, M, n_slots};
    const int blocks = auc_blocks(M);
    unsigned long long* parts = reinterpret_cast<unsigned long long*>(parts_ws);
    const size_t lds = (size_t)n_slots * 3 * sizeof(unsigned long long);
    const bool vec = a16(pos) && (pos_on == nullptr || (reinterpret_cast<uintptr_t>(pos_on) & 3) == 0);
    if (vec) hipLaunchKernelGGL((auc_count_kernel<true>), dim3(blocks), dim3(NT), lds, s, a, parts);
    else hipLaunchKernelGGL((auc_count_kernel<false>), dim3(blocks), dim3(NT), lds, s, a, parts);
    CODAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(auc_finish_kernel, dim3(1), dim3(NT), (size_t)(n_slots + 1) * sizeof(unsigned int), s, a, parts, blocks, counts);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

}  // namespace codae

using namespace codae;

extern "C" {

int codae_assemble_outfits(const void* src, int32_t src_bf16, int64_t n_rows, int32_t io, int32_t n_slots, const int32_t* items, int32_t Q,
                           const int32_t* blank, int32_t leave_one_out, const uint8_t* present, void* out, int32_t out_bf16, int64_t out_ld,
                           void* stream) {
    return launch_assemble_outfits(src, src_bf16, n_rows, io, n_slots, items, Q, blank, leave_one_out, present, out, out_bf16, out_ld,
                                   (hipStream_t)stream);
}

int codae_outfit_scores(const float* data, int64_t n_rows, int32_t io, int32_t n_slots, const int32_t* items, int32_t Q,
                        const uint8_t* present, const float* Y, int64_t y_ld, float* cos, float* sq, float* score, int32_t* n_present,
                        void* stream) {
    return launch_outfit_scores(data, n_rows, io, n_slots, items, Q, present, Y, y_ld, cos, sq, score, n_present, (hipStream_t)stream);
}

int codae_auc_blocks(int32_t M) { return auc_blocks(M < 1 ? 1 : M); }

int codae_auc_counts(const float* pos, const uint8_t* pos_on, int32_t P, const float* neg, const int32_t* neg_slot,
                     const int32_t* neg_parent, int32_t M, int32_t n_slots, void* parts_ws, int64_t* counts, void* stream) {
    return launch_auc_counts(pos, pos_on, P, neg, neg_slot, neg_parent, M, n_slots, parts_ws, counts, (hipStream_t)stream);
}

}  // extern "C"
