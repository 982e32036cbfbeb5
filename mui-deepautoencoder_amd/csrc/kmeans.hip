// Code clusters (codae_nearest_centroid, codae_centroid_update; include/codae_hip.h, "Code clusters"): the two halves of a Lloyd
// iteration of spherical k-means over a bank of outfit codes.
//   nearest_prepare_kernel<T>          the centroids rounded to the operand type into the work space, [Kpad][Zpad], pads zero
//   nearest_centroid_kernel<T, VEC>    a wave owns 32 bank rows from the first load to the last store: scores of a GROUP of 128
//                                      centroids on the matrix cores (16 accumulator tiles), the winner selected from the
//                                      accumulators, a running (max, index) pair kept across the groups.  No [M][K] matrix, no LDS.
//   update: a counting sort of the rows by (cluster, row) - rank inside chunks of 1024 rows, an exclusive scan over the chunks and the
//   clusters, a scatter - then one workgroup per (cluster, 64 columns) adds its members in ascending row order, and one wave per
//   cluster normalises.  Integer atomics count; every fp32 sum runs in an order fixed by the member list alone.
// T = the operand type of the product: bf16 (v_mfma_f32_16x16x32_bf16) or float (v_mfma_f32_16x16x4_f32, an exact fmaf chain).
// The scores of a row come from one accumulator column that no other row feeds, chunk after chunk of Z in ascending order: a row's
// bits depend on its values, the centroids and Z alone.
#include <math.h>

#include "codae_common.h"
#include "row_sweep.h"

namespace codae {
namespace {

constexpr int NC_WAVES = 4, NC_NT = 64 * NC_WAVES;
constexpr int RT = 2;                      // row tiles (16 rows) of a wave
constexpr int CT = 8;                      // centroid tiles (16 centroids) of a group: RT * CT accumulators of 4 registers
constexpr int WAVE_ROWS = 16 * RT, BLOCK_ROWS = NC_WAVES * WAVE_ROWS, GROUP = 16 * CT;
constexpr int MAX_K = 4096;
constexpr int SORT_CHUNK = 1024, SORT_NT = 256;       // rows per block of the counting sort
constexpr int SUM_COLS = 64, SUM_WAVES = 4;           // columns and waves of a member-sum block

template <typename T> struct Opnd;
// ZC: columns of Z per MFMA step (bf16: one 16x16x32; float: four 16x16x4), LC: the columns of them a lane holds
template <> struct Opnd<bf16_t> { static constexpr int ZC = 32, LC = 8; };
template <> struct Opnd<float> { static constexpr int ZC = 16, LC = 4; };

template <typename T> __device__ __forceinline__ T to_op(float v);
template <> __device__ __forceinline__ float to_op<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16_t to_op<bf16_t>(float v) { return f32_to_bf16(v); }

// ---- nearest centroid --------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void nearest_prepare_kernel(const float* __restrict__ c, int64_t ld_c, int K, int Z, T* __restrict__ cs,
                                                              int Kpad, int Zpad) {
    const int64_t n = (int64_t)Kpad * Zpad;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int k = (int)(i / Zpad), e = (int)(i % Zpad);
        cs[i] = to_op<T>((k < K && e < Z) ? c[(int64_t)k * ld_c + e] : 0.f);      // (caller memory past K or Z is not read)
    }
}

// acc[rt][t] += C^[g0 + 16 t ..][:] . X[rows of tile rt][:]^T over all of Z: lane l, register j of acc[rt][t] = centroid
// g0 + 16 t + 4 (l >> 4) + j against row 16 rt + (l & 15).  cg: this lane's place in the first centroid tile of the group.
template <typename T, bool VEC, bool FULL>
__device__ __forceinline__ void group_scores(f32x4 (&acc)[RT][CT], const float* const (&xr)[RT], int Z, const T* __restrict__ cg, int Zpad,
                                             int nct, int g) {
    constexpr int ZC = Opnd<T>::ZC, LC = Opnd<T>::LC;
    for (int e0 = 0; e0 < Zpad; e0 += ZC) {
        const int col = e0 + LC * g;
        float v[RT][LC];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) load_work<false, VEC, LC>(xr[rt], col, Z, v[rt]);      // (a column past Z: +0, not read)
        if constexpr (sizeof(T) == 2) {
            bf16x8 b[RT];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const u32x4 w = {pack_bf16x2(v[rt][0], v[rt][1]), pack_bf16x2(v[rt][2], v[rt][3]), pack_bf16x2(v[rt][4], v[rt][5]),
                                 pack_bf16x2(v[rt][6], v[rt][7])};
                b[rt] = __builtin_bit_cast(bf16x8, w);
            }
#pragma unroll
            for (int t = 0; t < CT; ++t) {
                if (FULL || t < nct) {
                    const bf16x8 a = *reinterpret_cast<const bf16x8*>(cg + (int64_t)t * 16 * Zpad + e0);
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) acc[rt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[rt], acc[rt][t], 0, 0, 0);
                }
            }
        } else {
#pragma unroll
            for (int t = 0; t < CT; ++t) {
                if (FULL || t < nct) {      // k slot g of product i: column e0 + 4 g + i, on both sides
                    const float4 a = *reinterpret_cast<const float4*>(cg + (int64_t)t * 16 * Zpad + e0);
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        f32x4 s = acc[rt][t];
                        s = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, v[rt][0], s, 0, 0, 0);
                        s = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, v[rt][1], s, 0, 0, 0);
                        s = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, v[rt][2], s, 0, 0, 0);
                        s = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, v[rt][3], s, 0, 0, 0);
                        acc[rt][t] = s;
                    }
                }
            }
        }
    }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(NC_NT) void nearest_centroid_kernel(const float* __restrict__ x, int64_t ld_x, int M, int Z,
                                                                 const T* __restrict__ cs, int Zpad, int K, int Kpad,
                                                                 const float* __restrict__ norm, int64_t* __restrict__ assign,
                                                                 float* __restrict__ best) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int64_t row0 = ((int64_t)blockIdx.x * NC_WAVES + wave) * WAVE_ROWS;
    if (row0 >= M) return;                                     // (no barrier in this kernel: a wave leaves alone)
    const float* xr[RT];
    int64_t row[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        row[rt] = row0 + 16 * rt + r16;
        xr[rt] = x + (row[rt] < M ? row[rt] : (int64_t)M - 1) * ld_x;      // a row past M: the last row again, its result dropped
    }
    float bv[RT];
    int bi[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) { bv[rt] = -INFINITY; bi[rt] = -1; }

    for (int g0 = 0; g0 < Kpad; g0 += GROUP) {
        const int left = (Kpad - g0) >> 4;
        const int nct = left < CT ? left : CT;
        f32x4 acc[RT][CT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int t = 0; t < CT; ++t) acc[rt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
        const T* __restrict__ cg = cs + (int64_t)(g0 + r16) * Zpad + Opnd<T>::LC * g;
        if (nct == CT) group_scores<T, VEC, true>(acc, xr, Z, cg, Zpad, nct, g);
        else group_scores<T, VEC, false>(acc, xr, Z, cg, Zpad, nct, g);
        // the lane's centroids in ascending order: a strict compare keeps the lowest index of equal scores (-0 == +0), a NaN
        // fails every compare and is never taken; the first non-NaN score is taken whatever it is (-inf included)
#pragma unroll
        for (int t = 0; t < CT; ++t) {
            if (t < nct) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int ci = g0 + 16 * t + 4 * g + j;
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        const float d = acc[rt][t][j];
                        const bool take = ci < K && (d > bv[rt] || (bi[rt] < 0 && d == d));      // (a pad centroid never takes part)
                        bv[rt] = take ? d : bv[rt];
                        bi[rt] = take ? ci : bi[rt];
                    }
                }
            }
        }
    }
    // the four lanes of a row: the larger score, the lower index of equal ones; both partners of a stage end with the same pair
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            const float ov = __shfl_xor(bv[rt], o);
            const int oi = __shfl_xor(bi[rt], o);
            const bool take = oi >= 0 && (bi[rt] < 0 || ov > bv[rt] || (ov == bv[rt] && oi < bi[rt]));
            bv[rt] = take ? ov : bv[rt];
            bi[rt] = take ? oi : bi[rt];
        }
        if (g == 0 && row[rt] < M) {
            float b = bv[rt];
            if (norm != nullptr) {
                const float n = norm[row[rt]];
                b = b / (n < CODAE_COS_EPS ? CODAE_COS_EPS : n);
            }
            assign[row[rt]] = bi[rt];
            best[row[rt]] = bi[rt] < 0 ? __int_as_float(0x7fc00000) : b;
        }
    }
}

// ---- centroid update ---------------------------------------------------------------------------------------------------------------
// a row's cluster, or -1 for nobody: -1 itself and anything outside [0, K) (never an index out of bounds)
__device__ __forceinline__ int member_of(const int64_t* __restrict__ assign, int64_t r, int K) {
    const int64_t a = assign[r];
    return (a >= 0 && a < K) ? (int)a : -1;
}

// inrank[r] = how many earlier rows of r's chunk share its cluster; table[chunk][j] = members of cluster j in the chunk
__global__ __launch_bounds__(SORT_NT) void cluster_rank_kernel(const int64_t* __restrict__ assign, int M, int K, int32_t* __restrict__ inrank,
                                                               int32_t* __restrict__ table) {
    __shared__ int32_t a_s[SORT_CHUNK];
    const int64_t base = (int64_t)blockIdx.x * SORT_CHUNK;
    const int n = (int)(M - base < SORT_CHUNK ? M - base : SORT_CHUNK);
    for (int i = threadIdx.x; i < SORT_CHUNK; i += SORT_NT) a_s[i] = i < n ? member_of(assign, base + i, K) : -1;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += SORT_NT) {
        const int a = a_s[i];
        int rank = 0;
        if (a >= 0) {
            for (int p = 0; p < i; ++p) rank += a_s[p] == a ? 1 : 0;
            atomicAdd(&table[(int64_t)blockIdx.x * K + a], 1);
        }
        inrank[base + i] = rank;
    }
}

// one block: table[chunk][j] <- members of j in earlier chunks, counts[j] <- all members, offsets[j] <- members of clusters < j
__global__ __launch_bounds__(1024) void cluster_scan_kernel(int32_t* __restrict__ table, int n_chunks, int K, int64_t* __restrict__ counts,
                                                            int64_t* __restrict__ offsets) {
    __shared__ int64_t part[1024];
    const int tid = threadIdx.x;
    int64_t mine[4];
    int64_t sum = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = 4 * tid + q;
        int64_t run = 0;
        if (j < K) {
            for (int c = 0; c < n_chunks; ++c) {
                const int32_t t = table[(int64_t)c * K + j];
                table[(int64_t)c * K + j] = (int32_t)run;
                run += t;
            }
            counts[j] = run;
        }
        mine[q] = run;
        sum += run;
    }
    part[tid] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {      // inclusive scan of the 1024 partial sums
        const int64_t add = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    int64_t run = part[tid] - sum;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = 4 * tid + q;
        if (j < K) offsets[j] = run;
        run += mine[q];
    }
}

// order[offsets[j] + position of r among the members of j] = r: the rows by (cluster, row)
__global__ __launch_bounds__(256) void cluster_scatter_kernel(const int64_t* __restrict__ assign, int M, int K, const int32_t* __restrict__ inrank,
                                                              const int32_t* __restrict__ table, const int64_t* __restrict__ offsets,
                                                              int32_t* __restrict__ order) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < M; r += (int64_t)gridDim.x * blockDim.x) {
        const int a = member_of(assign, r, K);
        if (a >= 0) order[offsets[a] + table[(r / SORT_CHUNK) * K + a] + inrank[r]] = (int32_t)r;
    }
}

// sums[j][col] = sum over the members of j of x[r][col] / max(n_r, eps): wave w adds members w, w + 4, .. in ascending order, the four
// partial sums are combined as (0 + 1) + (2 + 3)
__global__ __launch_bounds__(64 * SUM_WAVES) void cluster_sum_kernel(const float* __restrict__ x, int64_t ld_x, int Z, const float* __restrict__ norm,
                                                                     const int32_t* __restrict__ order, const int64_t* __restrict__ offsets,
                                                                     const int64_t* __restrict__ counts, float* __restrict__ sums) {
    __shared__ float part[SUM_WAVES][SUM_COLS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = blockIdx.x, col = blockIdx.y * SUM_COLS + lane;
    const int64_t n = counts[j];
    if (n == 0) return;                                        // (block-uniform; an empty cluster's sums are never read)
    const int32_t* __restrict__ mem = order + offsets[j];
    float s = 0.f;
    if (col < Z) {
        for (int64_t m = wave; m < n; m += SUM_WAVES) {
            const int64_t r = mem[m];
            const float nr = norm[r];
            s = opaque(s + x[r * ld_x + col] / (nr < CODAE_COS_EPS ? CODAE_COS_EPS : nr));
        }
    }
    part[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && col < Z) sums[(int64_t)j * Z + col] = opaque(part[0][lane] + part[1][lane]) + opaque(part[2][lane] + part[3][lane]);
}

// c_out[j] = sums[j] / max(|sums[j]|, eps), or c_in[j] bit for bit when the cluster is empty; one wave per cluster, |.| as the export
// kernel forms a row norm: a lane's columns in ascending order, the 64 lanes in one fixed tree
__global__ __launch_bounds__(64) void cluster_finish_kernel(const float* __restrict__ sums, int Z, const int64_t* __restrict__ counts,
                                                            const float* c_in, float* c_out, int64_t ld_c) {
    const int j = blockIdx.x, lane = threadIdx.x;
    if (counts[j] == 0) {
        if (c_in != c_out) {
            const uint32_t* src = reinterpret_cast<const uint32_t*>(c_in) + (int64_t)j * ld_c;
            uint32_t* dst = reinterpret_cast<uint32_t*>(c_out) + (int64_t)j * ld_c;
            for (int e = lane; e < Z; e += 64) dst[e] = src[e];
        }
        return;
    }
    const float* __restrict__ sj = sums + (int64_t)j * Z;
    float n2 = 0.f;
    for (int e = lane; e < Z; e += 64) { const float v = sj[e]; n2 = opaque(__fmaf_rn(v, v, n2)); }
    n2 = wave_sum(n2);
    const float nr = sqrtf(n2);
    const float nn = nr < CODAE_COS_EPS ? CODAE_COS_EPS : nr;
    for (int e = lane; e < Z; e += 64) c_out[(int64_t)j * ld_c + e] = sj[e] / nn;
}

struct UpdateWs { int n_chunks; int64_t sums_off, offsets_off, inrank_off, order_off, table_off, table_bytes, bytes; };
UpdateWs update_ws(int M, int Z, int K) {
    UpdateWs w;
    w.n_chunks = (M + SORT_CHUNK - 1) / SORT_CHUNK;
    w.sums_off = 0;
    w.offsets_off = round_up((int64_t)K * Z * 4, 16);
    w.inrank_off = w.offsets_off + round_up((int64_t)K * 8, 16);
    w.order_off = w.inrank_off + round_up((int64_t)M * 4, 16);
    w.table_off = w.order_off + round_up((int64_t)M * 4, 16);
    w.table_bytes = (int64_t)w.n_chunks * K * 4;
    w.bytes = w.table_off + round_up(w.table_bytes, 16);
    return w;
}

int check_shape(const char* who, int M, int Z, int K) {
    CODAE_REQUIRE(K >= 1 && K <= MAX_K, "%s: K %d outside [1, %d]", who, K, MAX_K);
    CODAE_REQUIRE(M >= 1, "%s: M %d must be >= 1", who, M);
    CODAE_REQUIRE(Z >= 1, "%s: Z %d must be >= 1", who, Z);
    return CODAE_OK;
}

}  // namespace
}  // namespace codae

using namespace codae;

int64_t codae_nearest_centroid_ws_bytes(int32_t Z, int32_t K, int32_t op_bf16) {
    if (Z < 1 || K < 1 || K > MAX_K || (op_bf16 != 0 && op_bf16 != 1)) return -1;
    const int64_t zc = op_bf16 ? Opnd<bf16_t>::ZC : Opnd<float>::ZC;
    return round_up(K, 16) * round_up(Z, zc) * (op_bf16 ? 2 : 4);
}

int codae_nearest_centroid(const float* x, int64_t ld_x, int32_t M, int32_t Z, const float* c, int64_t ld_c, int32_t K, int32_t op_bf16,
                           const float* norm, int64_t* assign, float* best, void* ws, void* stream) {
    int rc = check_shape("codae_nearest_centroid", M, Z, K);
    if (rc) return rc;
    CODAE_REQUIRE(op_bf16 == 0 || op_bf16 == 1, "codae_nearest_centroid: op_bf16 %d is neither 0 nor 1", op_bf16);
    CODAE_REQUIRE(ld_x >= Z, "codae_nearest_centroid: ld_x %lld below Z %d", (long long)ld_x, Z);
    CODAE_REQUIRE(ld_c >= Z, "codae_nearest_centroid: ld_c %lld below Z %d", (long long)ld_c, Z);
    CODAE_REQUIRE(x != nullptr && c != nullptr && assign != nullptr && best != nullptr, "codae_nearest_centroid: a NULL x, c, assign or best");
    CODAE_REQUIRE(ws != nullptr && aligned16(ws), "codae_nearest_centroid: ws %p missing or not 16-byte aligned", ws);
    hipStream_t s = (hipStream_t)stream;
    const int Kpad = (int)round_up(K, 16);
    const int Zpad = (int)round_up(Z, op_bf16 ? Opnd<bf16_t>::ZC : Opnd<float>::ZC);
    const int grid = (int)(((int64_t)M + BLOCK_ROWS - 1) / BLOCK_ROWS);
    const bool vec = rows_vec16(0, Z, {{x, ld_x}});
    const int prep = grid_for((int64_t)Kpad * Zpad);
#define NEAREST(T, V)                                                                                                                   \
    do {                                                                                                                                 \
        hipLaunchKernelGGL(nearest_prepare_kernel<T>, dim3(prep), dim3(256), 0, s, c, ld_c, K, Z, reinterpret_cast<T*>(ws), Kpad, Zpad); \
        CODAE_LAUNCH_CHECK();                                                                                                            \
        hipLaunchKernelGGL((nearest_centroid_kernel<T, V>), dim3(grid), dim3(NC_NT), 0, s, x, ld_x, M, Z, reinterpret_cast<const T*>(ws), \
                           Zpad, K, Kpad, norm, assign, best);                                                                           \
    } while (0)
    if (op_bf16) { if (vec) NEAREST(bf16_t, true); else NEAREST(bf16_t, false); }
    else { if (vec) NEAREST(float, true); else NEAREST(float, false); }
#undef NEAREST
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int64_t codae_centroid_update_ws_bytes(int32_t M, int32_t Z, int32_t K) {
    if (M < 1 || Z < 1 || K < 1 || K > MAX_K) return -1;
    return update_ws(M, Z, K).bytes;
}

int codae_centroid_update(const float* x, int64_t ld_x, int32_t M, int32_t Z, const float* norm, const int64_t* assign, const float* c_in,
                          float* c_out, int64_t ld_c, int32_t K, int64_t* counts, void* ws, void* stream) {
    int rc = check_shape("codae_centroid_update", M, Z, K);
    if (rc) return rc;
    CODAE_REQUIRE(ld_x >= Z, "codae_centroid_update: ld_x %lld below Z %d", (long long)ld_x, Z);
    CODAE_REQUIRE(ld_c >= Z, "codae_centroid_update: ld_c %lld below Z %d", (long long)ld_c, Z);
    CODAE_REQUIRE(x != nullptr && norm != nullptr && assign != nullptr && c_in != nullptr && c_out != nullptr && counts != nullptr,
                  "codae_centroid_update: a NULL x, norm, assign, c_in, c_out or counts");
    CODAE_REQUIRE(ws != nullptr && aligned16(ws), "codae_centroid_update: ws %p missing or not 16-byte aligned", ws);
    hipStream_t s = (hipStream_t)stream;
    const UpdateWs w = update_ws(M, Z, K);
    unsigned char* base = reinterpret_cast<unsigned char*>(ws);
    float* sums = reinterpret_cast<float*>(base + w.sums_off);
    int64_t* offsets = reinterpret_cast<int64_t*>(base + w.offsets_off);
    int32_t* inrank = reinterpret_cast<int32_t*>(base + w.inrank_off);
    int32_t* order = reinterpret_cast<int32_t*>(base + w.order_off);
    int32_t* table = reinterpret_cast<int32_t*>(base + w.table_off);
    CODAE_HIP_CHECK(hipMemsetAsync(table, 0, (size_t)w.table_bytes, s));
    hipLaunchKernelGGL(cluster_rank_kernel, dim3(w.n_chunks), dim3(SORT_NT), 0, s, assign, M, K, inrank, table);
    CODAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(cluster_scan_kernel, dim3(1), dim3(1024), 0, s, table, w.n_chunks, K, counts, offsets);
    CODAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(cluster_scatter_kernel, dim3(grid_for(M)), dim3(256), 0, s, assign, M, K, inrank, table, offsets, order);
    CODAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(cluster_sum_kernel, dim3(K, (Z + SUM_COLS - 1) / SUM_COLS), dim3(64 * SUM_WAVES), 0, s, x, ld_x, Z, norm, order, offsets,
                       counts, sums);
    CODAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(cluster_finish_kernel, dim3(K), dim3(64), 0, s, sums, Z, counts, c_in, c_out, ld_c);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}
