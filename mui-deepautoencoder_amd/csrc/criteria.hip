// "Next" rows of the scope table: the abalone training loss
// (CombinedCriterion, codae/tool/metering.py:82-180 of the reference) and the validation rank
// metric (RankingLoss, metering.py:29-79) as HIP kernels.  Small, HBM/latency-bound work: one pass
// per kernel, no GEMM reshaping.
#include "codae_common.h"

namespace codae {
namespace {

constexpr int NT = GRID_NT;

__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// log-softmax of y[p .. p+s) evaluated at index t (numerically as torch.log_softmax)
__device__ __forceinline__ float log_softmax_at(const float* __restrict__ yr, int p, int s, int t) {
    float m = yr[p];
    for (int k = 1; k < s; ++k) m = fmaxf(m, yr[p + k]);
    float se = 0.f;
    for (int k = 0; k < s; ++k) se += expf(yr[p + k] - m);
    return (yr[p + t] - m) - logf(se);
}
__device__ __forceinline__ int argmax_first(const float* __restrict__ xr, int p, int s) {
    int t = 0;
    float best = xr[p];
    for (int k = 1; k < s; ++k)
        if (xr[p + k] > best) { best = xr[p + k]; t = k; }
    return t;
}

// pass 1: acc[v] = sum over the batch of  sum_s (x-y)^2   (regression)
//                                        -log_softmax(y)[argmax x]   (classification)
__global__ __launch_bounds__(NT) void combined_reduce_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                             int B, int io, int nv, const int32_t* __restrict__ pos,
                                                             const int32_t* __restrict__ size,
                                                             const int32_t* __restrict__ type, double* __restrict__ acc) {
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < (int64_t)B * nv; e += (int64_t)gridDim.x * NT) {
        const int b = (int)(e / nv), v = (int)(e - (int64_t)b * nv);
        const float* xr = x + (int64_t)b * io;
        const float* yr = y + (int64_t)b * io;
        const int p = pos[v], s = size[v];
        float val = 0.f;
        if (type[v] == 0) {
            for (int k = 0; k < s; ++k) { const float d = xr[p + k] - yr[p + k]; val += d * d; }
        } else {
            val = -log_softmax_at(yr, p, s, argmax_first(xr, p, s));
        }
        atomicAdd(&acc[v], (double)val);
    }
}

// pass 2: loss = (1/nv) sum_v w_v L_v, L_v = sqrt(acc_v / (B s)) or acc_v / B; dy = dloss/dy
__global__ __launch_bounds__(NT) void combined_grad_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                           int B, int io, int nv, const int32_t* __restrict__ pos,
                                                           const int32_t* __restrict__ size,
                                                           const int32_t* __restrict__ type,
                                                           const float* __restrict__ weight,
                                                           const double* __restrict__ acc, float* __restrict__ dy,
                                                           double* __restrict__ loss_out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double loss = 0.0;
        for (int v = 0; v < nv; ++v) {
            const double lv = type[v] == 0 ? sqrt(acc[v] / ((double)B * size[v])) : acc[v] / (double)B;
            loss += (double)weight[v] * lv;
        }
        *loss_out = loss / nv;
    }
    if (dy == nullptr) return;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < (int64_t)B * nv; e += (int64_t)gridDim.x * NT) {
        const int b = (int)(e / nv), v = (int)(e - (int64_t)b * nv);
        const float* xr = x + (int64_t)b * io;
        const float* yr = y + (int64_t)b * io;
        float* gr = dy + (int64_t)b * io;
        const int p = pos[v], s = size[v];
        const float c = weight[v] / (float)nv;
        if (type[v] == 0) {
            const float rmse = (float)sqrt(acc[v] / ((double)B * s));
            const float k0 = c / ((float)B * (float)s * rmse);
            for (int k = 0; k < s; ++k) gr[p + k] = k0 * (yr[p + k] - xr[p + k]);
        } else {
            const int t = argmax_first(xr, p, s);
            float m = yr[p];
            for (int k = 1; k < s; ++k) m = fmaxf(m, yr[p + k]);
            float se = 0.f;
            for (int k = 0; k < s; ++k) se += expf(yr[p + k] - m);
            for (int k = 0; k < s; ++k) gr[p + k] = c * (expf(yr[p + k] - m) / se - (k == t ? 1.f : 0.f)) / (float)B;
        }
    }
}

// monitor criterion (reduction "none", metering.py:131-152): out[b][v] = (x-y)^2 (size-1 regression) | NLL
__global__ __launch_bounds__(NT) void combined_full_kernel(const float* __restrict__ x, const float* __restrict__ y, int B,
                                                           int io, int nv, const int32_t* __restrict__ pos,
                                                           const int32_t* __restrict__ size,
                                                           const int32_t* __restrict__ type, float* __restrict__ out) {
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < (int64_t)B * nv; e += (int64_t)gridDim.x * NT) {
        const int b = (int)(e / nv), v = (int)(e - (int64_t)b * nv);
        const float* xr = x + (int64_t)b * io;
        const float* yr = y + (int64_t)b * io;
        const int p = pos[v], s = size[v];
        float val;
        if (type[v] == 0) { const float d = xr[p] - yr[p]; val = d * d; }
        else val = -log_softmax_at(yr, p, s, argmax_first(xr, p, s));
        out[e] = val;
    }
}

// Per-step accounting of the abalone sweep (train_dae_on_abalone.py:227-236): ONE workgroup; thread (r, v) walks rows r, r + R,
// ... of variable v and keeps {f_k, p_k}[k] for its variable in LDS (its own slots: no atomics); thread v then adds the R
// partials of its variable in row-lane order and folds them into the fp64 tables - every addition in a fixed order.
constexpr int MON_KMAX = 16;
__global__ __launch_bounds__(NT) void monitor_accumulate_kernel(const float* __restrict__ x, const float* __restrict__ y, int B, int io, int nv,
                                                                const int32_t* __restrict__ pos, const int32_t* __restrict__ size,
                                                                const int32_t* __restrict__ type, const float* __restrict__ us,
                                                                const float* __restrict__ um, const int32_t* __restrict__ mask_id,
                                                                const uint8_t* __restrict__ table, const int32_t* __restrict__ k_of_mask,
                                                                int k_max, double* __restrict__ acc) {
    extern __shared__ double part[];                     // [NT][2 * k_max]
    const int R = NT / nv;                               // row lanes (host checks nv <= NT)
    const int r = threadIdx.x / nv, v = threadIdx.x - r * nv;
    double* mine = part + (size_t)threadIdx.x * 2 * k_max;
    for (int k = 0; k < 2 * k_max; ++k) mine[k] = 0.0;
    if (r < R) {
        const int p = pos[v], s = size[v], t = type[v];
        for (int b = r; b < B; b += R) {
            const float* xr = x + (int64_t)b * io;
            const float* yr = y + (int64_t)b * io;
            float val;
            if (t == 0) {
                const float sc = us ? us[p] : 1.f, mn = um ? um[p] : 0.f;
                const float xu = xr[p] * sc + mn, yu = yr[p] * sc + mn;      // (data * scale) + min, fp32, as torch
                const float d = xu - yu;
                val = d * d;
            } else {
                val = -log_softmax_at(yr, p, s, argmax_first(xr, p, s));     // (one-hot columns are not de-normalised)
            }
            const int id = mask_id[b];
            const int k = k_of_mask[id] - 1;
            if (k >= 0 && k < k_max) {
                mine[k] += (double)val;
                if (table[(int64_t)id * io + p] == 0) mine[k_max + k] += (double)val;
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < nv) {
        for (int k = 0; k < 2 * k_max; ++k) {
            double t = 0.0;
            for (int rr = 0; rr < R; ++rr) t += part[(size_t)(rr * nv + threadIdx.x) * 2 * k_max + k];
            acc[2 + (int64_t)k * nv + threadIdx.x] += t;
            part[(size_t)threadIdx.x * 2 * k_max + k] = t;       // (slot of row lane 0: read back by thread 0 below)
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double f = 0.0, pp = 0.0;
        for (int k = 0; k < k_max; ++k)
            for (int vv = 0; vv < nv; ++vv) { f += part[(size_t)vv * 2 * k_max + k]; pp += part[(size_t)vv * 2 * k_max + k_max + k]; }
        acc[0] += f; acc[1] += pp;
    }
}

// ||row||_2 of a [rows][E] matrix, one wave per row
__global__ __launch_bounds__(NT) void row_norm_kernel(const float* __restrict__ m, int64_t rows, int E, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4) {
        const float* p = m + r * E;
        float s = 0.f;
        for (int k = lane; k < E; k += 64) s += p[k] * p[k];
        s = wave_sum_f(s);
        if (lane == 0) out[r] = sqrtf(s);
    }
}

// RankingLoss.get (metering.py:46-79): one workgroup per batch sample.
//   c     = blanked slot = sum_s s * (1 - fmask[b][s*E])                       (metering.py:56)
//   s_j   = cos(inventory[c][j], prediction[b][cE:(c+1)E])                      (:66-68)
//   rank  = #{ j in validation : s[idx_b] > s_j }                               (:72-75)
//   out  += 1 - rank / (V - 1)                                                  (:77)
__global__ __launch_bounds__(NT) void ranking_kernel(const float* __restrict__ pred, const float* __restrict__ fmask,
                                                     const int32_t* __restrict__ idx, int io, int S, int E,
                                                     const float* __restrict__ inv, const float* __restrict__ inv_norm,
                                                     int64_t n_obs, const int32_t* __restrict__ val, int V,
                                                     double* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float q[];   // [E] + 8 scratch
    __shared__ float red[8];
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int c = 0;
    for (int s = 1; s < S; ++s) c += (fmask[(int64_t)b * io + (int64_t)s * E] == 0.f) ? s : 0;
    const float* pq = pred + (int64_t)b * io + (int64_t)c * E;
    float sq = 0.f;
    for (int k = threadIdx.x; k < E; k += NT) { const float v = pq[k]; q[k] = v; sq += v * v; }
    sq = wave_sum_f(sq);
    if (lane == 0) red[w] = sq;
    __syncthreads();
    const float qn = fmaxf(sqrtf(red[0] + red[1] + red[2] + red[3]), 1e-8f);
    const float* invc = inv + (int64_t)c * n_obs * E;
    const float* nrmc = inv_norm + (int64_t)c * n_obs;
    // own similarity (every wave computes it: cheaper than another barrier)
    const int64_t me = idx[b];
    float d = 0.f;
    for (int k = lane; k < E; k += 64) d += q[k] * invc[me * E + k];
    d = wave_sum_f(d);
    const float own = d / (qn * fmaxf(nrmc[me], 1e-8f));
    int rank = 0;
    for (int j = w; j < V; j += 4) {
        const int64_t r = val[j];
        const float* pr = invc + r * E;
        float dj = 0.f;
        for (int k = lane; k < E; k += 64) dj += q[k] * pr[k];
        dj = wave_sum_f(dj);
        const float sj = dj / (qn * fmaxf(nrmc[r], 1e-8f));
        rank += (own > sj) ? 1 : 0;
    }
    __syncthreads();
    if (lane == 0) red[4 + w] = (float)rank;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double total = (double)red[4] + red[5] + red[6] + red[7];
        atomicAdd(out, 1.0 - total / (double)(V - 1));
    }
}


// ---- RankingLoss as a GEMM --------------------------------------------------------------------------
// The wave-per-item kernel above reads the whole validation inventory once PER SAMPLE (V x E floats: 53 MB at C3's
// shape, 1.4 TB per validation epoch - 20x the training epoch).  Here the similarities of a whole batch against a chunk
// of the validation inventory are one exact-fp32 MFMA GEMM per slot (gemm_f32.hip: pred[:, cE:(c+1)E] . inv_val_c^T),
// followed by a compare-count pass; the batch's mask ids come from the Corrupter's device tables, nothing goes
// through the host, and *out accumulates over the batches of an epoch.
//   rs[b] = {slot c, |q| clamped, own similarity, rank so far}
struct RankRow { int slot; float qn; float own; int rank; int self_col; int pad[3]; };      // pad[1]: duplicate group of the own row or -1

// one wave per sample: blanked slot from the mask table (metering.py:56: sum of the blanked slots' indices), |q|, s[idx_b]
__global__ __launch_bounds__(NT) void rank_prep_kernel(const float* __restrict__ pred, const int32_t* __restrict__ row_idx,
                                                       const int32_t* __restrict__ mask_id, const int32_t* __restrict__ mask_to_use,
                                                       int nb_run, int run, const uint8_t* __restrict__ mask_table, int B, int io, int S,
                                                       int E, const float* __restrict__ inv, const float* __restrict__ inv_norm,
                                                       int64_t n_obs, const int32_t* __restrict__ val_pos, const int32_t* __restrict__ val_group,
                                                       int n_val, RankRow* __restrict__ rs, int32_t* __restrict__ perm,
                                                       int32_t* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (b >= B) return;
    const int64_t me = row_idx[b];
    const int id = mask_id ? mask_id[b] : mask_to_use[me * nb_run + run];
    int c = 0;
    for (int s = 1; s < S; ++s) c += (mask_table[(int64_t)id * io + (int64_t)s * E] == 0) ? s : 0;
    c = c < S ? c : S - 1;                       // (k > 1 blanks several slots; the reference's formula is meant for k = 1)
    const float* q = pred + (int64_t)b * io + (int64_t)c * E;
    const float* r = inv + ((int64_t)c * n_obs + me) * E;
    float sq = 0.f, d = 0.f;
    for (int k = lane; k < E; k += 64) { const float v = q[k]; sq += v * v; d += v * r[k]; }
    sq = wave_sum_f(sq); d = wave_sum_f(d);
    if (lane == 0) {
        const float qn = fmaxf(sqrtf(sq), 1e-8f);
        RankRow o; o.slot = c; o.qn = qn; o.own = d / (qn * fmaxf(inv_norm[(int64_t)c * n_obs + me], 1e-8f)); o.rank = 0;
        // The sample's own row, when it is a validation row, is never counted by the reference: s[idx] > s[idx] compares a
        // value with itself.  Here `own` and the GEMM's column for that row are summed in different orders, so that
        // column is skipped by position instead.
        o.self_col = val_pos ? val_pos[me] : -1;
        // the rows of one slot, compacted (in arrival order: which GEMM row a sample lands on does not change its rank)
        const int k = atomicAdd(&counts[c], 1);
        perm[(int64_t)c * B + k] = b;
        // rows of the inventory that are exact copies of the sample's own row are never counted either (see codae_hip.h)
        o.pad[0] = k; o.pad[1] = (val_group && o.self_col >= 0) ? val_group[(int64_t)c * n_val + o.self_col] : -1; o.pad[2] = 0;
        rs[b] = o;
    }
}

// compact rows of slot c (k < counts[c]; sample perm[c][k]): rank += #{ j < n : own > dots[k][j] / (|q| |inv_j|) }; one wave per row
__global__ __launch_bounds__(NT) void rank_count_kernel(const float* __restrict__ dots, int64_t ld, int B, int n, int c, int v0,
                                                        const float* __restrict__ val_norm, const int32_t* __restrict__ group,
                                                        RankRow* __restrict__ rs, const int32_t* __restrict__ perm,
                                                        const int32_t* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (k >= counts[c]) return;
    const int b = perm[(int64_t)c * B + k];
    const RankRow me = rs[b];
    const float* d = dots + (int64_t)k * ld;
    int cnt = 0;
    const int skip = me.self_col - v0;
    const int grp = me.pad[1];          // (group: this chunk's slice of the slot's duplicate-group ids, or null)
    for (int j = lane; j < n; j += 64) {
        const bool same = (j == skip) || (group != nullptr && grp >= 0 && group[j] == grp);
        cnt += (!same && me.own > d[j] / (me.qn * fmaxf(val_norm[j], 1e-8f))) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) rs[b].rank = me.rank + cnt;
}

// q[k][:] = pred[perm[c][k]][cE:(c+1)E] for k < counts[c]: the slot's queries, contiguous (the GEMM's A operand)
__global__ __launch_bounds__(NT) void rank_gather_q_kernel(const float* __restrict__ pred, int io, int E, int B, int c,
                                                           const int32_t* __restrict__ perm, const int32_t* __restrict__ counts,
                                                           float* __restrict__ q) {
    const int n = counts[c];
    const int64_t total = (int64_t)n * E;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < total; e += (int64_t)gridDim.x * NT) {
        const int k = (int)(e / E), x = (int)(e - (int64_t)k * E);
        q[e] = pred[(int64_t)perm[(int64_t)c * B + k] * io + (int64_t)c * E + x];
    }
}

// *out += sum_b 1 - rank_b / (V - 1), rows added in index order (one workgroup: the same bits every run)
__global__ __launch_bounds__(NT) void rank_finish_kernel(const RankRow* __restrict__ rs, int B, int V, double* __restrict__ out) {
    __shared__ double red[NT];
    double t = 0.0;
    for (int b = threadIdx.x; b < B; b += NT) t += 1.0 - (double)rs[b].rank / (double)(V - 1);
    red[threadIdx.x] = t;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out += red[0];
}

// rows val[j] of every slot's inventory, contiguous: dst[c][j][:] = inv[c][val[j]][:]
__global__ __launch_bounds__(NT) void gather_rows_kernel(const float* __restrict__ inv, int64_t n_obs, int E, int S,
                                                         const int32_t* __restrict__ val, int V, float* __restrict__ dst) {
    const int64_t total = (int64_t)S * V * E;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < total; e += (int64_t)gridDim.x * NT) {
        const int k = (int)(e % E);
        const int64_t cj = e / E;
        const int j = (int)(cj % V), c = (int)(cj / V);
        dst[e] = inv[((int64_t)c * n_obs + val[j]) * E + k];
    }
}

// ---- complementarity inference: top-k retrieval for a blanked slot -------------------------------------------------
// Candidates are ranked by a 64-bit key with one total order and no comparator branches:
//   key = orderable(score) << 32 | ~column,   orderable: the IEEE bits flipped so that unsigned order = float order
// -0 is folded to +0 first, NaN never gets a key.  Higher key = better: score descending, then column ascending (the
// tables keep candidates in ascending dataset-row order, so that is ascending row id).  Every finite or infinite score maps
// to a key > 0, so 0 marks an empty slot of the state.
__device__ __forceinline__ uint64_t topk_key(float s, int col) {
    uint32_t u = (s == 0.f) ? 0u : __float_as_uint(s);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((uint64_t)u << 32) | (uint32_t)~(uint32_t)col;
}
__device__ __forceinline__ float topk_key_score(uint64_t key) {
    const uint32_t u = (uint32_t)(key >> 32);
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// LDS written by one lane and read by another lane of the SAME wave: LDS operations of a wave complete in order, so a
// compiler fence at wavefront scope is all that is needed (what HIP's __syncwarp expands to)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

constexpr int TK_WAVES = NT / 64;
constexpr int TK_UNROLL = 4;             // columns in flight per lane (loads issued before the first compare)

// top[0, KP) descending  U  buf[0, KP) (unsorted, empty entries 0)  ->  top = the KP best of both, descending; buf = 0.
// Bitonic: sort buf ascending, keep the element-wise max (the upper half of a half-cleaner on top || buf: bitonic, and it
// holds the KP largest), then one bitonic merge down to descending order.
template <int KP>
__device__ __forceinline__ void topk_merge_lds(uint64_t* top, uint64_t* buf, int lane) {
    for (int size = 2; size <= KP; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
#pragma unroll
            for (int t = lane; t < KP / 2; t += 64) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const bool up = (i & size) == 0;
                const uint64_t a = buf[i], c = buf[j];
                if ((a > c) == up) { buf[i] = c; buf[j] = a; }
            }
            wave_lds_sync();
        }
    }
#pragma unroll
    for (int t = lane; t < KP; t += 64) {
        const uint64_t a = top[t], c = buf[t];
        top[t] = a > c ? a : c;
        buf[t] = 0;
    }
    wave_lds_sync();
    for (int stride = KP / 2; stride > 0; stride >>= 1) {
#pragma unroll
        for (int t = lane; t < KP / 2; t += 64) {
            const int i = 2 * t - (t & (stride - 1)), j = i + stride;
            const uint64_t a = top[i], c = top[j];
            if (a < c) { top[i] = c; top[j] = a; }
        }
        wave_lds_sync();
    }
}

// Running top-k over one chunk of a score matrix, one wave per score row r < min(rows, *rows_dev).  The row's state
// (k keys, descending, at state[b * k], b = row_map ? row_map[r] : r) is loaded into LDS; lanes read the row with stride 64
// (coalesced), drop a score at once when its key does not beat the current k-th key (a register), and append survivors to a
// per-wave LDS buffer at a ballot / mbcnt prefix.  A full buffer, and the end of the chunk, is merged into the state
// (topk_merge_lds), which raises the threshold.  Scores are read once; only the k keys are written back.
//   s = scores[r][j]                                         (raw; the selection primitive)
//   s = scores[r][j] / (row_norm[b] * max(col_norm[j], 1e-8))  (col_norm != null: cosine from GEMM dot products, as rank_count_kernel)
// Column j is candidate col0 + j; the candidate skip_col[b] (a global column, -1 = none) is skipped by position.
template <int KP>
__global__ __launch_bounds__(NT) void topk_merge_kernel(const float* __restrict__ scores, int64_t ld, int rows,
                                                        const int32_t* __restrict__ rows_dev, int n, int col0, int k,
                                                        const int32_t* __restrict__ row_map, const float* __restrict__ row_norm,
                                                        const float* __restrict__ col_norm, const int32_t* __restrict__ skip_col,
                                                        uint64_t* __restrict__ state) {
    __shared__ uint64_t lds[TK_WAVES][2 * KP];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r = blockIdx.x * TK_WAVES + w;
    const int nrows = rows_dev ? min(rows, *rows_dev) : rows;
    if (r >= nrows) return;
    const int b = row_map ? row_map[r] : r;
    uint64_t* top = lds[w];
    uint64_t* buf = lds[w] + KP;
    uint64_t* st = state + (int64_t)b * k;
    for (int i = lane; i < KP; i += 64) { top[i] = i < k ? st[i] : 0; buf[i] = 0; }
    wave_lds_sync();
    uint64_t thr = top[k - 1];
    const int skip = skip_col ? skip_col[b] : -1;
    const float qs = row_norm ? row_norm[b] : 1.f;
    const float* srow = scores + (int64_t)r * ld;
    int cnt = 0;
    for (int j0 = 0; j0 < n; j0 += 64 * TK_UNROLL) {
        float v[TK_UNROLL];
#pragma unroll
        for (int u = 0; u < TK_UNROLL; ++u) {
            const int j = j0 + u * 64 + lane;
            v[u] = j < n ? srow[j] : __builtin_nanf("");
        }
#pragma unroll
        for (int u = 0; u < TK_UNROLL; ++u) {
            const int j = j0 + u * 64 + lane;
            float s = v[u];
            if (col_norm && j < n) s = s / (qs * fmaxf(col_norm[j], 1e-8f));
            const uint64_t key = topk_key(s, col0 + j);
            bool keep = (s == s) && (col0 + j != skip) && key > thr;
            uint64_t m = __ballot(keep);
            if (m == 0) continue;
            if (cnt + __popcll(m) > KP) {            // buffer full: merge first (the threshold rises), then re-test
                topk_merge_lds<KP>(top, buf, lane);
                thr = top[k - 1];
                cnt = 0;
                keep = keep && key > thr;
                m = __ballot(keep);
            }
            const int pos = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            if (keep) buf[cnt + pos] = key;
            cnt += __popcll(m);
            wave_lds_sync();
        }
    }
    if (cnt > 0) topk_merge_lds<KP>(top, buf, lane);
    for (int i = lane; i < k; i += 64) st[i] = top[i];
}

// keys -> (dataset row id, score); an empty key -> (-1, -inf).  Row b's candidate table: cand_row_id + slot[b] * n_cand
// (slot == null: one table; a slot outside [0, n_slots) has an empty state: its whole row is the -1 / -inf tail)
__global__ __launch_bounds__(NT) void topk_finish_kernel(const uint64_t* __restrict__ state, int B, int k,
                                                         const int32_t* __restrict__ cand_row_id, const int32_t* __restrict__ slot,
                                                         int n_slots, int n_cand, int32_t* __restrict__ out_idx,
                                                         float* __restrict__ out_score) {
    const int64_t total = (int64_t)B * k;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < total; e += (int64_t)gridDim.x * NT) {
        const uint64_t key = state[e];
        int32_t id = -1;
        float sc = -__builtin_inff();
        if (key != 0) {
            const int pos = (int)~(uint32_t)key;
            sc = topk_key_score(key);
            id = pos;
            if (cand_row_id) {
                const int c = slot ? slot[e / k] : 0;
                id = (c >= 0 && c < n_slots) ? cand_row_id[(int64_t)c * n_cand + pos] : -1;
            }
        }
        out_idx[e] = id;
        out_score[e] = sc;
    }
}

// one wave per query: slot c (given, or the blanked slot of its mask as rank_prep_kernel finds it), |q| clamped, the
// candidate to skip (exclude[b] mapped through cand_pos[c]), and the compaction of the slot's rows (perm / counts).
// Row state: slot_out [B] (-1: slot outside [0, S), no candidates), qn_out [B], skip_out [B].
__global__ __launch_bounds__(NT) void complete_prep_kernel(const float* __restrict__ pred, int B, int io, int S, int E,
                                                           const int32_t* __restrict__ slot, const int32_t* __restrict__ row_idx,
                                                           const int32_t* __restrict__ mask_id, const int32_t* __restrict__ mask_to_use,
                                                           int nb_run, int run, const uint8_t* __restrict__ mask_table,
                                                           const int32_t* __restrict__ exclude, const int32_t* __restrict__ cand_pos,
                                                           int64_t n_obs, int32_t* __restrict__ slot_out, float* __restrict__ qn_out,
                                                           int32_t* __restrict__ skip_out, int32_t* __restrict__ perm,
                                                           int32_t* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (b >= B) return;
    int c;
    if (slot) {
        c = slot[b];
    } else {
        const int id = mask_id ? mask_id[b] : mask_to_use[(int64_t)row_idx[b] * nb_run + run];
        c = 0;
        for (int s = 1; s < S; ++s) c += (mask_table[(int64_t)id * io + (int64_t)s * E] == 0) ? s : 0;
        c = c < S ? c : S - 1;
    }
    if (c < 0 || c >= S) {
        if (lane == 0) { slot_out[b] = -1; qn_out[b] = 1.f; skip_out[b] = -1; }
        return;
    }
    const float* q = pred + (int64_t)b * io + (int64_t)c * E;
    float sq = 0.f;
    for (int x = lane; x < E; x += 64) { const float v = q[x]; sq += v * v; }
    sq = wave_sum_f(sq);
    if (lane == 0) {
        int skip = -1;
        if (exclude && cand_pos) {
            const int64_t ex = exclude[b];
            skip = (ex >= 0 && ex < n_obs) ? cand_pos[(int64_t)c * n_obs + ex] : -1;
        }
        slot_out[b] = c;
        qn_out[b] = fmaxf(sqrtf(sq), 1e-8f);
        skip_out[b] = skip;
        const int k = atomicAdd(&counts[c], 1);      // (integer: which GEMM row a query lands on changes none of its bits)
        perm[(int64_t)c * B + k] = b;
    }
}

template <int KP>
int launch_topk_merge(const float* scores, int64_t ld, int rows, const int32_t* rows_dev, int n, int col0, int k,
                      const int32_t* row_map, const float* row_norm, const float* col_norm, const int32_t* skip_col,
                      uint64_t* state, hipStream_t s) {
    hipLaunchKernelGGL(topk_merge_kernel<KP>, dim3((rows + TK_WAVES - 1) / TK_WAVES), dim3(NT), 0, s, scores, ld, rows, rows_dev,
                       n, col0, k, row_map, row_norm, col_norm, skip_col, state);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

// LDS capacity per wave: the k best plus a buffer of as many survivors, in powers of two from one wave's width
int topk_merge(const float* scores, int64_t ld, int rows, const int32_t* rows_dev, int n, int col0, int k, const int32_t* row_map,
               const float* row_norm, const float* col_norm, const int32_t* skip_col, uint64_t* state, hipStream_t s) {
    if (k <= 64) return launch_topk_merge<64>(scores, ld, rows, rows_dev, n, col0, k, row_map, row_norm, col_norm, skip_col, state, s);
    if (k <= 128) return launch_topk_merge<128>(scores, ld, rows, rows_dev, n, col0, k, row_map, row_norm, col_norm, skip_col, state, s);
    return launch_topk_merge<256>(scores, ld, rows, rows_dev, n, col0, k, row_map, row_norm, col_norm, skip_col, state, s);
}

constexpr int TOPK_KMAX = 256;

// ---- validation retrieval metrics: hit@k, MRR, rank error and a position histogram per slot ------------------------------
// (include/codae_hip.h, "Retrieval metrics".)  A query pair (b, c) is a batch row b and a slot c that its mask blanks and its
// dataset row has.  Its competitors are the items of slot c's candidate table (duplicates already folded into one item) except
// the item the row itself belongs to; position = 1 + competitors - beaten.  State [S][B], indexed by the BATCH row so that the
// finish pass adds the pairs of a slot in a fixed order whatever order the compaction handed the rows to the GEMM in.
struct MetricPair { float qn; float own; int self_col; int beaten; };      // self_col: candidate position of the own item, -1 none, -2 no pair
constexpr int RM_NO_PAIR = -2;
constexpr int RM_PREP_ROWS = 16;         // batch rows per workgroup of the prepare pass (four per wave): one counter update per slot
constexpr int RM_MAX_SLOTS = 128;
constexpr int RM_VEC = 4;                // 16-byte loads in flight per lane of the count pass
constexpr int RM_SEG = 64 * 4 * RM_VEC * 2;      // score columns per wave: two sweeps of 64 lanes x RM_VEC x 4 columns
struct MetricKs { int n; int k[CODAE_RM_MAX_KS]; };

// one wave per batch row: which slots are query pairs (mask table and presence byte, lanes over slots), then |q| and the own
// similarity of each of them (lanes over E).  The workgroup's rows take their places in every slot's compacted list with ONE
// atomic per slot and workgroup (flags in LDS, counted by one thread per slot).
__global__ __launch_bounds__(NT) void metrics_prep_kernel(const float* __restrict__ pred, const int32_t* __restrict__ row_idx,
                                                          const int32_t* __restrict__ mask_id, const int32_t* __restrict__ mask_to_use,
                                                          int nb_run, int run, const uint8_t* __restrict__ mask_table,
                                                          const uint8_t* __restrict__ presence, int B, int io, int S, int E,
                                                          const float* __restrict__ inv, const float* __restrict__ inv_norm, int64_t n_obs,
                                                          const int32_t* __restrict__ cand_pos, MetricPair* __restrict__ state,
                                                          int32_t* __restrict__ perm, int32_t* __restrict__ counts) {
    __shared__ uint8_t flag[RM_PREP_ROWS][RM_MAX_SLOTS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int row0 = blockIdx.x * RM_PREP_ROWS;
    for (int i = w; i < RM_PREP_ROWS; i += NT / 64) {
        const int b = row0 + i;
        const int64_t me = b < B ? row_idx[b] : -1;
        const bool row_ok = me >= 0 && me < n_obs;                       // (wave-uniform)
        const int id = !row_ok ? 0 : (mask_id ? mask_id[b] : mask_to_use[me * nb_run + run]);
        for (int c0 = 0; c0 < S; c0 += 64) {
            const int c = c0 + lane;
            bool q = false;
            if (row_ok && c < S)
                q = mask_table[(int64_t)id * io + (int64_t)c * E] == 0 && (presence == nullptr || presence[me * S + c] != 0);
            if (c < S) {
                flag[i][c] = q ? 1 : 0;
                if (b < B && !q) { MetricPair o; o.qn = 1.f; o.own = 0.f; o.self_col = RM_NO_PAIR; o.beaten = 0; state[(int64_t)c * B + b] = o; }
            }
            uint64_t m = __ballot(q);
            while (m != 0) {                                             // (wave-uniform: at most nb_missing turns)
                const int cc = c0 + __builtin_ctzll(m);
                m &= m - 1;
                const float* qv = pred + (int64_t)b * io + (int64_t)cc * E;
                const float* r = inv + ((int64_t)cc * n_obs + me) * E;
                float sq = 0.f, d = 0.f;
                for (int x = lane; x < E; x += 64) { const float v = qv[x]; sq += v * v; d += v * r[x]; }
                sq = wave_sum_f(sq); d = wave_sum_f(d);
                if (lane == 0) {
                    MetricPair o;
                    o.qn = fmaxf(sqrtf(sq), 1e-8f);
                    o.own = d / (o.qn * fmaxf(inv_norm[(int64_t)cc * n_obs + me], 1e-8f));
                    o.self_col = cand_pos[(int64_t)cc * n_obs + me];     // (-1: the row is no candidate of this slot)
                    o.beaten = 0;
                    state[(int64_t)cc * B + b] = o;
                }
            }
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < S; c += NT) {
        int cnt = 0;
        for (int i = 0; i < RM_PREP_ROWS; ++i) cnt += flag[i][c];
        if (cnt == 0) continue;
        int k = atomicAdd(&counts[c], cnt);          // (integer: which GEMM row a pair lands on changes none of its bits)
        for (int i = 0; i < RM_PREP_ROWS; ++i)
            if (flag[i][c]) perm[(int64_t)c * B + k++] = row0 + i;
    }
}

// The compare-and-count pass over one chunk of slot c's score block: wave (k, segment) takes RM_SEG columns of compact row
// k < counts[c].  Every score is read once, as 16-byte loads, RM_VEC of them issued before the first compare; one comparison
// and one skip-by-position test per element (s = dot / (|q| max(|v|, 1e-8)), as rank_count_kernel; a NaN on either side
// counts nothing); the n % 4 ragged columns go through scalar code; a wave reduction, then one integer add per wave.
__device__ __forceinline__ int metrics_beats(float own, float qn, float dot, float nrm, int j, int skip) {
    return (int)(j != skip) & (int)(own > dot / (qn * fmaxf(nrm, 1e-8f)));       // (no short circuit: no branch per element)
}
__global__ __launch_bounds__(NT) void metrics_count_kernel(const float* __restrict__ dots, int64_t ld, int B, int n, int c, int v0,
                                                           const float* __restrict__ col_norm, MetricPair* __restrict__ state,
                                                           const int32_t* __restrict__ perm, const int32_t* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (k >= counts[c]) return;
    MetricPair* st = state + (int64_t)c * B + perm[(int64_t)c * B + k];
    const float own = st->own, qn = st->qn;
    const int skip = st->self_col - v0;
    const float* d = dots + (int64_t)k * ld;
    const int j0 = blockIdx.y * RM_SEG;
    const int j1 = min(j0 + RM_SEG, n);
    const int jv = min(j1, n & ~3);                  // (a multiple of 4: whole 16-byte groups below it)
    int cnt = 0;
    int jw = j0;                                     // (wave-uniform)
    for (; jw + 64 * 4 * RM_VEC <= jv; jw += 64 * 4 * RM_VEC) {      // whole sweeps: every load in range, all issued before the first compare
        float4 v[RM_VEC], nr[RM_VEC];
#pragma unroll
        for (int u = 0; u < RM_VEC; ++u) {
            const int jj = jw + u * 256 + 4 * lane;
            v[u] = *reinterpret_cast<const float4*>(d + jj);
            nr[u] = *reinterpret_cast<const float4*>(col_norm + jj);
        }
#pragma unroll
        for (int u = 0; u < RM_VEC; ++u) {
            const int jj = jw + u * 256 + 4 * lane;
            cnt += metrics_beats(own, qn, v[u].x, nr[u].x, jj, skip) + metrics_beats(own, qn, v[u].y, nr[u].y, jj + 1, skip) +
                   metrics_beats(own, qn, v[u].z, nr[u].z, jj + 2, skip) + metrics_beats(own, qn, v[u].w, nr[u].w, jj + 3, skip);
        }
    }
    for (int jj = jw + 4 * lane; jj < jv; jj += 256) {               // the rest of the segment, one 16-byte group per lane and turn
        const float4 v = *reinterpret_cast<const float4*>(d + jj);
        const float4 nr = *reinterpret_cast<const float4*>(col_norm + jj);
        cnt += metrics_beats(own, qn, v.x, nr.x, jj, skip) + metrics_beats(own, qn, v.y, nr.y, jj + 1, skip) +
               metrics_beats(own, qn, v.z, nr.z, jj + 2, skip) + metrics_beats(own, qn, v.w, nr.w, jj + 3, skip);
    }
    if (j1 == n) {                                   // the last segment also takes the n % 4 ragged columns, one per lane
        const int j = (n & ~3) + lane;
        if (j < n) cnt += metrics_beats(own, qn, d[j], col_norm[j], j, skip);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0 && cnt != 0) atomicAdd(&st->beaten, cnt);
}

// One workgroup for one slot: position, rank error and reciprocal rank of every pair of the slot, added into the slot's block.
// Counts are integers (LDS atomics: exact in any order); the two fp64 sums are per-thread partials over rows t, t + NT, ...
// folded by a tree - a fixed order, the same bits every run.  nc: the slot's item count.
__global__ __launch_bounds__(NT) void metrics_finish_kernel(const MetricPair* __restrict__ st, int B, int nc, MetricKs ks,
                                                            double* __restrict__ acc) {
    __shared__ double red[2][NT];
    __shared__ unsigned int cnt[CODAE_RM_STRIDE];
    const int t = threadIdx.x;
    if (t < CODAE_RM_STRIDE) cnt[t] = 0;
    __syncthreads();
    double rre = 0.0, rr = 0.0;
    for (int b = t; b < B; b += NT) {
        const MetricPair p = st[b];
        if (p.self_col == RM_NO_PAIR) continue;
        const int n = nc - (p.self_col >= 0 ? 1 : 0);
        if (n < 1) continue;                         // (no competitor: not a query pair)
        const int beaten = p.beaten < 0 ? 0 : (p.beaten > n ? n : p.beaten);
        const int pos = 1 + n - beaten;
        rre += (double)(pos - 1) / (double)n;
        rr += 1.0 / (double)pos;
        atomicAdd(&cnt[CODAE_RM_PAIRS], 1u);
        for (int i = 0; i < ks.n; ++i)
            if (pos <= ks.k[i]) atomicAdd(&cnt[CODAE_RM_HIT + i], 1u);
        atomicAdd(&cnt[CODAE_RM_HIST + 31 - __builtin_clz((unsigned)pos)], 1u);
    }
    red[0][t] = rre; red[1][t] = rr;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if (t < o) { red[0][t] += red[0][t + o]; red[1][t] += red[1][t + o]; }
        __syncthreads();
    }
    if (t < CODAE_RM_STRIDE) {
        double add = (double)cnt[t];
        if (t == CODAE_RM_RRE) add = red[0][0];
        if (t == CODAE_RM_RR) add = red[1][0];
        acc[t] += add;
    }
}

}  // namespace
}  // namespace codae

using namespace codae;

extern "C" {

int codae_combined_loss_fwd_bwd(const float* x, const float* y, int32_t B, int32_t io, int32_t n_var, const int32_t* var_pos,
                                const int32_t* var_size, const int32_t* var_type, const float* var_weight, double* acc,
                                float* dy, double* loss_out, void* stream) {
    CODAE_REQUIRE(x && y && var_pos && var_size && var_type && var_weight && acc && loss_out, "combined_loss: null argument");
    CODAE_REQUIRE(B > 0 && io > 0 && n_var > 0, "combined_loss: empty problem");
    hipStream_t s = (hipStream_t)stream;
    CODAE_HIP_CHECK(hipMemsetAsync(acc, 0, (size_t)n_var * sizeof(double), s));
    const int grid = grid_for((int64_t)B * n_var);
    hipLaunchKernelGGL(combined_reduce_kernel, dim3(grid), dim3(NT), 0, s, x, y, B, io, n_var, var_pos, var_size, var_type, acc);
    CODAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(combined_grad_kernel, dim3(grid), dim3(NT), 0, s, x, y, B, io, n_var, var_pos, var_size, var_type,
                       var_weight, acc, dy, loss_out);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int codae_combined_loss_full(const float* x, const float* y, int32_t B, int32_t io, int32_t n_var, const int32_t* var_pos,
                             const int32_t* var_size, const int32_t* var_type, float* out, void* stream) {
    CODAE_REQUIRE(x && y && var_pos && var_size && var_type && out && B > 0 && io > 0 && n_var > 0, "combined_full: bad argument");
    hipLaunchKernelGGL(combined_full_kernel, dim3(grid_for((int64_t)B * n_var)), dim3(NT), 0, (hipStream_t)stream, x, y, B, io,
                       n_var, var_pos, var_size, var_type, out);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int codae_monitor_accumulate(const float* x, const float* y, int32_t B, int32_t io, int32_t n_var, const int32_t* var_pos,
                             const int32_t* var_size, const int32_t* var_type, const float* undo_scale, const float* undo_min,
                             const int32_t* mask_id, const uint8_t* mask_table, const int32_t* k_of_mask, int32_t k_max,
                             double* acc, void* stream) {
    CODAE_REQUIRE(x && y && var_pos && var_size && var_type && mask_id && mask_table && k_of_mask && acc, "monitor_accumulate: null argument");
    CODAE_REQUIRE(B > 0 && io > 0 && n_var > 0 && n_var <= NT, "monitor_accumulate: bad sizes (B %d, io %d, n_var %d)", B, io, n_var);
    CODAE_REQUIRE(k_max >= 1 && k_max <= MON_KMAX, "monitor_accumulate: k_max %d outside [1, %d]", k_max, MON_KMAX);
    CODAE_REQUIRE((undo_scale == nullptr) == (undo_min == nullptr), "monitor_accumulate: undo_scale and undo_min come together");
    hipLaunchKernelGGL(monitor_accumulate_kernel, dim3(1), dim3(NT), (size_t)NT * 2 * k_max * sizeof(double), (hipStream_t)stream, x, y, B,
                       io, n_var, var_pos, var_size, var_type, undo_scale, undo_min, mask_id, mask_table, k_of_mask, k_max, acc);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int codae_row_norms(const float* m, int64_t rows, int32_t E, float* out, void* stream) {
    CODAE_REQUIRE(m && out && rows > 0 && E > 0, "row_norms: bad argument");
    int64_t g = (rows + 3) / 4;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(row_norm_kernel, dim3((unsigned)g), dim3(NT), 0, (hipStream_t)stream, m, rows, E, out);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int codae_ranking_loss(const float* pred, const float* fmask, const int32_t* idx, int32_t B, int32_t io, int32_t n_slots,
                       int32_t E, const float* inventory, const float* inventory_norm, int64_t n_obs, const int32_t* val_idx,
                       int32_t n_val, double* out, void* stream) {
    CODAE_REQUIRE(pred && fmask && idx && inventory && inventory_norm && val_idx && out, "ranking_loss: null argument");
    CODAE_REQUIRE(B > 0 && n_slots > 0 && E > 0 && io == n_slots * E && n_val > 1 && n_obs > 0, "ranking_loss: bad sizes");
    CODAE_REQUIRE((size_t)E * sizeof(float) <= 64 * 1024, "ranking_loss: embedding size %d too large for LDS staging", E);
    hipLaunchKernelGGL(ranking_kernel, dim3(B), dim3(NT), (size_t)E * sizeof(float), (hipStream_t)stream, pred, fmask, idx, io,
                       n_slots, E, inventory, inventory_norm, n_obs, val_idx, n_val, out);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int codae_gather_inventory_rows(const float* inventory, int64_t n_obs, int32_t E, int32_t n_slots, const int32_t* val_idx,
                                int32_t n_val, float* dst, void* stream) {
    CODAE_REQUIRE(inventory && val_idx && dst && n_obs > 0 && E > 0 && n_slots > 0 && n_val > 0, "gather_inventory_rows: bad argument");
    hipLaunchKernelGGL(gather_rows_kernel, dim3(grid_for((int64_t)n_slots * n_val * E)), dim3(NT), 0, (hipStream_t)stream, inventory,
                       n_obs, E, n_slots, val_idx, n_val, dst);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int codae_ranking_loss_batched(const float* pred, int32_t B, int32_t io, int32_t n_slots, int32_t E, const int32_t* row_idx,
                               const int32_t* mask_id, const int32_t* mask_to_use, int32_t nb_run, int32_t run,
                               const uint8_t* mask_table, const float* inventory, const float* inventory_norm, int64_t n_obs,
                               const float* inv_val, const float* inv_val_norm, const int32_t* val_pos, const int32_t* val_group,
                               int32_t n_val, float* work, int32_t chunk, void* row_state, int32_t* perm_ws, float* q_ws, double* out,
                               void* stream) {
    CODAE_REQUIRE(pred && row_idx && (mask_id || mask_to_use) && mask_table && inventory && inventory_norm && inv_val && inv_val_norm &&
                      work && row_state && perm_ws && q_ws && out, "ranking_loss_batched: null argument");
    CODAE_REQUIRE(B > 0 && n_slots > 0 && E > 0 && io == n_slots * E && n_val > 1 && n_obs > 0 && chunk > 0, "ranking_loss_batched: bad sizes");
    CODAE_REQUIRE(mask_id || (nb_run > 0 && run >= 0 && run < nb_run), "ranking_loss_batched: run %d outside [0, %d)", run, nb_run);
    hipStream_t s = (hipStream_t)stream;
    RankRow* rs = reinterpret_cast<RankRow*>(row_state);
    int32_t* perm = perm_ws;                               // [n_slots][B]
    int32_t* counts = perm_ws + (int64_t)n_slots * B;      // [n_slots]
    CODAE_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)n_slots * sizeof(int32_t), s));
    const int rows_grid = (B + NT / 64 - 1) / (NT / 64);
    hipLaunchKernelGGL(rank_prep_kernel, dim3(rows_grid), dim3(NT), 0, s, pred, row_idx, mask_id, mask_to_use, nb_run, run, mask_table, B,
                       io, n_slots, E, inventory, inventory_norm, n_obs, val_pos, val_group, n_val, rs, perm, counts);
    CODAE_LAUNCH_CHECK();
    // per slot: its rows' queries gathered, then one GEMM per chunk of validation rows over THOSE rows only (the row count
    // stays on the device: the grid covers B rows, tiles past counts[c] return at once), then the compare-count pass
    for (int c = 0; c < n_slots; ++c) {
        hipLaunchKernelGGL(rank_gather_q_kernel, dim3(grid_for((int64_t)B * E / 4)), dim3(NT), 0, s, pred, io, E, B, c, perm, counts, q_ws);
        CODAE_LAUNCH_CHECK();
        for (int v0 = 0; v0 < n_val; v0 += chunk) {
            const int n = n_val - v0 < chunk ? n_val - v0 : chunk;
            GemmF32 g{};
            g.A = q_ws; g.a_rs = E; g.a_ks = 1;
            g.B = inv_val + ((int64_t)c * n_val + v0) * E; g.b_rs = E; g.b_ks = 1;
            g.C = work; g.ldc = chunk;
            g.M = B; g.N = n; g.K = E;
            g.m_dev = counts + c;
            int rc = gemm_f32(g, s);
            if (rc) return rc;
            hipLaunchKernelGGL(rank_count_kernel, dim3(rows_grid), dim3(NT), 0, s, work, (int64_t)chunk, B, n, c, v0,
                               inv_val_norm + (int64_t)c * n_val + v0, val_group ? val_group + (int64_t)c * n_val + v0 : nullptr, rs, perm,
                               counts);
            CODAE_LAUNCH_CHECK();
        }
    }
    hipLaunchKernelGGL(rank_finish_kernel, dim3(1), dim3(NT), 0, s, rs, B, n_val, out);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int codae_topk_init(void* state, int32_t B, int32_t k, void* stream) {
    CODAE_REQUIRE(state && B > 0 && k >= 1 && k <= TOPK_KMAX, "topk_init: bad argument (B %d, k %d)", B, k);
    CODAE_HIP_CHECK(hipMemsetAsync(state, 0, (size_t)B * k * sizeof(uint64_t), (hipStream_t)stream));
    return CODAE_OK;
}

int codae_topk_merge(const float* scores, int64_t ld, int32_t rows, int32_t n, int32_t col0, int32_t k, const int32_t* row_map,
                     const int32_t* skip_col, void* state, void* stream) {
    CODAE_REQUIRE(scores && state, "topk_merge: null argument");
    CODAE_REQUIRE(rows > 0 && n > 0 && ld >= n && col0 >= 0 && (int64_t)col0 + n <= INT32_MAX, "topk_merge: bad sizes");
    CODAE_REQUIRE(k >= 1 && k <= TOPK_KMAX, "topk_merge: k %d outside [1, %d]", k, TOPK_KMAX);
    return topk_merge(scores, ld, rows, nullptr, n, col0, k, row_map, nullptr, nullptr, skip_col, (uint64_t*)state,
                      (hipStream_t)stream);
}

int codae_topk_finish(const void* state, int32_t B, int32_t k, const int32_t* cand_row_id, int32_t* out_idx, float* out_score,
                      void* stream) {
    CODAE_REQUIRE(state && out_idx && out_score, "topk_finish: null argument");
    CODAE_REQUIRE(B > 0 && k >= 1 && k <= TOPK_KMAX, "topk_finish: bad sizes (B %d, k %d)", B, k);
    hipLaunchKernelGGL(topk_finish_kernel, dim3(grid_for((int64_t)B * k)), dim3(NT), 0, (hipStream_t)stream, (const uint64_t*)state, B,
                       k, cand_row_id, nullptr, 1, 0, out_idx, out_score);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int codae_complete_topk(const float* pred, int32_t B, int32_t io, int32_t n_slots, int32_t E, const int32_t* slot,
                        const int32_t* row_idx, const int32_t* mask_id, const int32_t* mask_to_use, int32_t nb_run, int32_t run,
                        const uint8_t* mask_table, const float* cand, const float* cand_norm, const int32_t* cand_row_id,
                        int32_t n_cand, const int32_t* cand_count, const int32_t* exclude, const int32_t* cand_pos, int64_t n_obs,
                        int32_t k, float* work, int32_t chunk, void* row_state, int32_t* perm_ws, float* q_ws, void* topk_state,
                        int32_t* out_idx, float* out_score, void* stream) {
    CODAE_REQUIRE(pred && cand && cand_norm && cand_row_id && work && row_state && perm_ws && q_ws && topk_state && out_idx && out_score,
                  "complete_topk: null argument");
    CODAE_REQUIRE(slot || (mask_table && (mask_id || (mask_to_use && row_idx))), "complete_topk: neither a slot array nor a mask route");
    CODAE_REQUIRE(slot || mask_id || (nb_run > 0 && run >= 0 && run < nb_run), "complete_topk: run %d outside [0, %d)", run, nb_run);
    CODAE_REQUIRE(B > 0 && n_slots > 0 && E > 0 && io == n_slots * E && n_cand > 0 && chunk > 0, "complete_topk: bad sizes");
    CODAE_REQUIRE(k >= 1 && k <= TOPK_KMAX, "complete_topk: k %d outside [1, %d]", k, TOPK_KMAX);
    CODAE_REQUIRE(!exclude || (cand_pos && n_obs > 0), "complete_topk: exclude needs cand_pos and n_obs");
    if (cand_count)
        for (int c = 0; c < n_slots; ++c)
            CODAE_REQUIRE(cand_count[c] >= 0 && cand_count[c] <= n_cand, "complete_topk: cand_count[%d] = %d outside [0, %d]", c,
                          cand_count[c], n_cand);
    hipStream_t s = (hipStream_t)stream;
    int32_t* slot_rs = reinterpret_cast<int32_t*>(row_state);          // [B] slot (-1: none)
    float* qn_rs = reinterpret_cast<float*>(slot_rs + B);             // [B] |q| clamped
    int32_t* skip_rs = slot_rs + 2 * (int64_t)B;                      // [B] candidate position to skip (-1: none)
    int32_t* perm = perm_ws;                                          // [n_slots][B]
    int32_t* counts = perm_ws + (int64_t)n_slots * B;                 // [n_slots]
    uint64_t* st = reinterpret_cast<uint64_t*>(topk_state);
    CODAE_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)n_slots * sizeof(int32_t), s));
    CODAE_HIP_CHECK(hipMemsetAsync(st, 0, (size_t)B * k * sizeof(uint64_t), s));
    const int rows_grid = (B + NT / 64 - 1) / (NT / 64);
    hipLaunchKernelGGL(complete_prep_kernel, dim3(rows_grid), dim3(NT), 0, s, pred, B, io, n_slots, E, slot, row_idx, mask_id, mask_to_use,
                       nb_run, run, mask_table, exclude, cand_pos, n_obs, slot_rs, qn_rs, skip_rs, perm, counts);
    CODAE_LAUNCH_CHECK();
    // per slot: its queries gathered (compacted: the row count stays on the device), one fp32 GEMM per chunk of candidates over
    // those rows (gemm_f32: the x3 / native switch of the parity path), then the selection pass over the chunk it wrote
    for (int c = 0; c < n_slots; ++c) {
        const int nc = cand_count ? cand_count[c] : n_cand;
        if (nc == 0) continue;
        hipLaunchKernelGGL(rank_gather_q_kernel, dim3(grid_for((int64_t)B * E / 4)), dim3(NT), 0, s, pred, io, E, B, c, perm, counts, q_ws);
        CODAE_LAUNCH_CHECK();
        for (int v0 = 0; v0 < nc; v0 += chunk) {
            const int n = nc - v0 < chunk ? nc - v0 : chunk;
            GemmF32 g{};
            g.A = q_ws; g.a_rs = E; g.a_ks = 1;
            g.B = cand + ((int64_t)c * n_cand + v0) * E; g.b_rs = E; g.b_ks = 1;
            g.C = work; g.ldc = chunk;
            g.M = B; g.N = n; g.K = E;
            g.m_dev = counts + c;
            int rc = gemm_f32(g, s);
            if (rc) return rc;
            rc = topk_merge(work, chunk, B, counts + c, n, v0, k, perm + (int64_t)c * B, qn_rs, cand_norm + (int64_t)c * n_cand + v0,
                            skip_rs, st, s);
            if (rc) return rc;
        }
    }
    hipLaunchKernelGGL(topk_finish_kernel, dim3(grid_for((int64_t)B * k)), dim3(NT), 0, s, st, B, k, cand_row_id, slot_rs, n_slots, n_cand,
                       out_idx, out_score);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int codae_retrieval_metrics_batched(const float* pred, int32_t B, int32_t io, int32_t n_slots, int32_t E, const int32_t* row_idx,
                                    const int32_t* mask_id, const int32_t* mask_to_use, int32_t nb_run, int32_t run,
                                    const uint8_t* mask_table, const uint8_t* presence, const float* inventory,
                                    const float* inventory_norm, int64_t n_obs, const float* cand, const float* cand_norm,
                                    int32_t n_cand, const int32_t* cand_count, const int32_t* cand_pos, const int32_t* ks, int32_t n_ks,
                                    float* work, int32_t chunk, void* pair_state, int32_t* perm_ws, float* q_ws, double* acc,
                                    void* stream) {
    CODAE_REQUIRE(pred && row_idx && (mask_id || mask_to_use) && mask_table && inventory && inventory_norm && cand && cand_norm &&
                      cand_count && cand_pos && work && pair_state && perm_ws && q_ws && acc, "retrieval_metrics: null argument");
    CODAE_REQUIRE(B > 0 && n_slots > 0 && n_slots <= RM_MAX_SLOTS && E > 0 && io == n_slots * E && n_obs > 0 && n_cand > 0,
                  "retrieval_metrics: bad sizes (B %d, slots %d, E %d, io %d)", B, n_slots, E, io);
    CODAE_REQUIRE(mask_id || (nb_run > 0 && run >= 0 && run < nb_run), "retrieval_metrics: run %d outside [0, %d)", run, nb_run);
    // 16-byte loads of the score rows and of the norms: whole groups of four columns from aligned bases
    CODAE_REQUIRE(chunk > 0 && chunk % 4 == 0 && n_cand % 4 == 0, "retrieval_metrics: chunk %d and n_cand %d must be multiples of 4", chunk, n_cand);
    CODAE_REQUIRE((reinterpret_cast<uintptr_t>(work) & 15) == 0 && (reinterpret_cast<uintptr_t>(cand_norm) & 15) == 0,
                  "retrieval_metrics: work and cand_norm must be 16-byte aligned");
    CODAE_REQUIRE(n_ks >= 0 && n_ks <= CODAE_RM_MAX_KS && (n_ks == 0 || ks), "retrieval_metrics: %d thresholds (at most %d)", n_ks, CODAE_RM_MAX_KS);
    MetricKs mk{};
    mk.n = n_ks;
    for (int i = 0; i < n_ks; ++i) {
        CODAE_REQUIRE(ks[i] >= 1 && (i == 0 || ks[i] > ks[i - 1]), "retrieval_metrics: thresholds must be ascending positive ints (ks[%d] = %d)", i, ks[i]);
        mk.k[i] = ks[i];
    }
    for (int c = 0; c < n_slots; ++c)
        CODAE_REQUIRE(cand_count[c] >= 0 && cand_count[c] <= n_cand, "retrieval_metrics: cand_count[%d] = %d outside [0, %d]", c, cand_count[c], n_cand);
    hipStream_t s = (hipStream_t)stream;
    MetricPair* st = reinterpret_cast<MetricPair*>(pair_state);        // [n_slots][B]
    int32_t* perm = perm_ws;                                           // [n_slots][B]
    int32_t* counts = perm_ws + (int64_t)n_slots * B;                  // [n_slots]
    CODAE_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)n_slots * sizeof(int32_t), s));
    hipLaunchKernelGGL(metrics_prep_kernel, dim3((B + RM_PREP_ROWS - 1) / RM_PREP_ROWS), dim3(NT), 0, s, pred, row_idx, mask_id, mask_to_use,
                       nb_run, run, mask_table, presence, B, io, n_slots, E, inventory, inventory_norm, n_obs, cand_pos, st, perm, counts);
    CODAE_LAUNCH_CHECK();
    // per slot: its pairs' queries gathered, one fp32 GEMM per chunk of items over those rows only (gemm_f32 with the row count on
    // the device, exactly as codae_complete_topk), the count pass over the chunk it wrote, then the slot's finish
    const int rows_grid = (B + NT / 64 - 1) / (NT / 64);
    for (int c = 0; c < n_slots; ++c) {
        const int nc = cand_count[c];
        if (nc == 0) continue;                        // (no item: no competitor, no pair)
        hipLaunchKernelGGL(rank_gather_q_kernel, dim3(grid_for((int64_t)B * E / 4)), dim3(NT), 0, s, pred, io, E, B, c, perm, counts, q_ws);
        CODAE_LAUNCH_CHECK();
        for (int v0 = 0; v0 < nc; v0 += chunk) {
            const int n = nc - v0 < chunk ? nc - v0 : chunk;
            GemmF32 g{};
            g.A = q_ws; g.a_rs = E; g.a_ks = 1;
            g.B = cand + ((int64_t)c * n_cand + v0) * E; g.b_rs = E; g.b_ks = 1;
            g.C = work; g.ldc = chunk;
            g.M = B; g.N = n; g.K = E;
            g.m_dev = counts + c;
            int rc = gemm_f32(g, s);
            if (rc) return rc;
            hipLaunchKernelGGL(metrics_count_kernel, dim3(rows_grid, (n + RM_SEG - 1) / RM_SEG), dim3(NT), 0, s, work, (int64_t)chunk, B, n, c,
                               v0, cand_norm + (int64_t)c * n_cand + v0, st, perm, counts);
            CODAE_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(metrics_finish_kernel, dim3(1), dim3(NT), 0, s, st + (int64_t)c * B, B, nc, mk, acc + (int64_t)c * CODAE_RM_STRIDE);
        CODAE_LAUNCH_CHECK();
    }
    return CODAE_OK;
}

}  // extern "C"
