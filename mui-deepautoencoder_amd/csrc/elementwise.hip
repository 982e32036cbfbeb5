// HBM-bound pieces of the DAE step: the stand-alone MSE losses (forward/backward with the reference's per-step metrics) and their
// finishes, the split-K slab reductions, the bias-gradient column sums and their finish, the bf16 transposes.  (The gather is
// gather.hip's, the parameter update optimizer.hip's.)
#include "loss_sweep.h"

namespace codae {
namespace {

constexpr int NT = GRID_NT;
static_assert(NT == LOSS_NT, "loss_sweep strides the columns by LOSS_NT threads");

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
template <bool VEC, bool DY_BF16, bool PRES, bool SWAP = false>
__global__ __launch_bounds__(NT) void emph_loss_kernel(const float* __restrict__ data, const int32_t* __restrict__ row_idx,
                                                       const int32_t* __restrict__ mask_id, const uint8_t* __restrict__ table,
                                                       int B, int io, const float* __restrict__ y, void* __restrict__ dy,
                                                       float inv_n, float* __restrict__ colsum_part, double* __restrict__ parts,
                                                       const int32_t* __restrict__ mask_to_use, int nb_run, int run, int64_t dy_ld,
                                                       WeightArgsOf<SWAP> wa, PresArgs pa) {
    __shared__ float red[4];
    const bool masked = (mask_id != nullptr) || (mask_to_use != nullptr);
    const BatchArgs ba{data, row_idx, mask_id, table, mask_to_use, nb_run, run, B, io};
    EmphTerm term(wa, inv_n);
    loss_sweep<VEC, DY_BF16, PRES, SWAP>(ba, y, dy, dy_ld, colsum_part, pa, wa, term);
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
    if (ll.noise != nullptr && ll.noise->kind == CODAE_NOISE_SWAP) {
        rc = check_swap(ll.swap, b->io, ll.present, ll.n_slots, who);
        if (rc) return rc;
    }
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
    const SwapWeightArgs wa = weight_args(ll, true);
    const bool vec = (b->io % 4 == 0) && (dy_ld % 4 == 0) && loss_inputs_a16(ll) && a16(ll.dy) && (!wa.col_weight || a16(wa.col_weight));
    const dim3 grid(mse_loss_colsum_rows(b->B));
    loss_dispatch(vec, ll.dy_bf16, ll.present != nullptr, [&](auto V, auto O, auto P) {
        swap_dispatch(wa, [&](auto W) {
            hipLaunchKernelGGL((emph_loss_kernel<decltype(V)::value, decltype(O)::value, decltype(P)::value, decltype(W)::value>), grid, dim3(NT), 0,
                               s, b->data, b->row_idx, b->mask_id, b->mask_table, b->B, b->io, ll.y, ll.dy, ll.scale, ll.colsum_part, ll.parts,
                               b->mask_to_use, b->nb_run, b->run, dy_ld, weight_args_of<decltype(W)::value>(wa), pres_args(ll));
        });
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
