// Mixed-variable criterion (codae_variable_loss, include/codae_hip.h, "Mixed-variable criterion"): the reference's
// CombinedCriterion(reduction="mean") as a criterion of the training step, on the seam of the other stand-alone losses - behind the
// last forward GEMM, one block per LOSS_ROWS batch rows, dY in the engine's type, one partial column-sum row per block.
// A regression variable's gradient needs the batch-wide sum of its squared errors before any dY exists, so three launches:
//   variable_partials_kernel   per (row block, variable) the block's sum in double: squared error (regression) or NLL
//                              (classification); per block the two unweighted squared-error sums of the monitors
//   variable_finish_kernel     one workgroup: every variable's blocks added IN INDEX ORDER, L_v, the coefficient of its dY, L
//   variable_grad_kernel       dY = coef_v (y - x) or coef_v (softmax - onehot), and the block's column sums of dY
// Work layout of the two row kernels: 32 consecutive lanes hold the 32 rows of the block for ONE variable (a wave: two variables),
// lane rr walks the variable's columns of row rr.  A sum over the block's rows is a butterfly inside the 32 lanes: no atomics, no
// LDS, an order that depends on nothing but the lane - the same inputs give the same bits.
// Work space (codae_variable_loss.ws): [n_var] VarEntry | [n_var] double coef | [blocks][n_var + 2] double parts.
#include <vector>

#include "loss_sweep.h"

namespace codae {
namespace {

constexpr int NT = LOSS_NT;
constexpr int GROUPS = NT / LOSS_ROWS;       // variables in flight per block
static_assert(LOSS_ROWS == 32, "a variable's rows are the 32 lanes of half a wave");

struct VarEntry { int32_t pos, size, type; float weight; };
static_assert(sizeof(VarEntry) == 16, "VarEntry is read as one 16-byte row of the work space");

// sum over the 32 lanes that share a variable (xor distances below 32 stay inside the half wave)
template <typename T>
__device__ __forceinline__ T rows_sum(T v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// what a lane needs of its row
struct RowRef { const float* x; const float* y; const uint8_t* t; bool live; int b; };
__device__ __forceinline__ RowRef row_ref(const BatchArgs& ba, const float* __restrict__ y) {
    const bool masked = (ba.mask_id != nullptr) || (ba.mask_to_use != nullptr);
    const int r = blockIdx.x * LOSS_ROWS + (threadIdx.x & (LOSS_ROWS - 1));
    RowRef rr;
    rr.live = r < ba.B;
    rr.b = rr.live ? r : ba.B - 1;           // (rows past the batch run on the last row's addresses and contribute nothing)
    const int64_t src_row = ba.row_idx ? ba.row_idx[rr.b] : rr.b;
    const int id = !masked ? 0 : (ba.mask_id ? ba.mask_id[rr.b] : ba.mask_to_use[src_row * ba.nb_run + ba.run]);
    rr.x = ba.data + src_row * ba.io;
    rr.y = y + (int64_t)rr.b * ba.io;
    rr.t = masked ? ba.table + (int64_t)id * ba.io : nullptr;
    return rr;
}

// classification: t = the first maximum of the clean slice, m = max y, se = sum exp(y - m) (a NaN in y reaches se)
__device__ __forceinline__ void softmax_stats(const float* __restrict__ xs, const float* __restrict__ ys, int size, int& t, float& m,
                                              float& se) {
    t = 0;
    float xm = xs[0];
    m = ys[0];
    for (int k = 1; k < size; ++k) {
        const float xv = xs[k], yv = ys[k];
        if (xv > xm) { xm = xv; t = k; }
        if (yv > m) m = yv;
    }
    se = 0.f;
    for (int k = 0; k < size; ++k) se += expf(ys[k] - m);
}

__global__ __launch_bounds__(NT) void variable_partials_kernel(BatchArgs ba, const float* __restrict__ y, const VarEntry* __restrict__ tab,
                                                               int n_var, double* __restrict__ parts) {
    __shared__ float red[NT / 64];
    const RowRef rr = row_ref(ba, y);
    const int lane_row = threadIdx.x & (LOSS_ROWS - 1), group = threadIdx.x / LOSS_ROWS;
    double* __restrict__ out = parts + (int64_t)blockIdx.x * (n_var + 2);
    float sq = 0.f, sqp = 0.f;
    for (int v0 = 0; v0 < n_var; v0 += GROUPS) {          // (the trip count is the block's: every lane reaches every butterfly)
        const int v = v0 + group;
        float val = 0.f;
        if (v < n_var && rr.live) {
            const VarEntry e = tab[v];
            const float* __restrict__ xs = rr.x + e.pos;
            const float* __restrict__ ys = rr.y + e.pos;
            float se = 0.f;
            for (int k = 0; k < e.size; ++k) {
                const float d = xs[k] - ys[k];
                const float d2 = d * d;
                se += d2;
                if (rr.t != nullptr && rr.t[e.pos + k] == 0) sqp += d2;
            }
            sq += se;
            if (e.type == CODAE_VAR_REGRESSION) {
                val = se;
            } else {
                int t;
                float m, sum;
                softmax_stats(xs, ys, e.size, t, m, sum);
                val = -((ys[t] - m) - logf(sum));
            }
        }
        const double block_val = rows_sum((double)val);
        if (v < n_var && lane_row == 0) out[v] = block_val;
    }
    const float bsq = block_sum(sq, red);
    const float bsqp = block_sum(sqp, red);
    if (threadIdx.x == 0) {
        out[n_var] = (double)bsq;
        out[n_var + 1] = rr.t != nullptr ? (double)bsqp : 0.0;
    }
}

// One workgroup.  coef[v]: dY = coef (y - x) for a regression variable - (w / n_var) / (B s L_v), inf when L_v is 0, so that an
// exactly reconstructed variable gets 0 * inf = NaN as torch's autograd of sqrt(mse) gives -, dY = coef (softmax - onehot) for a
// classification variable - (w / n_var) / B.  The epoch accumulators take the unweighted squared-error sums; the per-step norm
// accumulators are reset as the other finishes reset them.
__global__ __launch_bounds__(NT) void variable_finish_kernel(const VarEntry* __restrict__ tab, int n_var, int B, int blocks,
                                                             const double* __restrict__ parts, double* __restrict__ coef,
                                                             double* __restrict__ scalars) {
    __shared__ double red[3][NT];
    const int64_t stride = n_var + 2;
    double a[3] = {0.0, 0.0, 0.0};
    for (int v = threadIdx.x; v < n_var; v += NT) {
        double sum = 0.0;
        for (int i = 0; i < blocks; ++i) sum += parts[i * stride + v];
        const VarEntry e = tab[v];
        const double w = (double)e.weight;
        double Lv, c;
        if (e.type == CODAE_VAR_REGRESSION) {
            const double n = (double)B * (double)e.size;
            Lv = sqrt(sum / n);
            c = (w / (double)n_var) / (n * Lv);
        } else {
            Lv = sum / (double)B;
            c = (w / (double)n_var) / (double)B;
        }
        coef[v] = c;
        a[0] += w * Lv;
    }
    for (int i = threadIdx.x; i < blocks; i += NT) { a[1] += parts[i * stride + n_var]; a[2] += parts[i * stride + n_var + 1]; }
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
        scalars[CODAE_S_LAST_LOSS] = red[0][0] / (double)n_var;
        scalars[CODAE_S_STEP_SQ] = 0.0;
        scalars[CODAE_S_GRAD_SQ] = 0.0;
    }
    if (threadIdx.x < CODAE_S_N_SLOTS) scalars[CODAE_S_GRAD_SQ_SLOTS + threadIdx.x] = 0.0;
}

template <bool DY_BF16>
__global__ __launch_bounds__(NT) void variable_grad_kernel(BatchArgs ba, const float* __restrict__ y, const VarEntry* __restrict__ tab,
                                                           int n_var, const double* __restrict__ coef, void* __restrict__ dy, int64_t dy_ld,
                                                           float* __restrict__ colsum_part) {
    const RowRef rr = row_ref(ba, y);
    const int lane_row = threadIdx.x & (LOSS_ROWS - 1), group = threadIdx.x / LOSS_ROWS;
    for (int v0 = 0; v0 < n_var; v0 += GROUPS) {
        const int v = v0 + group;
        VarEntry e{0, 0, 0, 0.f};
        float c = 0.f, m = 0.f, rsum = 0.f;
        int t = 0;
        if (v < n_var) {
            e = tab[v];
            c = (float)coef[v];
            if (e.type != CODAE_VAR_REGRESSION) {
                float sum;
                softmax_stats(rr.x + e.pos, rr.y + e.pos, e.size, t, m, sum);
                rsum = 1.f / sum;
            }
        }
        // the two variables of a wave walk their columns together (the longer one's count): every butterfly runs with all 64 lanes
        const int other = __shfl_xor(e.size, 32);
        const int kmax = e.size > other ? e.size : other;
        for (int k = 0; k < kmax; ++k) {
            const bool on = k < e.size;
            float g = 0.f;
            if (on) {
                const float xv = rr.x[e.pos + k], yv = rr.y[e.pos + k];
                if (e.type == CODAE_VAR_REGRESSION) g = c * (yv - xv);
                else g = c * (expf(yv - m) * rsum - (k == t ? 1.f : 0.f));
                if (rr.live) {
                    const int64_t o = (int64_t)rr.b * dy_ld + e.pos + k;
                    if constexpr (DY_BF16) reinterpret_cast<bf16_t*>(dy)[o] = f32_to_bf16(g);
                    else reinterpret_cast<float*>(dy)[o] = g;
                }
            }
            const float cs = rows_sum(rr.live ? g : 0.f);
            if (on && lane_row == 0 && colsum_part != nullptr) colsum_part[(int64_t)blockIdx.x * ba.io + e.pos + k] = cs;
        }
    }
}

inline int64_t table_bytes(int n_var) { return (int64_t)n_var * (int64_t)sizeof(VarEntry); }

}  // namespace

int64_t variable_loss_ws_bytes(int n_var, int B) {
    if (n_var < 1 || n_var > CODAE_VAR_MAX || B < 1) return -1;
    return table_bytes(n_var) + 8 * ((int64_t)n_var + (int64_t)mse_loss_colsum_rows(B) * (n_var + 2));
}

int check_variable_loss(const codae_variable_loss* v, int io, int max_B) {
    CODAE_REQUIRE(v != nullptr, "variable loss: null struct");
    CODAE_REQUIRE(v->n_var >= 1 && v->n_var <= CODAE_VAR_MAX, "variable loss: n_var %d outside [1, %d]", v->n_var, CODAE_VAR_MAX);
    CODAE_REQUIRE(v->position && v->size && v->type && v->weight, "variable loss: null position / size / type / weight");
    int64_t next = 0;
    for (int i = 0; i < v->n_var; ++i) {
        CODAE_REQUIRE(v->size[i] >= 1, "variable loss: variable %d has size %d (must be >= 1)", i, v->size[i]);
        CODAE_REQUIRE(v->type[i] == CODAE_VAR_REGRESSION || v->type[i] == CODAE_VAR_CLASSIFICATION, "variable loss: variable %d has unknown type %d", i,
                      v->type[i]);
        CODAE_REQUIRE(finite_f(v->weight[i]) && v->weight[i] >= 0.f, "variable loss: variable %d has weight %g (must be finite and >= 0)", i,
                      (double)v->weight[i]);
        CODAE_REQUIRE(v->position[i] >= next, "variable loss: variable %d at position %d overlaps the one before it (which ends at %lld)", i,
                      v->position[i], (long long)next);
        CODAE_REQUIRE(v->position[i] == next, "variable loss: columns [%lld, %d) are covered by no variable", (long long)next, v->position[i]);
        next += v->size[i];
        CODAE_REQUIRE(io <= 0 || next <= io, "variable loss: variable %d ends at column %lld, past io %d", i, (long long)next, io);
    }
    CODAE_REQUIRE(io <= 0 || next == io, "variable loss: columns [%lld, %d) are covered by no variable", (long long)next, io);
    CODAE_REQUIRE(v->ws != nullptr && a16(v->ws), "variable loss: the work space must be there and 16-byte aligned");
    CODAE_REQUIRE(max_B < 1 || v->ws_bytes >= variable_loss_ws_bytes(v->n_var, max_B), "variable loss: work space of %lld bytes, %lld needed",
                  (long long)v->ws_bytes, (long long)variable_loss_ws_bytes(v->n_var, max_B));
    return CODAE_OK;
}

int variable_loss_upload(const codae_variable_loss* v) {
    std::vector<VarEntry> host((size_t)v->n_var);
    for (int i = 0; i < v->n_var; ++i) host[(size_t)i] = VarEntry{v->position[i], v->size[i], v->type[i], v->weight[i]};
    CODAE_HIP_CHECK(hipMemcpy(v->ws, host.data(), (size_t)table_bytes(v->n_var), hipMemcpyHostToDevice));
    return CODAE_OK;
}

int launch_variable_partials(const LossLaunch& ll, const void* ws, int n_var, hipStream_t s) {
    int rc = check_loss_launch("variable loss", ll, true);
    if (rc) return rc;
    CODAE_REQUIRE(ws != nullptr && n_var >= 1, "variable loss: no work space");
    const int blocks = mse_loss_colsum_rows(ll.batch->B);
    const VarEntry* tab = reinterpret_cast<const VarEntry*>(ws);
    double* coef = reinterpret_cast<double*>(const_cast<char*>(reinterpret_cast<const char*>(ws)) + table_bytes(n_var));
    hipLaunchKernelGGL(variable_partials_kernel, dim3(blocks), dim3(NT), 0, s, batch_args(ll.batch), ll.y, tab, n_var, coef + n_var);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_variable_finish(const LossLaunch& ll, const void* ws, int n_var, double* scalars, hipStream_t s) {
    CODAE_REQUIRE(scalars != nullptr, "variable loss: null scalars");
    const int blocks = mse_loss_colsum_rows(ll.batch->B);
    const VarEntry* tab = reinterpret_cast<const VarEntry*>(ws);
    double* coef = reinterpret_cast<double*>(const_cast<char*>(reinterpret_cast<const char*>(ws)) + table_bytes(n_var));
    hipLaunchKernelGGL(variable_finish_kernel, dim3(1), dim3(NT), 0, s, tab, n_var, ll.batch->B, blocks, coef + n_var, coef, scalars);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_variable_grad(const LossLaunch& ll, const void* ws, int n_var, hipStream_t s) {
    const int blocks = mse_loss_colsum_rows(ll.batch->B);
    const VarEntry* tab = reinterpret_cast<const VarEntry*>(ws);
    const double* coef = reinterpret_cast<const double*>(reinterpret_cast<const char*>(ws) + table_bytes(n_var));
    const int64_t dy_ld = loss_dy_ld(ll);
    if (ll.dy_bf16)
        hipLaunchKernelGGL(variable_grad_kernel<true>, dim3(blocks), dim3(NT), 0, s, batch_args(ll.batch), ll.y, tab, n_var, coef, ll.dy, dy_ld,
                           ll.colsum_part);
    else
        hipLaunchKernelGGL(variable_grad_kernel<false>, dim3(blocks), dim3(NT), 0, s, batch_args(ll.batch), ll.y, tab, n_var, coef, ll.dy, dy_ld,
                           ll.colsum_part);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

}  // namespace codae

using namespace codae;

int64_t codae_variable_loss_ws_bytes(int32_t n_var, int32_t max_batch) { return variable_loss_ws_bytes(n_var, max_batch); }

int codae_variable_loss_blocks(int32_t B) { return B > 0 ? mse_loss_colsum_rows(B) : 0; }

int codae_variable_loss_fwd_bwd(const codae_batch* batch, const codae_variable_loss* loss, const float* y, void* dy, int32_t dy_bf16,
                                int64_t dy_ld, float* colsum_part, double* scalars, void* stream) {
    CODAE_REQUIRE(batch != nullptr && batch->B >= 1, "codae_variable_loss_fwd_bwd: null or empty batch");
    int rc = check_variable_loss(loss, batch->io, batch->B);
    if (rc) return rc;
    CODAE_REQUIRE(scalars != nullptr, "codae_variable_loss_fwd_bwd: null scalars");
    LossLaunch ll{};
    ll.batch = batch; ll.y = y; ll.dy = dy; ll.dy_bf16 = dy_bf16; ll.dy_ld = dy_ld; ll.colsum_part = colsum_part;
    ll.parts = scalars;      // (check_loss_launch wants one; the per-block sums of this criterion live in its work space)
    rc = check_loss_launch("codae_variable_loss_fwd_bwd", ll, true);
    if (rc) return rc;
    rc = variable_loss_upload(loss);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    rc = launch_variable_partials(ll, loss->ws, loss->n_var, s);
    if (rc) return rc;
    rc = launch_variable_finish(ll, loss->ws, loss->n_var, scalars, s);
    if (rc) return rc;
    return launch_variable_grad(ll, loss->ws, loss->n_var, s);
}
