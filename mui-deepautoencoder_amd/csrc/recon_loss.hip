// Training criterion other than the mean squared error (codae_recon_loss, include/codae_hip.h, "Training criterion"): the
// stand-alone loss kernels behind the last forward GEMM, on the seam emph_loss_kernel (elementwise.hip) uses - one block per
// LOSS_ROWS batch rows, dY + one partial column-sum row + three per-block sums, finished by finish_emph_loss_kernel.
//   recon_elem_kernel<KIND, ..>   L1 / SmoothL1 / Huber: the row sweep of loss_sweep.h with RhoTerm<KIND>
//   slot_cosine_kernel<..>        1 - cos per (row, slot): a wave reduces each pair, then the row sweep with CosineTerm writes dY
// The emphasis weight w of an element is formed exactly as emph_loss_kernel forms it (WeightArgs, loss_sweep.h).
#include "loss_sweep.h"

namespace codae {
namespace {

constexpr int NT = GRID_NT;
static_assert(NT == LOSS_NT, "loss_sweep strides the columns by LOSS_NT threads");
constexpr int WAVES = NT / 64;
constexpr int MAX_SLOTS = 128;   // slot_cosine: the coefficient table is LOSS_ROWS * n_slots * 2 floats of LDS (32 KiB at most)

// ---- L1 / SmoothL1 / Huber -----------------------------------------------------------------------------------------------------
//   dy = w rho'(d) (-1) inv_n, d = x - y;   parts[block] = { sum w rho(d), sum d^2, sum (1-fmask) d^2 }
template <int KIND, bool VEC, bool DY_BF16, bool PRES, bool SWAP = false>
__global__ __launch_bounds__(NT) void recon_elem_kernel(BatchArgs ba, const float* __restrict__ y, void* __restrict__ dy, float inv_n,
                                                        float* __restrict__ colsum_part, double* __restrict__ parts, int64_t dy_ld,
                                                        WeightArgsOf<SWAP> wa, ReconArgs ra, PresArgs pa) {
    __shared__ float red[WAVES];
    const bool masked = (ba.mask_id != nullptr) || (ba.mask_to_use != nullptr);
    RhoTerm<KIND> term(wa, ra, inv_n);
    loss_sweep<VEC, DY_BF16, PRES, SWAP>(ba, y, dy, dy_ld, colsum_part, pa, wa, term);
    const float bwr = block_sum(term.wr, red);
    const float bsq = block_sum(term.sq, red);
    const float bsqp = block_sum(term.sqp, red);
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
// Phase 2 (after one barrier): the row sweep with CosineTerm: g = -(a x - b y) + mse_weight 2 w (y - x) inv_n, dY, the column
// sums in registers, the squared-error sums.  x and y are read again (from L2: a block's rows are 2 x 32 x io x 4 B).
//   parts[block] = { mse_weight sum w d^2 + E sum W (1 - cos), sum d^2, sum (1-fmask) d^2 }
template <bool VEC1, bool SWAP>
__device__ __forceinline__ void slot_pair_sums(const BatchArgs& ba, const float* __restrict__ y, const WeightArgsOf<SWAP>& ea, int E, int b, int s,
                                               uint32_t step, float& dot, float& nx2, float& ny2, float& sw) {
    const int io = ba.io;
    const int lane = threadIdx.x & 63;
    const bool masked = (ba.mask_id != nullptr) || (ba.mask_to_use != nullptr);
    const int64_t src_row = ba.row_idx ? ba.row_idx[b] : b;
    const int id = !masked ? 0 : (ba.mask_id ? ba.mask_id[b] : ba.mask_to_use[src_row * ba.nb_run + ba.run]);
    const float* __restrict__ xr = ba.data + src_row * io;
    const float* __restrict__ yr = y + (int64_t)b * io;
    const uint8_t* __restrict__ tr = ba.table + (int64_t)id * io;
    const bool weighted = ea.col_weight != nullptr || ea.replace || ea.alpha != ea.beta;
    dot = 0.f; nx2 = 0.f; ny2 = 0.f; sw = 0.f;
    // swap noise: the pair's own draw when the swap's slots are the criterion's (one word per pair), else a draw per column
    bool swap_pair = false, pair_hit = false;
    if constexpr (SWAP) {
        swap_pair = ea.sw.E == E;
        pair_hit = weighted && swap_pair && swap_source(ea.sw, (uint32_t)src_row, s, step) >= 0;
    }
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
                if constexpr (SWAP) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) hit[k] = swap_pair ? pair_hit : swap_hit1(c + k, (uint32_t)src_row, step, ea.sw);
                } else {
                    if (ea.replace) hits4(hit, c, (uint32_t)src_row, step, ea);
                }
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
                    bool hit;
                    if constexpr (SWAP) hit = swap_pair ? pair_hit : swap_hit1(c + k, (uint32_t)src_row, step, ea.sw);
                    else hit = ea.replace ? hit1(c + k, (uint32_t)src_row, step, ea) : false;
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
template <bool VEC1, bool VEC, bool DY_BF16, bool PRES, bool SWAP = false>
__global__ __launch_bounds__(NT) void slot_cosine_kernel(BatchArgs ba, const float* __restrict__ y, void* __restrict__ dy, float inv_n,
                                                         float* __restrict__ colsum_part, double* __restrict__ parts, int64_t dy_ld,
                                                         WeightArgsOf<SWAP> ea, ReconArgs ra, PresArgs pa) {
    extern __shared__ float coef[];      // [LOSS_ROWS][S][2]
    __shared__ float red[WAVES];
    const int B = ba.B, S = ra.S, E = ra.E;
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
            slot_pair_sums<VEC1, SWAP>(ba, y, ea, E, r_begin + rr, s, step, dot, nx2, ny2, sw);
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
    const float mw = ra.mse_weight;
    CosineTerm term(coef, ea, ra, inv_n);
    loss_sweep<VEC, DY_BF16, PRES, SWAP>(ba, y, dy, dy_ld, colsum_part, pa, ea, term);
    // every lane of a wave holds the same cos_terms: count it once per wave
    const float bcos = block_sum((threadIdx.x & 63) == 0 ? cos_terms : 0.f, red);
    const float bwsq = block_sum(term.wsq, red);
    const float bsq = block_sum(term.sq, red);
    const float bsqp = block_sum(term.sqp, red);
    if (threadIdx.x == 0) {
        const double cos_part = (double)E * (double)bcos;
        parts[3 * blockIdx.x] = mw != 0.f ? (double)mw * (double)bwsq + cos_part : cos_part;
        parts[3 * blockIdx.x + 1] = (double)bsq;
        parts[3 * blockIdx.x + 2] = masked ? (double)bsqp : 0.0;
    }
}

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

int launch_recon_loss(const LossLaunch& ll, const codae_recon_loss* loss, hipStream_t s) {
    CODAE_REQUIRE(loss, "recon_loss: bad args");
    int rc = check_loss_launch("recon_loss", ll, true);
    if (rc) return rc;
    const codae_batch* b = ll.batch;
    CODAE_REQUIRE(ll.present == nullptr || loss->kind != CODAE_LOSS_SLOT_COSINE || loss->n_slots == ll.n_slots,
                  "recon_loss: slot_cosine n_slots %d differs from the presence table's %d", loss->n_slots, ll.n_slots);
    rc = check_recon_loss(loss, b->io);
    if (rc) return rc;
    CODAE_REQUIRE(loss->kind != CODAE_LOSS_MSE, "recon_loss: kind MSE runs on the mean-squared-error kernels (codae_emph_loss)");
    const SwapWeightArgs wa = weight_args(ll, ll.emph != nullptr);
    ReconArgs ra{};
    ra.param = loss->param; ra.rparam = (loss->kind == CODAE_LOSS_SMOOTH_L1) ? (float)(1.0 / (double)loss->param) : 0.f;
    const BatchArgs ba = batch_args(b);
    const PresArgs pa = pres_args(ll);
    const int64_t dy_ld = loss_dy_ld(ll);
    const bool in16 = loss_inputs_a16(ll) && (!wa.col_weight || a16(wa.col_weight));
    const bool vec = (b->io % 4 == 0) && (dy_ld % 4 == 0) && in16 && a16(ll.dy);
    const dim3 grid(mse_loss_colsum_rows(b->B)), block(NT);
    if (loss->kind == CODAE_LOSS_SLOT_COSINE) {
        ra.mse_weight = loss->mse_weight; ra.S = loss->n_slots; ra.E = b->io / loss->n_slots;
        const bool vec1 = (ra.E % 4 == 0) && in16;
        const size_t lds = (size_t)LOSS_ROWS * ra.S * 2 * sizeof(float);
        loss_dispatch(vec, ll.dy_bf16, ll.present != nullptr, [&](auto V, auto O, auto P) {
            constexpr bool v = decltype(V)::value, o = decltype(O)::value, p = decltype(P)::value;
            swap_dispatch(wa, [&](auto W) {
                constexpr bool w = decltype(W)::value;
                if (vec1) hipLaunchKernelGGL((slot_cosine_kernel<true, v, o, p, w>), grid, block, lds, s, ba, ll.y, ll.dy, ll.scale, ll.colsum_part,
                                             ll.parts, dy_ld, weight_args_of<w>(wa), ra, pa);
                else hipLaunchKernelGGL((slot_cosine_kernel<false, v, o, p, w>), grid, block, lds, s, ba, ll.y, ll.dy, ll.scale, ll.colsum_part,
                                        ll.parts, dy_ld, weight_args_of<w>(wa), ra, pa);
            });
        });
    } else {
        loss_dispatch(vec, ll.dy_bf16, ll.present != nullptr, [&](auto V, auto O, auto P) {
            constexpr bool v = decltype(V)::value, o = decltype(O)::value, p = decltype(P)::value;
            auto go = [&](auto K) {
                swap_dispatch(wa, [&](auto W) {
                    hipLaunchKernelGGL((recon_elem_kernel<decltype(K)::value, v, o, p, decltype(W)::value>), grid, block, 0, s, ba, ll.y, ll.dy,
                                       ll.scale, ll.colsum_part, ll.parts, dy_ld, weight_args_of<decltype(W)::value>(wa), ra, pa);
                });
            };
            if (loss->kind == CODAE_LOSS_L1) go(std::integral_constant<int, CODAE_LOSS_L1>{});
            else if (loss->kind == CODAE_LOSS_SMOOTH_L1) go(std::integral_constant<int, CODAE_LOSS_SMOOTH_L1>{});
            else go(std::integral_constant<int, CODAE_LOSS_HUBER>{});
        });
    }
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

}  // namespace codae
