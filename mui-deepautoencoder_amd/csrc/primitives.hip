// Stand-alone C-ABI primitives of libcodae_hip.so: single kernels and single GEMMs on the caller's tensors, no engine.
#include "layer_gemm.h"

using namespace codae;

namespace {

int linear_f32(const char* who, const float* x, const float* W, const float* bias, float* y, int M, int N, int K, int relu, int act,
               const float* p, hipStream_t s) {
    CODAE_REQUIRE(x && W && y, "%s: null operand", who);
    GemmF32 g = fwd_gemm_f32(x, W, y, M, N, K, bias);
    set_activation(g, relu, act, p);
    return gemm_f32(g, s);
}

// src: the saved activation the mask / derivative is taken from, or null
int dgrad_f32(const char* who, const float* dy, const float* W, const float* src, float* dx, int M, int N, int K, int act, const float* p,
              hipStream_t s) {
    CODAE_REQUIRE(dy && W && dx, "%s: null operand", who);
    GemmF32 g = dgrad_gemm_f32(dy, W, dx, M, N, K);
    g.relu_src = src; g.ld_relu = K;
    set_activation(g, 0, act, p);
    return gemm_f32(g, s);
}

int linear_bf16(const char* who, const void* x, const void* W, const float* bias, void* y, int y_f32, int M, int N, int K, int relu,
                int act, const float* p, hipStream_t s) {
    CODAE_REQUIRE(x && W && y, "%s: null operand", who);
    GemmBf16 g = fwd_gemm_bf16(x, K, W, K, y, N, y_f32, M, N, K, bias);
    set_activation(g, relu, act, p);
    return gemm_bf16(g, s);
}

// data gradient, then (db_prev != null) the finish of its one bias job: db_prev[k] = column sums of dx
int dgrad_bf16(const char* who, const void* dy, const void* W, const void* src, void* dx, float* db_prev, float* db_ws, int M, int N,
               int K, int act, const float* p, hipStream_t s) {
    CODAE_REQUIRE(dy && W && dx, "%s: null operand", who);
    CODAE_REQUIRE(db_prev == nullptr || db_ws != nullptr, "%s: db_prev needs the db_ws scratch", who);
    GemmBf16 g = dgrad_gemm_bf16(dy, N, W, K, false, dx, K, 0, M, K, N);
    g.relu_src = reinterpret_cast<const bf16_t*>(src); g.ld_relu = K;
    g.colsum_part = db_prev ? db_ws : nullptr;
    set_activation(g, 0, act, p);
    int rc = gemm_bf16(g, s);
    if (rc || db_prev == nullptr) return rc;
    BiasFinishJobs jobs;
    jobs.n = 1; jobs.parts[0] = db_ws; jobs.out[0] = db_prev; jobs.rows[0] = gemm_bf16_colsum_rows(g); jobs.cols[0] = K;
    jobs.col_begin[0] = 0; jobs.col_begin[1] = K;
    return launch_bias_finish(jobs, nullptr, s);
}

// the C entry points' arguments as one stand-alone loss launch (no device step scalar: these run outside any graph)
LossLaunch loss_launch(const codae_batch* batch, const codae_noise* noise, int32_t step, const codae_emphasis* emphasis, const float* y,
                       void* dy, int32_t dy_bf16, int64_t dy_ld, float scale, float* colsum_part, double* parts,
                       const uint8_t* present = nullptr, int32_t n_slots = 0, const codae_swap* swap = nullptr) {
    return LossLaunch{batch, noise, step, nullptr, emphasis, present, n_slots, y, dy, dy_bf16, dy_ld, scale, colsum_part, parts, swap};
}

}  // namespace

extern "C" {

int codae_corrupt(const float* x, const float* mask, float* out, int64_t n, void* stream) {
    return launch_corrupt(x, mask, out, n, (hipStream_t)stream);
}

int codae_corrupt_batch(const codae_batch* batch, const codae_noise* noise, int32_t step, const int32_t* noise_rows, void* out,
                        int32_t out_bf16, int64_t out_ld, void* stream) {
    CODAE_REQUIRE(noise_rows == nullptr || (batch != nullptr && batch->row_idx == nullptr), "codae_corrupt_batch: noise_rows go with an already gathered batch (row_idx NULL)");
    return launch_gather_noise(batch, noise, step, nullptr, out, out_bf16, (hipStream_t)stream, out_ld, noise_rows);
}

int codae_emph_loss(const codae_batch* batch, const codae_noise* noise, int32_t step, const codae_emphasis* emphasis, const float* y,
                    void* dy, int32_t dy_bf16, int64_t dy_ld, float inv_n, float* colsum_part, double* parts, void* stream) {
    return launch_emph_loss(loss_launch(batch, noise, step, emphasis, y, dy, dy_bf16, dy_ld, inv_n, colsum_part, parts), (hipStream_t)stream);
}

int codae_corrupt_batch_present(const codae_batch* batch, const codae_noise* noise, int32_t step, const int32_t* noise_rows, void* out,
                                int32_t out_bf16, int64_t out_ld, const uint8_t* present, int32_t n_slots, void* stream) {
    CODAE_REQUIRE(noise_rows == nullptr || (batch != nullptr && batch->row_idx == nullptr), "codae_corrupt_batch_present: noise_rows go with an already gathered batch (row_idx NULL)");
    return launch_gather_noise(batch, noise, step, nullptr, out, out_bf16, (hipStream_t)stream, out_ld, noise_rows, nullptr, present, n_slots);
}

int codae_mse_loss_present(const codae_batch* batch, const float* y, void* dy, int32_t dy_bf16, int64_t dy_ld, float inv_n,
                           float* colsum_part, double* parts, const uint8_t* present, int32_t n_slots, void* stream) {
    return launch_mse_loss(loss_launch(batch, nullptr, 0, nullptr, y, dy, dy_bf16, dy_ld, inv_n, colsum_part, parts, present, n_slots), dy != nullptr,
                           (hipStream_t)stream);
}

int codae_emph_loss_present(const codae_batch* batch, const codae_noise* noise, int32_t step, const codae_emphasis* emphasis, const float* y,
                            void* dy, int32_t dy_bf16, int64_t dy_ld, float inv_n, float* colsum_part, double* parts,
                            const uint8_t* present, int32_t n_slots, void* stream) {
    return launch_emph_loss(loss_launch(batch, noise, step, emphasis, y, dy, dy_bf16, dy_ld, inv_n, colsum_part, parts, present, n_slots),
                            (hipStream_t)stream);
}

int codae_recon_loss_fwd_bwd_present(const codae_batch* batch, const codae_noise* noise, int32_t step, const codae_emphasis* emphasis,
                                     const codae_recon_loss* loss, const float* y, void* dy, int32_t dy_bf16, int64_t dy_ld, float inv_n,
                                     float* colsum_part, double* parts, const uint8_t* present, int32_t n_slots, void* stream) {
    return launch_recon_loss(loss_launch(batch, noise, step, emphasis, y, dy, dy_bf16, dy_ld, inv_n, colsum_part, parts, present, n_slots), loss,
                             (hipStream_t)stream);
}

int codae_slot_contrast_prepare_present(const float* data, int32_t io, const codae_slot_contrast* contrast, int32_t step, int32_t bf16,
                                        const uint8_t* present, int32_t n_slots, void* stream) {
    return launch_slot_contrast_prepare(data, io, contrast, step, nullptr, bf16, (hipStream_t)stream, present, n_slots);
}

int codae_slot_contrast_fwd_bwd_present(const codae_batch* batch, const codae_noise* noise, int32_t step, const codae_emphasis* emphasis,
                                        const codae_slot_contrast* contrast, const float* y, void* dy, int32_t dy_bf16, int64_t dy_ld,
                                        float scale, float* colsum_part, double* parts, const uint8_t* present, int32_t n_slots, void* stream) {
    return launch_slot_contrast(loss_launch(batch, noise, step, emphasis, y, dy, dy_bf16, dy_ld, scale, colsum_part, parts, present, n_slots),
                                contrast, (hipStream_t)stream);
}

int codae_corrupt_batch_swap(const codae_batch* batch, const codae_noise* noise, int32_t step, const int32_t* noise_rows, const void* dataset,
                             const codae_swap* swap, void* out, int32_t out_bf16, int64_t out_ld, const uint8_t* present, int32_t image,
                             void* stream) {
    CODAE_REQUIRE(batch != nullptr && noise != nullptr && noise->kind == CODAE_NOISE_SWAP && swap != nullptr,
                  "codae_corrupt_batch_swap: needs a batch, a CODAE_NOISE_SWAP noise and its codae_swap");
    CODAE_REQUIRE(noise_rows == nullptr || batch->row_idx == nullptr, "codae_corrupt_batch_swap: noise_rows go with an already gathered batch (row_idx NULL)");
    if (image) {
        CODAE_REQUIRE(out_bf16 && noise_rows == nullptr && (dataset == nullptr || dataset == (const void*)batch->data),
                      "codae_corrupt_batch_swap: the image gather writes bf16 and reads the one image (no noise_rows, no other dataset)");
        return launch_gather_image(batch, reinterpret_cast<const bf16_t*>(batch->data), reinterpret_cast<bf16_t*>(out), (hipStream_t)stream, out_ld,
                                   nullptr, present, present ? swap->n_slots : 0, noise, step, nullptr, swap);
    }
    return launch_gather_noise(batch, noise, step, nullptr, out, out_bf16, (hipStream_t)stream, out_ld, noise_rows, nullptr, present,
                               present ? swap->n_slots : 0, swap, reinterpret_cast<const float*>(dataset));
}

int codae_emph_loss_swap(const codae_batch* batch, const codae_noise* noise, int32_t step, const codae_emphasis* emphasis, const float* y,
                         void* dy, int32_t dy_bf16, int64_t dy_ld, float inv_n, float* colsum_part, double* parts, const codae_swap* swap,
                         const uint8_t* present, int32_t n_slots, void* stream) {
    return launch_emph_loss(loss_launch(batch, noise, step, emphasis, y, dy, dy_bf16, dy_ld, inv_n, colsum_part, parts, present, n_slots, swap),
                            (hipStream_t)stream);
}

int codae_recon_loss_fwd_bwd_swap(const codae_batch* batch, const codae_noise* noise, int32_t step, const codae_emphasis* emphasis,
                                  const codae_recon_loss* loss, const float* y, void* dy, int32_t dy_bf16, int64_t dy_ld, float inv_n,
                                  float* colsum_part, double* parts, const codae_swap* swap, const uint8_t* present, int32_t n_slots,
                                  void* stream) {
    return launch_recon_loss(loss_launch(batch, noise, step, emphasis, y, dy, dy_bf16, dy_ld, inv_n, colsum_part, parts, present, n_slots, swap),
                             loss, (hipStream_t)stream);
}

int codae_emph_loss_blocks(int32_t B) { return B > 0 ? mse_loss_colsum_rows(B) : 0; }

int codae_recon_loss_fwd_bwd(const codae_batch* batch, const codae_noise* noise, int32_t step, const codae_emphasis* emphasis,
                             const codae_recon_loss* loss, const float* y, void* dy, int32_t dy_bf16, int64_t dy_ld, float inv_n,
                             float* colsum_part, double* parts, void* stream) {
    return launch_recon_loss(loss_launch(batch, noise, step, emphasis, y, dy, dy_bf16, dy_ld, inv_n, colsum_part, parts), loss, (hipStream_t)stream);
}

int codae_recon_loss_blocks(int32_t B) { return B > 0 ? mse_loss_colsum_rows(B) : 0; }

int64_t codae_slot_contrast_ws_bytes(int32_t n_slots, int32_t n_neg, int32_t E, int32_t bf16) {
    return slot_contrast_ws_bytes(n_slots, n_neg, E, bf16);
}

int codae_slot_contrast_prepare(const float* data, int32_t io, const codae_slot_contrast* contrast, int32_t step, int32_t bf16, void* stream) {
    return launch_slot_contrast_prepare(data, io, contrast, step, nullptr, bf16, (hipStream_t)stream);
}

int codae_slot_contrast_fwd_bwd(const codae_batch* batch, const codae_noise* noise, int32_t step, const codae_emphasis* emphasis,
                                const codae_slot_contrast* contrast, const float* y, void* dy, int32_t dy_bf16, int64_t dy_ld, float scale,
                                float* colsum_part, double* parts, void* stream) {
    return launch_slot_contrast(loss_launch(batch, noise, step, emphasis, y, dy, dy_bf16, dy_ld, scale, colsum_part, parts), contrast,
                                (hipStream_t)stream);
}

int codae_slot_contrast_blocks(int32_t B) { return B > 0 ? slot_contrast_blocks(B) : 0; }

int codae_dropout_fwd(void* a, int32_t bf16, int64_t ld, int32_t B, int32_t width, const int32_t* row_idx, int32_t layer, int32_t step,
                      float p, uint64_t seed, void* stream) {
    return launch_dropout_fwd(a, bf16, ld, B, width, row_idx, layer, step, nullptr, p, seed, (hipStream_t)stream);
}

int codae_dropout_bwd(void* d, int32_t bf16, int64_t ld, int32_t B, int32_t width, const int32_t* row_idx, int32_t layer, int32_t step,
                      float p, uint64_t seed, float* colsum_part, void* stream) {
    return launch_dropout_bwd(d, bf16, ld, B, width, row_idx, layer, step, nullptr, p, seed, colsum_part, (hipStream_t)stream);
}

int codae_dropout_blocks(int32_t B) { return B > 0 ? row_sweep_blocks(B) : 0; }

int codae_residual_fwd(void* y, const void* x, int32_t bf16, int64_t ldy, int64_t ldx, int32_t B, int32_t width, uint8_t* bits,
                       int64_t ld_bits, void* stream) {
    return launch_residual_fwd(y, x, bf16, ldy, ldx, B, width, bits, ld_bits, (hipStream_t)stream);
}

int codae_residual_bwd(void* d, int32_t bf16, int64_t ld, int32_t B, int32_t width, const float* g_in, float* g_out, int64_t ld_g,
                       const uint8_t* bits, int64_t ld_bits, const void* src, int64_t ld_src, int32_t act_kind, const float* act_param,
                       float* colsum_part, void* stream) {
    ResidualBwd r{{g_in, g_out, ld_g, bits, ld_bits, act_kind, 0.f}, src, ld_src, {0.f, 0.f, 0.f}};
    for (int k = 0; k < 3 && act_param != nullptr; ++k) r.act_p[k] = act_param[k];
    r.slope = r.act_p[0];
    return launch_residual_bwd(d, bf16, ld, B, width, r, colsum_part, (hipStream_t)stream);
}

int codae_residual_blocks(int32_t B) { return B > 0 ? row_sweep_blocks(B) : 0; }

int codae_norm_fwd(void* y, int32_t bf16, int64_t ld, int32_t B, int32_t width, int32_t kind, float eps, float* rstd, uint8_t* bits,
                   int64_t ld_bits, void* stream) {
    return launch_norm_fwd(y, bf16, ld, B, width, kind, eps, rstd, bits, ld_bits, (hipStream_t)stream);
}

int codae_norm_bwd(void* d, int32_t bf16, int64_t ld, int32_t B, int32_t width, int32_t kind, const void* xhat, int64_t ld_x,
                   const float* rstd, const float* g_in, float* g_out, int64_t ld_g, const uint8_t* bits, int64_t ld_bits,
                   int32_t act_kind, const float* act_param, float* colsum_part, void* stream) {
    NormBwd n{{g_in, g_out, ld_g, bits, ld_bits, act_kind, act_param != nullptr ? act_param[0] : 0.f}, xhat, ld_x, rstd};
    return launch_norm_bwd(d, bf16, ld, B, width, kind, n, colsum_part, (hipStream_t)stream);
}

int codae_norm_blocks(int32_t B) { return B > 0 ? row_sweep_blocks(B) : 0; }

int codae_sparse_code_fwd(void* y, int32_t bf16, int64_t ld, int32_t B, int32_t width, int32_t keep, uint8_t* bits, int64_t ld_bits,
                          void* stream) {
    return launch_sparse_code_fwd(y, bf16, ld, B, width, keep, bits, ld_bits, (hipStream_t)stream);
}

int codae_sparse_code_bwd(void* d, int32_t bf16, int64_t ld, int32_t B, int32_t width, const uint8_t* bits, int64_t ld_bits,
                          float* colsum_part, void* stream) {
    return launch_sparse_code_bwd(d, bf16, ld, B, width, bits, ld_bits, colsum_part, (hipStream_t)stream);
}

int codae_sparse_code_blocks(int32_t B) { return B > 0 ? row_sweep_blocks(B) : 0; }

int codae_export_rows(const void* src, int32_t bf16, int64_t ld_src, int32_t B, int32_t width, float* dst, int64_t ld_dst, float* norm,
                      void* stream) {
    return launch_export_rows(src, bf16, ld_src, B, width, dst, ld_dst, norm, (hipStream_t)stream);
}

int codae_noise_box_muller(const uint32_t* ra, const uint32_t* rb, float* rho, float* c, float* s, int64_t n, void* stream) {
    return launch_noise_box_muller(ra, rb, rho, c, s, n, (hipStream_t)stream);
}

int codae_expand_masks(const int32_t* mask_id, const uint8_t* mask_table, const int32_t* k_of_mask, int32_t B, int32_t io,
                       int32_t k_max, float* masks_out, float* fmask_out, void* stream) {
    return launch_expand_masks(mask_id, mask_table, k_of_mask, B, io, k_max, masks_out, fmask_out, (hipStream_t)stream);
}

int codae_mse_loss_fwd_bwd(const float* x, const float* y, const float* fmask, float* dy, int64_t n, float inv_n,
                           double* scalars, void* stream) {
    int rc = launch_mse_dense(x, y, fmask, dy, n, inv_n, scalars, (hipStream_t)stream);
    if (rc) return rc;
    return launch_finish_loss(scalars, 1.0 / (double)n, (hipStream_t)stream);
}

// (codae_optimizer_update with opt NULL: the default Adam, the instantiation this entry always ran)
int codae_clip_adam(float* params, float* grads, float* adam_m, float* adam_v, int64_t n, const codae_hyper* hyper,
                    double* scalars, void* stream) {
    CODAE_REQUIRE(hyper && scalars, "codae_clip_adam: null argument");
    return codae_optimizer_update(params, grads, adam_m, adam_v, nullptr, n, hyper, nullptr, scalars, stream);
}

int codae_optimizer_update(float* p, float* g, float* m, float* v, float* vmax, int64_t n, const codae_hyper* hyper,
                           const codae_optimizer* opt, double* scalars, void* stream) {
    CODAE_REQUIRE(hyper && scalars, "codae_optimizer_update: null argument");
    CODAE_REQUIRE(!is_trust_kind(opt), "codae_optimizer_update: lamb / lars need a work space: codae_trust_update");
    codae_optimizer o{};
    if (opt != nullptr) { o = *opt; o.vmax = vmax; }       // (the range checks are the setter's; the maximum is this call's own)
    int rc = check_optimizer(opt != nullptr ? &o : nullptr);
    if (rc) return rc;
    o = optimizer_canonical(opt != nullptr ? &o : nullptr);
    hipStream_t s = (hipStream_t)stream;
    if (hyper->max_grad_norm > 0.f) {
        rc = launch_grad_sumsq(g, n, scalars, true, s);
        if (rc) return rc;
    }
    UpdateLaunch u{};
    u.x.p = p; u.x.g = g; u.x.m = m; u.x.v = v; u.x.vmax = o.vmax; u.n = n; u.hp = hyper; u.grad_sq = scalars + CODAE_S_GRAD_SQ; u.opt = &o;
    return launch_update(u, s);
}

int64_t codae_trust_ws_bytes_flat(int64_t n) {
    return n > 0 ? CODAE_TRUST_MAX_MATRICES * (int64_t)sizeof(float) + 2 * (int64_t)sizeof(double) * trust_parts_flat(n) : 0;
}

int codae_trust_update(float* p, float* g, float* m, float* v, int64_t n, const codae_hyper* hyper, const codae_optimizer* opt,
                       double* scalars, void* trust_ws, int64_t ws_bytes, void* stream) {
    CODAE_REQUIRE(hyper && scalars && opt, "codae_trust_update: null argument");
    CODAE_REQUIRE(is_trust_kind(opt), "codae_trust_update: kind %d is neither lamb nor lars", opt->kind);
    CODAE_REQUIRE(n > 0 && trust_ws != nullptr && ws_bytes >= codae_trust_ws_bytes_flat(n), "codae_trust_update: trust_ws of %lld bytes, %lld needed",
                  (long long)ws_bytes, (long long)codae_trust_ws_bytes_flat(n));
    codae_optimizer o = *opt;
    o.vmax = nullptr; o.trust_ws = trust_ws;               // (the range checks are the setter's; the work space is this call's own)
    int rc = check_optimizer(&o);
    if (rc) return rc;
    o = optimizer_canonical(&o);
    hipStream_t s = (hipStream_t)stream;
    if (hyper->max_grad_norm > 0.f) {
        rc = launch_grad_sumsq(g, n, scalars, true, s);
        if (rc) return rc;
    }
    UpdateLaunch u{};
    u.x.p = p; u.x.g = g; u.x.m = m; u.x.v = v; u.n = n; u.hp = hyper; u.grad_sq = scalars + CODAE_S_GRAD_SQ; u.opt = &o;
    const int64_t off = 0;
    rc = launch_trust_norms(u, 1, &off, &n, s);
    if (rc) return rc;
    return launch_update(u, s);
}

int codae_weight_average_update(float* avg, const float* p, int64_t n, const codae_weight_average* wa, int32_t step, void* stream) {
    return launch_weight_average(avg, p, n, wa, step, (hipStream_t)stream);
}

// ---- GEMM primitives ------------------------------------------------------------------------
// The plain entry points run the ReLU / identity code (`relu`); the _act_ ones the generic-activation instantiation, CODAE_ACT_RELU
// included, and hand CODAE_ACT_NONE (or a data gradient without a saved activation) to the plain one.

int codae_linear_f32(const float* x, const float* W, const float* bias, float* y, int32_t M, int32_t N, int32_t K,
                     int32_t relu, void* stream) {
    return linear_f32("codae_linear_f32", x, W, bias, y, M, N, K, relu, CODAE_ACT_NONE, nullptr, (hipStream_t)stream);
}

int codae_dgrad_f32(const float* dy, const float* W, const float* relu_src, float* dx, int32_t M, int32_t N, int32_t K,
                    void* stream) {
    return dgrad_f32("codae_dgrad_f32", dy, W, relu_src, dx, M, N, K, CODAE_ACT_NONE, nullptr, (hipStream_t)stream);
}

int codae_wgrad_f32(const float* dy, const float* x, float* dW, float* db, int32_t M, int32_t N, int32_t K, void* stream) {
    CODAE_REQUIRE(dy && x && dW, "codae_wgrad_f32: null operand");
    int rc = gemm_f32(wgrad_gemm_f32(dy, x, dW, M, N, K), (hipStream_t)stream);
    if (rc) return rc;
    if (db) return launch_colsum_f32(dy, M, N, db, (hipStream_t)stream);
    return CODAE_OK;
}

int codae_linear_bf16(const void* x, const void* W, const float* bias, void* y, int32_t y_f32, int32_t M, int32_t N,
                      int32_t K, int32_t relu, void* stream) {
    return linear_bf16("codae_linear_bf16", x, W, bias, y, y_f32, M, N, K, relu, CODAE_ACT_NONE, nullptr, (hipStream_t)stream);
}

int codae_dgrad_bf16(const void* dy, const void* W, const void* relu_src, void* dx, float* db_prev, float* db_ws, int32_t M,
                     int32_t N, int32_t K, void* stream) {
    return dgrad_bf16("codae_dgrad_bf16", dy, W, relu_src, dx, db_prev, db_ws, M, N, K, CODAE_ACT_NONE, nullptr, (hipStream_t)stream);
}

int codae_linear_act_f32(const float* x, const float* W, const float* bias, float* y, int32_t M, int32_t N, int32_t K, int32_t act,
                         float p0, float p1, float p2, void* stream) {
    CODAE_REQUIRE(act >= CODAE_ACT_NONE && act <= CODAE_ACT_HARDSIGMOID, "codae_linear_act_f32: activation kind %d", act);
    if (act == CODAE_ACT_NONE) return codae_linear_f32(x, W, bias, y, M, N, K, 0, stream);
    const float p[3] = {p0, p1, p2};
    return linear_f32("codae_linear_act_f32", x, W, bias, y, M, N, K, 0, act, p, (hipStream_t)stream);
}

int codae_dgrad_act_f32(const float* dy, const float* W, const float* act_src, float* dx, int32_t M, int32_t N, int32_t K, int32_t act,
                        float p0, float p1, float p2, void* stream) {
    CODAE_REQUIRE(act >= CODAE_ACT_NONE && act <= CODAE_ACT_HARDSIGMOID, "codae_dgrad_act_f32: activation kind %d", act);
    if (act == CODAE_ACT_NONE || act_src == nullptr) return codae_dgrad_f32(dy, W, nullptr, dx, M, N, K, stream);
    const float p[3] = {p0, p1, p2};
    return dgrad_f32("codae_dgrad_act_f32", dy, W, act_src, dx, M, N, K, act, p, (hipStream_t)stream);
}

int codae_linear_act_bf16(const void* x, const void* W, const float* bias, void* y, int32_t y_f32, int32_t M, int32_t N, int32_t K,
                          int32_t act, float p0, float p1, float p2, void* stream) {
    CODAE_REQUIRE(act >= CODAE_ACT_NONE && act <= CODAE_ACT_HARDSIGMOID, "codae_linear_act_bf16: activation kind %d", act);
    if (act == CODAE_ACT_NONE) return codae_linear_bf16(x, W, bias, y, y_f32, M, N, K, 0, stream);
    const float p[3] = {p0, p1, p2};
    return linear_bf16("codae_linear_act_bf16", x, W, bias, y, y_f32, M, N, K, 0, act, p, (hipStream_t)stream);
}

int codae_dgrad_act_bf16(const void* dy, const void* W, const void* act_src, void* dx, float* db_prev, float* db_ws, int32_t M,
                         int32_t N, int32_t K, int32_t act, float p0, float p1, float p2, void* stream) {
    CODAE_REQUIRE(act >= CODAE_ACT_NONE && act <= CODAE_ACT_HARDSIGMOID, "codae_dgrad_act_bf16: activation kind %d", act);
    if (act == CODAE_ACT_NONE || act_src == nullptr) return codae_dgrad_bf16(dy, W, nullptr, dx, db_prev, db_ws, M, N, K, stream);
    const float p[3] = {p0, p1, p2};
    return dgrad_bf16("codae_dgrad_act_bf16", dy, W, act_src, dx, db_prev, db_ws, M, N, K, act, p, (hipStream_t)stream);
}

int codae_wgrad_bf16(const void* dy, const void* x, float* dW, void* slabs, int64_t slab_bytes, int32_t M, int32_t N,
                     int32_t K, void* stream) {
    CODAE_REQUIRE(dy && x && dW, "codae_wgrad_bf16: null operand");
    CODAE_REQUIRE(M % 64 == 0, "codae_wgrad_bf16: batch rows %d must be a multiple of 64 (pad with zero rows)", M);
    int S = choose_split_k(N, K, M);
    while (S > 1 && (slabs == nullptr || (int64_t)S * N * K * 4 > slab_bytes)) --S;
    GemmBf16 g = wgrad_gemm_bf16(dy, N, x, K, S > 1 ? slabs : (void*)dW, M, N, K);
    g.split_k = S;
    int rc = gemm_bf16(g, (hipStream_t)stream);
    if (rc) return rc;
    if (S > 1) return launch_reduce_slabs(reinterpret_cast<const float*>(slabs), S, (int64_t)N * K, dW, (int64_t)N * K, nullptr, (hipStream_t)stream);
    return CODAE_OK;
}

// what gemm_bf16() would launch for a descriptor with these facts: the plan, and the counts the engine derives from it
int codae_debug_gemm_bf16_plan(const int32_t* desc, int32_t* out, int32_t capacity) {
    CODAE_REQUIRE(desc && out && capacity >= CODAE_GEMM_PLAN_FIELDS, "codae_debug_gemm_bf16_plan: needs room for %d fields", CODAE_GEMM_PLAN_FIELDS);
    GemmBf16 g{};
    g.a_mode = desc[0]; g.b_mode = desc[1]; g.c_f32 = desc[2]; g.M = desc[3]; g.N = desc[4]; g.K = desc[5]; g.split_k = desc[6];
    g.act = desc[7]; g.loss.enabled = desc[8]; g.coscheduled = desc[10]; g.store_policy = desc[11]; g.ldc = desc[12];
    if (desc[11] < 0) g.store_policy = store_policy_for((int64_t)g.M * g.N * (g.c_f32 ? 4 : 2));      // (as the descriptor builders of layer_gemm.h)
    static float some_rows;
    if (desc[9]) g.colsum_part = &some_rows;          // (the plan only asks whether there is a backward epilogue; nothing is launched)
    CODAE_REQUIRE(gemm_bf16_supported(g.M, g.N, g.K) && g.split_k >= 1, "codae_debug_gemm_bf16_plan: unsupported shape M=%d N=%d K=%d", g.M, g.N, g.K);
    const Bf16Plan p = gemm_bf16_plan(g);
    const int32_t fields[CODAE_GEMM_PLAN_FIELDS] = {p.family, p.bm, p.bn, p.stages, p.loader, p.epi, p.sched, p.act, p.store_policy, p.tiles_m, p.tiles_n,
                                                    (int32_t)p.workgroups, gemm_bf16_colsum_rows(g), g.loss.enabled ? gemm_bf16_loss_parts(g) : 0,
                                                    gemm_bf16_takes_relu_bits(g.M, g.N) ? 1 : 0};
    for (int i = 0; i < CODAE_GEMM_PLAN_FIELDS; ++i) out[i] = fields[i];
    return CODAE_OK;
}

int codae_debug_gemm_bf16(const void* A, int64_t lda, int32_t a_mode, const void* B, int64_t ldb, int32_t b_mode, void* C, int64_t ldc,
                          int32_t c_f32, int32_t M, int32_t N, int32_t K, int32_t split_k, const float* bias, int32_t relu, void* stream) {
    CODAE_REQUIRE(A && B && C, "codae_debug_gemm_bf16: null operand");
    CODAE_REQUIRE((a_mode == OP_KC || a_mode == OP_KS) && (b_mode == OP_KC || b_mode == OP_KS), "codae_debug_gemm_bf16: operand modes %d, %d", a_mode, b_mode);
    CODAE_REQUIRE(split_k >= 1 && (c_f32 ? (bias == nullptr && !relu) : split_k == 1), "codae_debug_gemm_bf16: epilogue and output kind do not go together");
    CODAE_REQUIRE(lda >= (a_mode == OP_KC ? K : M) && ldb >= (b_mode == OP_KC ? K : N) && ldc >= N,
                  "codae_debug_gemm_bf16: a leading dimension is shorter than its row");
    GemmBf16 g{};
    g.A = reinterpret_cast<const bf16_t*>(A); g.lda = lda; g.a_mode = a_mode;
    g.B = reinterpret_cast<const bf16_t*>(B); g.ldb = ldb; g.b_mode = b_mode;
    g.C = C; g.ldc = ldc; g.c_f32 = c_f32 != 0 ? 1 : 0;
    g.M = M; g.N = N; g.K = K;
    g.bias = bias; g.split_k = split_k;
    g.store_policy = store_policy_for((int64_t)M * N * (c_f32 ? 4 : 2));
    set_activation(g, relu != 0, CODAE_ACT_NONE, nullptr);
    return gemm_bf16(g, (hipStream_t)stream);
}

int codae_transpose_bf16(const void* src, void* dst, int32_t rows, int32_t cols, void* stream) {
    CODAE_REQUIRE(src && dst && rows > 0 && cols > 0, "transpose: bad args");
    const int64_t off = 0;
    return launch_transpose_bf16(reinterpret_cast<const bf16_t*>(src), reinterpret_cast<bf16_t*>(dst), 1, &off, &rows, &cols,
                                 (hipStream_t)stream);
}

int codae_corrupt_batch_image(const codae_batch* batch, const void* image_bf16, const uint8_t* present, int32_t n_slots, void* out,
                              int64_t out_ld, void* stream) {
    return launch_gather_image(batch, reinterpret_cast<const bf16_t*>(image_bf16), reinterpret_cast<bf16_t*>(out), (hipStream_t)stream, out_ld,
                               nullptr, present, n_slots);
}

int codae_cast_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream) {
    return launch_cast_bf16(src, reinterpret_cast<bf16_t*>(dst), n, (hipStream_t)stream);
}

}  // extern "C"
