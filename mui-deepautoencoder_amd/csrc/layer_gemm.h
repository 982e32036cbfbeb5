// The three GEMMs of a Linear layer - forward y = x W^T + b, data gradient dx = dy W, weight gradient dW = dy^T x - as
// launch descriptors, once per role and precision.  Host code only (engine.hip, primitives.hip).  A builder takes what
// varies between callers (operand pointers, leading dimensions, extents, bias, output kind) and sets what the role fixes:
// operand modes / strides, which extent is the batch, split_k = 1.  Everything else stays zero for the caller to add
// (activation, mask source, column sums, prefetch, fused loss, split-K slabs, norm slots).  The output store policy comes from
// the output's size (store_policy_for).
// x [rows][n_in], W [n_out][n_in], y / dy [rows][n_out]; ld*: row strides in elements.
#pragma once
#include "codae_common.h"

namespace codae {

// k: the reduction extent - n_in, or x's padded row width (the pad columns of x are zeros, see codae_engine::in_ld)
inline GemmBf16 fwd_gemm_bf16(const void* x, int64_t ldx, const void* W, int64_t ldw, void* y, int64_t ldy, int y_f32,
                              int rows, int n_out, int k, const float* bias) {
    GemmBf16 g{};
    g.A = reinterpret_cast<const bf16_t*>(x); g.lda = ldx; g.a_mode = OP_KC;
    g.B = reinterpret_cast<const bf16_t*>(W); g.ldb = ldw; g.b_mode = OP_KC;
    g.C = y; g.ldc = ldy; g.c_f32 = y_f32;
    g.M = rows; g.N = n_out; g.K = k;
    g.bias = bias; g.split_k = 1;
    g.store_policy = store_policy_for((int64_t)rows * n_out * (y_f32 ? 4 : 2));
    return g;
}

// W: [n_out][ldw = n_in], or with w_transposed the transposed copy [n_in][ldw = n_out] - dx[m][j] = sum_n dy[m][n] Wt[j][n], both
// operands k-contiguous: the forward-form kernel.  k: n_out, or dy's padded row width (zero pad columns)
inline GemmBf16 dgrad_gemm_bf16(const void* dy, int64_t lddy, const void* W, int64_t ldw, bool w_transposed, void* dx, int64_t lddx,
                                int dx_f32, int rows, int n_in, int k) {
    GemmBf16 g{};
    g.A = reinterpret_cast<const bf16_t*>(dy); g.lda = lddy; g.a_mode = OP_KC;
    g.B = reinterpret_cast<const bf16_t*>(W); g.ldb = ldw; g.b_mode = w_transposed ? OP_KC : OP_KS;
    g.C = dx; g.ldc = lddx; g.c_f32 = dx_f32;
    g.M = rows; g.N = n_in; g.K = k;
    g.split_k = 1;
    g.store_policy = store_policy_for((int64_t)rows * n_in * (dx_f32 ? 4 : 2));
    return g;
}

// fp32 dW [n_out][n_in]; the batch is the reduction extent, both operands k-strided
inline GemmBf16 wgrad_gemm_bf16(const void* dy, int64_t lddy, const void* x, int64_t ldx, void* dW, int rows, int n_out, int n_in) {
    GemmBf16 g{};
    g.A = reinterpret_cast<const bf16_t*>(dy); g.lda = lddy; g.a_mode = OP_KS;
    g.B = reinterpret_cast<const bf16_t*>(x); g.ldb = ldx; g.b_mode = OP_KS;
    g.C = dW; g.ldc = n_in; g.c_f32 = 1;
    g.M = n_out; g.N = n_in; g.K = rows;
    g.split_k = 1;
    g.store_policy = store_policy_for((int64_t)n_out * n_in * 4);
    return g;
}

// exact fp32: dense operands, no padding
inline GemmF32 fwd_gemm_f32(const float* x, const float* W, float* y, int rows, int n_out, int n_in, const float* bias) {
    GemmF32 g{};
    g.A = x; g.a_rs = n_in; g.a_ks = 1;
    g.B = W; g.b_rs = n_in; g.b_ks = 1;
    g.C = y; g.ldc = n_out;
    g.M = rows; g.N = n_out; g.K = n_in;
    g.bias = bias; g.split_k = 1;
    return g;
}

inline GemmF32 dgrad_gemm_f32(const float* dy, const float* W, float* dx, int rows, int n_out, int n_in) {
    GemmF32 g{};
    g.A = dy; g.a_rs = n_out; g.a_ks = 1;
    g.B = W; g.b_rs = 1; g.b_ks = n_in;
    g.C = dx; g.ldc = n_in;
    g.M = rows; g.N = n_in; g.K = n_out;
    g.split_k = 1;
    return g;
}

inline GemmF32 wgrad_gemm_f32(const float* dy, const float* x, float* dW, int rows, int n_out, int n_in) {
    GemmF32 g{};
    g.A = dy; g.a_rs = 1; g.a_ks = n_out;
    g.B = x; g.b_rs = 1; g.b_ks = n_in;
    g.C = dW; g.ldc = n_in;
    g.M = n_out; g.N = n_in; g.K = rows;
    g.split_k = 1;
    return g;
}

// relu: the ReLU code (clamp_below, 1-bit masks); act != CODAE_ACT_NONE: the generic-activation instantiation with parameters
// p[3] (null: zeros).  A data gradient passes relu = 0: its mask comes from relu_src.
template <typename G>
inline void set_activation(G& g, int relu, int act, const float* p) {
    g.relu = relu;
    g.act = act;
    for (int k = 0; k < 3; ++k) g.act_p[k] = p != nullptr ? p[k] : 0.f;
}

}  // namespace codae
