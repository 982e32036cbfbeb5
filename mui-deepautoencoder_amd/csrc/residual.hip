// Residual connections (codae_residual, include/codae_hip.h): two streaming kernels around the GEMMs of a skipped layer l.
//   forward   act[l + 1] <- rne(act[l + 1] + act[l])  behind the forward GEMM of layer l (and its dropout kernel); a training
//             forward first leaves the 1-bit mask "a_l > 0" of the value before the add - afterwards act[l + 1] holds h_{l+1},
//             from which the sign of a_l cannot be recovered
//   backward  behind the UNMASKED data-gradient GEMM of layer l, which left U_l in dA_{l-1}: G_l = U_l + G_{l+1} (fp32, kept in
//             the setting's work space), dA_{l-1} <- D_{l-1} = G_l * act'_{l-1}, + the column sums of the stored D: the sweep of
//             row_sweep.h
// Templates on <BF16, VEC> like the dropout kernels: 16 B per access where every row is 16-B aligned and the width is whole
// chunks, element accesses otherwise (the fp32 engine runs widths like 21 and 11); pad columns and pad rows are never written.
#include "codae_common.h"
#include "row_sweep.h"

namespace codae {
namespace {

// ---- forward ----------------------------------------------------------------------------------------------------------------
// Block shape and grid cap of dropout_fwd_kernel (256 threads, at most 2048 blocks, grid-stride loop).  A thread owns 8 columns
// whatever the type - one 16-B access of bf16, two of fp32 - so its chunk is exactly one mask byte and no two threads share one.
constexpr int FWD_NT = 256, FWD_C = 8;

template <bool BF16, bool VEC>
__global__ __launch_bounds__(FWD_NT) void residual_fwd_kernel(void* __restrict__ y, int64_t ldy, const void* __restrict__ x, int64_t ldx, int B,
                                                              int width, uint8_t* __restrict__ bits, int64_t ld_bits) {
    constexpr int ES = BF16 ? 2 : 4;
    const int chunks = (width + FWD_C - 1) / FWD_C;
    const int64_t total = (int64_t)B * chunks;
    for (int64_t e = (int64_t)blockIdx.x * FWD_NT + threadIdx.x; e < total; e += (int64_t)gridDim.x * FWD_NT) {
        const int b = (int)(e / chunks);
        const int c = (int)(e - (int64_t)b * chunks) * FWD_C;
        char* yrow = reinterpret_cast<char*>(y) + (int64_t)b * ldy * ES;
        const char* xrow = reinterpret_cast<const char*>(x) + (int64_t)b * ldx * ES;
        float a[FWD_C], h[FWD_C], out[FWD_C];
        load_work<BF16, VEC, FWD_C>(yrow, c, width, a);
        load_work<BF16, VEC, FWD_C>(xrow, c, width, h);
        uint32_t m = 0;
#pragma unroll
        for (int k = 0; k < FWD_C; ++k) {
            m |= positive_bit(a[k]) << k;              // (a column past the width was loaded as +0: bit clear)
            a[k] = opaque(a[k] + h[k]);
        }
        store_work<BF16, VEC, FWD_C>(yrow, c, width, a, out);
        if (bits != nullptr) bits[(int64_t)b * ld_bits + (c >> 3)] = (uint8_t)m;
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
// The shared sweep (row_sweep.h), no prologue; a chunk is 8 bf16 / 4 fp32 columns.
enum { DERIV_NONE = 0, DERIV_BITS = 1, DERIV_SRC = 2 };

template <bool BF16, bool VEC>
__global__ __launch_bounds__(SWEEP_NT) void residual_bwd_kernel(void* d, int64_t ld, int B, int width, ResidualBwd r, int deriv,
                                                                float* __restrict__ colsum_part) {
    constexpr int C = access_cols<BF16, VEC>();
    constexpr int ES = BF16 ? 2 : 4;
    const bool selects = r.act_kind == CODAE_ACT_RELU;         // (ReLU selects 0 under a dead unit, every other kind multiplies)
    row_sweep<C>(B, width, colsum_part, [=](int b, int, int c, float* out) {
        char* drow = reinterpret_cast<char*>(d) + (int64_t)b * ld * ES;
        float g[C];
        load_gh<BF16, VEC, C>(drow, r, b, c, width, g);                   // G = U + g_in
        store_g<VEC, C>(r, b, c, width, g);
        if (deriv == DERIV_BITS) {
            mask_deriv<C>(r, b, c, g);
        } else if (deriv == DERIV_SRC) {
            float y[C];
            load_work<BF16, VEC, C>(reinterpret_cast<const char*>(r.src) + (int64_t)b * r.ld_src * ES, c, width, y);
#pragma unroll
            for (int k = 0; k < C; ++k) g[k] = selects ? (positive_bit(y[k]) ? g[k] : 0.f) : act_bwd(r.act_kind, r.act_p, g[k], y[k]);
        }
        store_work<BF16, VEC, C>(drow, c, width, g, out);                 // D
    });
}

}  // namespace

int launch_residual_fwd(void* y, const void* x, int bf16, int64_t ldy, int64_t ldx, int B, int width, uint8_t* bits, int64_t ld_bits,
                        hipStream_t s) {
    CODAE_REQUIRE(y != nullptr && x != nullptr && y != x, "codae_residual_fwd: null or aliased matrices");
    CODAE_REQUIRE(B > 0 && width > 0 && ldy >= width && ldx >= width, "codae_residual_fwd: B %d, width %d, ld %lld / %lld", B, width,
                  (long long)ldy, (long long)ldx);
    CODAE_REQUIRE(bits == nullptr || ld_bits >= (width + 7) / 8, "codae_residual_fwd: ld_bits %lld for %d columns", (long long)ld_bits, width);
    int64_t blocks = ((int64_t)B * ((width + FWD_C - 1) / FWD_C) + FWD_NT - 1) / FWD_NT;
    if (blocks > 2048) blocks = 2048;
    dispatch_bf16_vec(bf16, rows_vec16(bf16, width, {{y, ldy}, {x, ldx}}), [&](auto BF, auto V) {
        hipLaunchKernelGGL((residual_fwd_kernel<decltype(BF)::value, decltype(V)::value>), dim3((unsigned)blocks), dim3(FWD_NT), 0, s, y, ldy, x,
                           ldx, B, width, bits, ld_bits);
    });
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_residual_bwd(void* d, int bf16, int64_t ld, int B, int width, const ResidualBwd& r, float* colsum_part, hipStream_t s) {
    CODAE_REQUIRE(d != nullptr, "codae_residual_bwd: null matrix");
    CODAE_REQUIRE(B > 0 && width > 0 && ld >= width, "codae_residual_bwd: B %d, width %d, ld %lld", B, width, (long long)ld);
    CODAE_REQUIRE(r.bits == nullptr || r.src == nullptr, "codae_residual_bwd: the derivative comes from the bits or from the saved activation, not both");
    int rc = check_stream_bwd("codae_residual_bwd", r, width);
    if (rc) return rc;
    CODAE_REQUIRE(r.src == nullptr || (r.ld_src >= width && r.act_kind >= CODAE_ACT_NONE && r.act_kind <= CODAE_ACT_HARDSIGMOID),
                  "codae_residual_bwd: ld_src %lld, activation kind %d", (long long)r.ld_src, r.act_kind);
    const int deriv = r.bits != nullptr ? DERIV_BITS : (r.src != nullptr && r.act_kind != CODAE_ACT_NONE ? DERIV_SRC : DERIV_NONE);
    const bool vec = deriv == DERIV_SRC ? rows_vec16(bf16, width, {{d, ld}, {r.src, r.ld_src}}, &r) : rows_vec16(bf16, width, {{d, ld}}, &r);
    dispatch_bf16_vec(bf16, vec, [&](auto BF, auto V) {
        hipLaunchKernelGGL((residual_bwd_kernel<decltype(BF)::value, decltype(V)::value>), dim3(row_sweep_blocks(B)), dim3(SWEEP_NT), 0, s, d, ld,
                           B, width, r, deriv, colsum_part);
    });
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

}  // namespace codae
