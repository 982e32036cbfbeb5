// Normalisation (codae_norm, include/codae_hip.h): two streaming kernels around the GEMMs of a normalised layer l; a wave owns a row.
//   forward   behind the forward GEMM of layer l (and its dropout and skip kernels): the row statistics in fp32 from the stored
//             values, act[l + 1] <- rne(xhat) in place, r[b]; a training forward of a ReLU / LeakyReLU layer without a skip first
//             leaves the 1-bit mask "value > 0" of what it read - afterwards act[l + 1] holds xhat, whose sign says nothing
//   backward  behind the UNMASKED data-gradient GEMM of layer l + 1, which left U in dA_l: Gh = U + G (iff layer l + 1 is skipped),
//             the row reductions c1, c2 against xhat = act[l + 1] and r, Gs = r (Gh - c1 - xhat c2), G <- Gs (iff layer l is
//             skipped), dA_l <- D_l = Gs * act'_l, + the column sums of the stored D: the residual backward kernel's whole job,
//             in the same sweep (row_sweep.h)
// The row is RE-READ, not kept in registers: one code path for every width (the fp32 engine runs 21 and 11, the headline 1536, and
// nothing bounds it), no register-count cliff and no scratch; a wave re-reads only what it read itself a pass earlier, 3 KB per bf16
// row at the headline width, which the passes after the first find in the caches - HBM sees every matrix once.
// Templates on <BF16, VEC, KIND>: 16 B per access where every row is 16-B aligned and the width is whole chunks, element accesses
// otherwise; pad columns and pad rows are never written (xhat of a zero pad column would be -mu r, and the next GEMM's k runs over it).
#include "codae_common.h"
#include "row_sweep.h"

namespace codae {
namespace {

// A lane owns 8 columns per chunk whatever the type - one 16-B access of bf16, two of fp32: exactly one mask byte.
constexpr int NC = 8;

// ---- forward ----------------------------------------------------------------------------------------------------------------
constexpr int FWD_WAVES = 4, FWD_NT = 64 * FWD_WAVES;

template <bool BF16, bool VEC, int KIND>
__global__ __launch_bounds__(FWD_NT) void norm_fwd_kernel(void* __restrict__ y, int64_t ld, int B, int width, float eps,
                                                          float* __restrict__ rstd, uint8_t* __restrict__ bits, int64_t ld_bits) {
    constexpr int ES = BF16 ? 2 : 4;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float w = (float)width;
    for (int b = blockIdx.x * FWD_WAVES + wave; b < B; b += gridDim.x * FWD_WAVES) {
        char* row = reinterpret_cast<char*>(y) + (int64_t)b * ld * ES;
        // pass 1: sum x (layer) or sum x^2 (rms), a lane's columns in ascending order; the mask of what was read
        float s = 0.f;
        for (int c = lane * NC; c < width; c += 64 * NC) {
            float x[NC];
            load_work<BF16, VEC, NC>(row, c, width, x);
            uint32_t m = 0;
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                m |= positive_bit(x[k]) << k;                  // (a column past the width was loaded as +0: bit clear)
                s = (KIND == CODAE_NORM_LAYER) ? opaque(s + x[k]) : opaque(s + opaque(x[k] * x[k]));
            }
            if (bits != nullptr) bits[(int64_t)b * ld_bits + (c >> 3)] = (uint8_t)m;
        }
        s = wave_sum(s);
        float mu = 0.f;
        if constexpr (KIND == CODAE_NORM_LAYER) {
            // pass 2: the centred squares (a column past the width would add mu^2: left out)
            mu = s / w;
            s = 0.f;
            for (int c = lane * NC; c < width; c += 64 * NC) {
                float x[NC];
                load_work<BF16, VEC, NC>(row, c, width, x);
#pragma unroll
                for (int k = 0; k < NC; ++k) {
                    const float dlt = opaque(x[k] - mu);
                    if (c + k < width) s = opaque(s + opaque(dlt * dlt));
                }
            }
            s = wave_sum(s);
        }
        const float r = 1.f / sqrtf(opaque(s / w) + eps);
        // pass 3: xhat in place
        for (int c = lane * NC; c < width; c += 64 * NC) {
            float x[NC], out[NC];
            load_work<BF16, VEC, NC>(row, c, width, x);
#pragma unroll
            for (int k = 0; k < NC; ++k) x[k] = (KIND == CODAE_NORM_LAYER) ? opaque(x[k] - mu) * r : x[k] * r;
            store_work<BF16, VEC, NC>(row, c, width, x, out);
        }
        if (lane == 0) rstd[b] = r;
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
// The shared sweep (row_sweep.h) behind a prologue: the row reductions c1, c2 of the wave's four rows, a wave per row as in the
// forward.  The sweep's chunk then re-reads Gh - the bits the reductions saw - and writes Gs and D, 8 columns whatever the type.
template <bool BF16, bool VEC, int KIND>
__global__ __launch_bounds__(SWEEP_NT) void norm_bwd_kernel(void* d, int64_t ld, int B, int width, NormBwd n, float* __restrict__ colsum_part) {
    constexpr int ES = BF16 ? 2 : 4;
    const int lane = threadIdx.x & 63;
    const int row0 = sweep_row0();
    const float w = (float)width;
    float c1[SWEEP_RPW], c2[SWEEP_RPW], r[SWEEP_RPW];
#pragma unroll
    for (int i = 0; i < SWEEP_RPW; ++i) {
        const int b = row0 + i;
        c1[i] = 0.f; c2[i] = 0.f; r[i] = 0.f;
        if (b < B) {                                           // (wave-uniform)
            const char* drow = reinterpret_cast<const char*>(d) + (int64_t)b * ld * ES;
            const char* xrow = reinterpret_cast<const char*>(n.xhat) + (int64_t)b * n.ld_x * ES;
            float s1 = 0.f, s2 = 0.f;
            for (int c = lane * NC; c < width; c += 64 * NC) {
                float g[NC], xh[NC];
                load_gh<BF16, VEC, NC>(drow, n, b, c, width, g);
                load_work<BF16, VEC, NC>(xrow, c, width, xh);
#pragma unroll
                for (int k = 0; k < NC; ++k) {                 // (a column past the width was loaded as 0 in both)
                    if constexpr (KIND == CODAE_NORM_LAYER) s1 = opaque(s1 + g[k]);
                    s2 = opaque(s2 + opaque(g[k] * xh[k]));
                }
            }
            if constexpr (KIND == CODAE_NORM_LAYER) c1[i] = wave_sum(s1) / w;
            c2[i] = wave_sum(s2) / w;
            r[i] = n.rstd[b];
        }
    }
    row_sweep<NC>(B, width, colsum_part, [=](int b, int i, int c, float* out) {
        char* drow = reinterpret_cast<char*>(d) + (int64_t)b * ld * ES;
        float g[NC], xh[NC];
        load_gh<BF16, VEC, NC>(drow, n, b, c, width, g);
        load_work<BF16, VEC, NC>(reinterpret_cast<const char*>(n.xhat) + (int64_t)b * n.ld_x * ES, c, width, xh);
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            float t = opaque(g[k] - opaque(xh[k] * c2[i]));
            if constexpr (KIND == CODAE_NORM_LAYER) t = opaque(t - c1[i]);
            g[k] = opaque(t * r[i]);                                      // Gs
        }
        store_g<VEC, NC>(n, b, c, width, g);
        if (n.bits != nullptr) mask_deriv<NC>(n, b, c, g);
        store_work<BF16, VEC, NC>(drow, c, width, g, out);                // D
    });
}

// launch(BF16, VEC, KIND) as integral constants: dispatch_bf16_vec and the norm's kind
template <class Launch>
void dispatch_norm(int bf16, bool vec, int kind, Launch launch) {
    dispatch_bf16_vec(bf16, vec, [&](auto BF, auto V) {
        if (kind == CODAE_NORM_LAYER) launch(BF, V, std::integral_constant<int, CODAE_NORM_LAYER>{});
        else launch(BF, V, std::integral_constant<int, CODAE_NORM_RMS>{});
    });
}

}  // namespace

int launch_norm_fwd(void* y, int bf16, int64_t ld, int B, int width, int kind, float eps, float* rstd, uint8_t* bits, int64_t ld_bits,
                    hipStream_t s) {
    CODAE_REQUIRE(y != nullptr && rstd != nullptr, "codae_norm_fwd: null matrix or rstd");
    CODAE_REQUIRE(B > 0 && width > 0 && ld >= width, "codae_norm_fwd: B %d, width %d, ld %lld", B, width, (long long)ld);
    CODAE_REQUIRE(kind == CODAE_NORM_LAYER || kind == CODAE_NORM_RMS, "codae_norm_fwd: kind %d is neither CODAE_NORM_LAYER nor CODAE_NORM_RMS", kind);
    CODAE_REQUIRE(eps > 0.f && eps <= 3.402823466e38f, "codae_norm_fwd: eps %g must be finite and > 0", (double)eps);
    CODAE_REQUIRE(bits == nullptr || ld_bits >= (width + 7) / 8, "codae_norm_fwd: ld_bits %lld for %d columns", (long long)ld_bits, width);
    int blocks = (B + FWD_WAVES - 1) / FWD_WAVES;
    if (blocks > 4096) blocks = 4096;
    dispatch_norm(bf16, rows_vec16(bf16, width, {{y, ld}}), kind, [&](auto BF, auto V, auto K) {
        hipLaunchKernelGGL((norm_fwd_kernel<decltype(BF)::value, decltype(V)::value, decltype(K)::value>), dim3(blocks), dim3(FWD_NT), 0, s, y, ld,
                           B, width, eps, rstd, bits, ld_bits);
    });
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_norm_bwd(void* d, int bf16, int64_t ld, int B, int width, int kind, const NormBwd& n, float* colsum_part, hipStream_t s) {
    CODAE_REQUIRE(d != nullptr && n.xhat != nullptr && n.rstd != nullptr && d != n.xhat, "codae_norm_bwd: null or aliased matrix, xhat or rstd");
    CODAE_REQUIRE(B > 0 && width > 0 && ld >= width && n.ld_x >= width, "codae_norm_bwd: B %d, width %d, ld %lld, ld_x %lld", B, width,
                  (long long)ld, (long long)n.ld_x);
    CODAE_REQUIRE(kind == CODAE_NORM_LAYER || kind == CODAE_NORM_RMS, "codae_norm_bwd: kind %d is neither CODAE_NORM_LAYER nor CODAE_NORM_RMS", kind);
    int rc = check_stream_bwd("codae_norm_bwd", n, width);
    if (rc) return rc;
    dispatch_norm(bf16, rows_vec16(bf16, width, {{d, ld}, {n.xhat, n.ld_x}}, &n), kind, [&](auto BF, auto V, auto K) {
        hipLaunchKernelGGL((norm_bwd_kernel<decltype(BF)::value, decltype(V)::value, decltype(K)::value>), dim3(row_sweep_blocks(B)),
                           dim3(SWEEP_NT), 0, s, d, ld, B, width, n, colsum_part);
    });
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

}  // namespace codae
