// Residual connections (codae_residual, include/codae_hip.h): two streaming kernels around the GEMMs of a skipped layer l.
//   forward   act[l + 1] <- rne(act[l + 1] + act[l])  behind the forward GEMM of layer l (and its dropout kernel); a training
//             forward first leaves the 1-bit mask "a_l > 0" of the value before the add - afterwards act[l + 1] holds h_{l+1},
//             from which the sign of a_l cannot be recovered
//   backward  behind the UNMASKED data-gradient GEMM of layer l, which left U_l in dA_{l-1}: G_l = U_l + G_{l+1} (fp32, kept in
//             the setting's work space), dA_{l-1} <- D_{l-1} = G_l * act'_{l-1}, + the column sums of the stored D
// Templates on <BF16, VEC> like the dropout kernels: 16 B per access where every row is 16-B aligned and the width is whole
// chunks, element accesses otherwise (the fp32 engine runs widths like 21 and 11); pad columns and pad rows are never written.
#include "codae_common.h"
#include "row_access.h"

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
// The row blocking, block shape and reduction of dropout_bwd_kernel: one block per 64 batch rows and all columns, 1024 threads, wave
// w owns rows 4 w .. 4 w + 3, its lanes 64 consecutive chunks (8 bf16 / 4 fp32 columns); a thread adds its four rows' STORED values
// in row order, the 16 waves' sums meet in LDS and are added in wave order by one thread per column: a fixed order, no atomics.
constexpr int BWD_ROWS = 64, BWD_WAVES = 16, BWD_NT = 64 * BWD_WAVES, BWD_ROWS_PER_WAVE = BWD_ROWS / BWD_WAVES;
enum { DERIV_NONE = 0, DERIV_BITS = 1, DERIV_SRC = 2 };

template <bool BF16, bool VEC>
constexpr int bwd_chunk_cols() { return (BF16 && VEC) ? 8 : 4; }

// G (fp32) columns [c, c + C) of a row, 0 past the width
template <bool VEC, int C>
__device__ __forceinline__ void load_g(const float* row, int c, int width, float* v) { load_work<false, VEC, C>(row, c, width, v); }

template <bool BF16, bool VEC>
__global__ __launch_bounds__(BWD_NT) void residual_bwd_kernel(void* d, int64_t ld, int B, int width, ResidualBwd r, int deriv,
                                                              float* __restrict__ colsum_part) {
    constexpr int C = bwd_chunk_cols<BF16, VEC>();
    constexpr int ES = BF16 ? 2 : 4;
    constexpr int TILE = 64 * C;                               // columns per tile
    __shared__ float red[BWD_WAVES][TILE];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row0 = blockIdx.x * BWD_ROWS + wave * BWD_ROWS_PER_WAVE;
    const bool selects = r.act_kind == CODAE_ACT_RELU;         // (ReLU selects 0 under a dead unit, every other kind multiplies)
    for (int t0 = 0; t0 < width; t0 += TILE) {
        const int c = t0 + lane * C;
        float sum[C];
#pragma unroll
        for (int k = 0; k < C; ++k) sum[k] = 0.f;
        if (c < width) {
#pragma unroll
            for (int i = 0; i < BWD_ROWS_PER_WAVE; ++i) {
                const int b = row0 + i;
                if (b < B) {
                    char* drow = reinterpret_cast<char*>(d) + (int64_t)b * ld * ES;
                    float g[C], out[C];
                    load_work<BF16, VEC, C>(drow, c, width, g);                       // U
                    if (r.g_in != nullptr) {
                        float gi[C];
                        load_g<VEC, C>(r.g_in + (int64_t)b * r.ld_g, c, width, gi);
#pragma unroll
                        for (int k = 0; k < C; ++k) g[k] = opaque(g[k] + gi[k]);
                    }
                    if (r.g_out != nullptr) {
                        float unused[C];
                        store_work<false, VEC, C>(r.g_out + (int64_t)b * r.ld_g, c, width, g, unused);
                    }
                    if (deriv == DERIV_BITS) {
                        const uint32_t m = (uint32_t)r.bits[(int64_t)b * r.ld_bits + (c >> 3)] >> (c & 7);
#pragma unroll
                        for (int k = 0; k < C; ++k)
                            g[k] = ((m >> k) & 1u) ? g[k] : (selects ? 0.f : opaque(g[k] * r.act_p[0]));
                    } else if (deriv == DERIV_SRC) {
                        float y[C];
                        load_work<BF16, VEC, C>(reinterpret_cast<const char*>(r.src) + (int64_t)b * r.ld_src * ES, c, width, y);
#pragma unroll
                        for (int k = 0; k < C; ++k)
                            g[k] = selects ? (positive_bit(y[k]) ? g[k] : 0.f) : act_bwd(r.act_kind, r.act_p, g[k], y[k]);
                    }
                    store_work<BF16, VEC, C>(drow, c, width, g, out);                 // D
#pragma unroll
                    for (int k = 0; k < C; ++k) sum[k] = opaque(sum[k] + out[k]);
                }
            }
        }
        if (colsum_part != nullptr) {                          // (block-uniform)
#pragma unroll
            for (int k = 0; k < C; ++k) red[wave][lane * C + k] = sum[k];
            __syncthreads();
            if (threadIdx.x < TILE && t0 + (int)threadIdx.x < width) {
                float s = red[0][threadIdx.x];
#pragma unroll
                for (int w = 1; w < BWD_WAVES; ++w) s = opaque(s + red[w][threadIdx.x]);
                colsum_part[(int64_t)blockIdx.x * width + t0 + threadIdx.x] = s;
            }
            __syncthreads();
        }
    }
}

}  // namespace

int launch_residual_fwd(void* y, const void* x, int bf16, int64_t ldy, int64_t ldx, int B, int width, uint8_t* bits, int64_t ld_bits,
                        hipStream_t s) {
    CODAE_REQUIRE(y != nullptr && x != nullptr && y != x, "codae_residual_fwd: null or aliased matrices");
    CODAE_REQUIRE(B > 0 && width > 0 && ldy >= width && ldx >= width, "codae_residual_fwd: B %d, width %d, ld %lld / %lld", B, width,
                  (long long)ldy, (long long)ldx);
    CODAE_REQUIRE(bits == nullptr || ld_bits >= (width + 7) / 8, "codae_residual_fwd: ld_bits %lld for %d columns", (long long)ld_bits, width);
    const int per = bf16 ? 8 : 4;
    const bool vec = aligned16(y) && aligned16(x) && ldy % per == 0 && ldx % per == 0 && width % per == 0;
    int64_t blocks = ((int64_t)B * ((width + FWD_C - 1) / FWD_C) + FWD_NT - 1) / FWD_NT;
    if (blocks > 2048) blocks = 2048;
#define RF(BF, V) hipLaunchKernelGGL((residual_fwd_kernel<BF, V>), dim3((unsigned)blocks), dim3(FWD_NT), 0, s, y, ldy, x, ldx, B, width, bits, ld_bits)
    if (bf16) { if (vec) RF(true, true); else RF(true, false); }
    else { if (vec) RF(false, true); else RF(false, false); }
#undef RF
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_residual_bwd(void* d, int bf16, int64_t ld, int B, int width, const ResidualBwd& r, float* colsum_part, hipStream_t s) {
    CODAE_REQUIRE(d != nullptr, "codae_residual_bwd: null matrix");
    CODAE_REQUIRE(B > 0 && width > 0 && ld >= width, "codae_residual_bwd: B %d, width %d, ld %lld", B, width, (long long)ld);
    CODAE_REQUIRE((r.g_in == nullptr && r.g_out == nullptr) || r.ld_g >= width, "codae_residual_bwd: ld_g %lld for %d columns", (long long)r.ld_g, width);
    CODAE_REQUIRE(r.bits == nullptr || r.src == nullptr, "codae_residual_bwd: the derivative comes from the bits or from the saved activation, not both");
    CODAE_REQUIRE(r.bits == nullptr || r.ld_bits >= (width + 7) / 8, "codae_residual_bwd: ld_bits %lld for %d columns", (long long)r.ld_bits, width);
    CODAE_REQUIRE(r.bits == nullptr || r.act_kind == CODAE_ACT_RELU || r.act_kind == CODAE_ACT_LEAKY,
                  "codae_residual_bwd: 1-bit masks carry the derivative of ReLU and LeakyReLU only (kind %d)", r.act_kind);
    CODAE_REQUIRE(r.src == nullptr || (r.ld_src >= width && r.act_kind >= CODAE_ACT_NONE && r.act_kind <= CODAE_ACT_HARDSIGMOID),
                  "codae_residual_bwd: ld_src %lld, activation kind %d", (long long)r.ld_src, r.act_kind);
    const int deriv = r.bits != nullptr ? DERIV_BITS : (r.src != nullptr && r.act_kind != CODAE_ACT_NONE ? DERIV_SRC : DERIV_NONE);
    const int per = bf16 ? 8 : 4;
    bool vec = aligned16(d) && ld % per == 0 && width % per == 0;
    if (r.g_in != nullptr || r.g_out != nullptr) vec = vec && aligned16(r.g_in) && aligned16(r.g_out) && r.ld_g % 4 == 0;
    if (deriv == DERIV_SRC) vec = vec && aligned16(r.src) && r.ld_src % per == 0;
    const int blocks = residual_blocks(B);
#define RB(BF, V) hipLaunchKernelGGL((residual_bwd_kernel<BF, V>), dim3(blocks), dim3(BWD_NT), 0, s, d, ld, B, width, r, deriv, colsum_part)
    if (bf16) { if (vec) RB(true, true); else RB(true, false); }
    else { if (vec) RB(false, true); else RB(false, false); }
#undef RB
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

}  // namespace codae
