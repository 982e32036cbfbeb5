// Sparse code (codae_sparse_code, include/codae_hip.h): two in-place streaming kernels around the GEMMs of the layer m that produces
// the code.
//   forward   behind the forward GEMM of layer m (and its dropout kernel): per batch row the `keep` columns that rank first by
//             (key descending, column ascending) keep their bits, every other column is stored as +0; a training forward also
//             leaves the 1-bit keep mask
//   backward  behind the data-gradient GEMM that produced dA_m (and the residual kernel of a skip around the layer that reads the
//             code): dA_m <- kept ? dA_m : +0 - a SELECTION, a NaN gradient under a dropped column becomes +0 -, + the column sums of
//             the stored values: the sweep of row_sweep.h, the shape of dropout's backward
// key(v) = the stored bits with the sign cleared, read as an unsigned integer (15 bits of a bf16, 31 of an fp32): -0 and +0 tie, Inf
// ranks above every finite value and every NaN above Inf.  Both kernels move BITS, never floats: what is kept is kept exactly.
// The forward kernel is a radix select, a wave per row: per 8-bit digit from the top, the wave counts the keys that share the
// prefix found so far into its own 256-bin histogram in LDS (integer atomics: counts, so deterministic), and a prefix count over
// the bins in descending order names the digit that holds the keep-th key.  2 passes for bf16, 4 for fp32, then the write-out;
// the row is RE-READ per pass as norm.hip re-reads it - any width, no register cliff; the passes after the first hit the caches.
// Ties at the threshold key go to the lowest columns: a wave prefix count of the equal keys in column order.
#include "codae_common.h"
#include "row_sweep.h"

namespace codae {
namespace {

// A lane owns 8 columns per chunk whatever the type - one 16-B access of bf16, two of fp32: exactly one mask byte, so no two
// lanes share a byte of the mask.
constexpr int NC = 8;

// the raw bits of columns [c, c + 8) of a working-precision row (a bf16 in the low half); returns the mask of the columns that lie
// inside the width - the others are not read and give 0
template <bool BF16, bool VEC>
__device__ __forceinline__ uint32_t load_bits8(const void* row, int c, int width, uint32_t* u) {
    uint32_t vm = 0;
    if constexpr (BF16 && VEC) {
        const uint4 q = *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16_t*>(row) + c);
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) { u[2 * k] = w[k] & 0xffffu; u[2 * k + 1] = w[k] >> 16; }
        vm = 0xffu;
    } else if constexpr (VEC) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            uint4 f = make_uint4(0u, 0u, 0u, 0u);
            if (c + 4 * q < width) {
                f = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint32_t*>(row) + c + 4 * q);
                vm |= 0xfu << (4 * q);
            }
            u[4 * q] = f.x; u[4 * q + 1] = f.y; u[4 * q + 2] = f.z; u[4 * q + 3] = f.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            u[k] = 0u;
            if (c + k < width) {
                if constexpr (BF16) u[k] = reinterpret_cast<const bf16_t*>(row)[c + k];
                else u[k] = reinterpret_cast<const uint32_t*>(row)[c + k];
                vm |= 1u << k;
            }
        }
    }
    return vm;
}

// columns [c, c + 8) <- u where `touched` says a column changed: a 16-B access that holds a touched column is written whole (its
// other columns with the bits they were read with), an element access only where touched; `touched` lies inside the width
template <bool BF16, bool VEC>
__device__ __forceinline__ void store_bits8(void* row, int c, const uint32_t* u, uint32_t touched) {
    if constexpr (BF16 && VEC) {
        if (touched)
            *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(row) + c) =
                make_uint4(u[0] | (u[1] << 16), u[2] | (u[3] << 16), u[4] | (u[5] << 16), u[6] | (u[7] << 16));
    } else if constexpr (VEC) {
#pragma unroll
        for (int q = 0; q < 2; ++q)
            if ((touched >> (4 * q)) & 0xfu)
                *reinterpret_cast<uint4*>(reinterpret_cast<uint32_t*>(row) + c + 4 * q) = make_uint4(u[4 * q], u[4 * q + 1], u[4 * q + 2], u[4 * q + 3]);
    } else {
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            if ((touched >> k) & 1u) {
                if constexpr (BF16) reinterpret_cast<bf16_t*>(row)[c + k] = (bf16_t)u[k];
                else reinterpret_cast<uint32_t*>(row)[c + k] = u[k];
            }
        }
    }
}

// the wave's exclusive prefix count of v in lane order; *total = the count of all 64 lanes (the same in every lane)
__device__ __forceinline__ int wave_prefix_count(int v, int lane, int* total) {
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    *total = __shfl(inc, 63, 64);
    return inc - v;
}

// ---- forward ----------------------------------------------------------------------------------------------------------------
// 4 waves per block, a wave per row as norm_fwd_kernel; the row loop is BLOCK-uniform (a wave past the last row idles through the
// barriers that separate the clearing, the counting and the reading of the histograms).
constexpr int FWD_WAVES = 4, FWD_NT = 64 * FWD_WAVES, BINS = 256;

template <bool BF16, bool VEC>
__global__ __launch_bounds__(FWD_NT) void sparse_code_fwd_kernel(void* __restrict__ y, int64_t ld, int B, int width, int keep,
                                                                 uint8_t* __restrict__ bits, int64_t ld_bits) {
    constexpr int ES = BF16 ? 2 : 4;
    constexpr int PASSES = BF16 ? 2 : 4;                       // 7 + 8 bits, or 7 + 8 + 8 + 8
    constexpr uint32_t KEY = BF16 ? 0x7fffu : 0x7fffffffu;
    __shared__ uint32_t hist[FWD_WAVES][BINS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t* const h = hist[wave];
    for (int b0 = blockIdx.x * FWD_WAVES; b0 < B; b0 += gridDim.x * FWD_WAVES) {
        const int b = b0 + wave;
        const bool active = b < B;                             // (wave-uniform)
        char* row = reinterpret_cast<char*>(y) + (int64_t)(active ? b : 0) * ld * ES;
        // the threshold key, digit by digit: `prefix` = its digits so far, `need` = how many of the keys that share them are kept
        uint32_t prefix = 0;
        int need = keep;
#pragma unroll
        for (int pass = 0; pass < PASSES; ++pass) {
            const int shift = 8 * (PASSES - 1 - pass);
            // a lane clears the four bins it reads below: bins 255 - 4 lane - j, the highest digits in lane 0
#pragma unroll
            for (int j = 0; j < 4; ++j) h[BINS - 1 - 4 * lane - j] = 0u;
            __syncthreads();
            if (active) {
                for (int c = lane * NC; c < width; c += 64 * NC) {
                    uint32_t u[NC];
                    const uint32_t vm = load_bits8<BF16, VEC>(row, c, width, u);
#pragma unroll
                    for (int k = 0; k < NC; ++k) {
                        const uint32_t key = u[k] & KEY;
                        if (((vm >> k) & 1u) && (pass == 0 || (uint32_t)((uint64_t)key >> (shift + 8)) == prefix))
                            atomicAdd(&h[(key >> shift) & 0xffu], 1u);
                    }
                }
            }
            __syncthreads();
            if (active) {
                int cnt[4], mine = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) { cnt[j] = (int)h[BINS - 1 - 4 * lane - j]; mine += cnt[j]; }
                int total;
                const int before = wave_prefix_count(mine, lane, &total);
                // exactly one lane holds the need-th key in descending order (1 <= need <= total: keep <= width)
                const bool found = need > before && need <= before + mine;
                int digit = 0, left = need;
                if (found) {
                    int acc = before;
                    bool done = false;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (!done && need <= acc + cnt[j]) { digit = BINS - 1 - 4 * lane - j; left = need - acc; done = true; }
                        acc += cnt[j];
                    }
                }
                const unsigned long long who = __ballot(found);
                const int src = who ? __ffsll((long long)who) - 1 : 0;
                digit = __shfl(digit, src, 64);
                need = __shfl(left, src, 64);
                prefix = (prefix << 8) | (uint32_t)digit;
            }
        }
        if (!active) continue;
        // write-out: keys above the threshold are kept, of those equal to it the first `need` in column order
        int seen = 0;                                          // equal keys in the tiles before this one (wave-uniform)
        for (int c0 = 0; c0 < width; c0 += 64 * NC) {          // (wave-uniform trips: the prefix count needs every lane)
            const int c = c0 + lane * NC;
            uint32_t u[NC], vm = 0u, above = 0u, equal = 0u;
            if (c < width) vm = load_bits8<BF16, VEC>(row, c, width, u);
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                if ((vm >> k) & 1u) {
                    const uint32_t key = u[k] & KEY;
                    above |= (key > prefix ? 1u : 0u) << k;
                    equal |= (key == prefix ? 1u : 0u) << k;
                }
            }
            int total;
            int rank = seen + wave_prefix_count(__popc(equal), lane, &total);
            seen += total;
            uint32_t kept = above;
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                if ((equal >> k) & 1u) {
                    if (rank < need) kept |= 1u << k;
                    ++rank;
                }
            }
            if (c < width) {
                const uint32_t dropped = vm & ~kept;
#pragma unroll
                for (int k = 0; k < NC; ++k)
                    if ((dropped >> k) & 1u) u[k] = 0u;        // +0
                store_bits8<BF16, VEC>(row, c, u, dropped);
                if (bits != nullptr) bits[(int64_t)b * ld_bits + (c >> 3)] = (uint8_t)kept;     // (bits past the width: clear)
            }
        }
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
// The shared sweep (row_sweep.h), 8 columns per chunk whatever the type: one mask byte.
template <bool BF16, bool VEC>
__global__ __launch_bounds__(SWEEP_NT) void sparse_code_bwd_kernel(void* __restrict__ d, int64_t ld, int B, int width,
                                                                   const uint8_t* __restrict__ bits, int64_t ld_bits,
                                                                   float* __restrict__ colsum_part) {
    constexpr int ES = BF16 ? 2 : 4;
    row_sweep<NC>(B, width, colsum_part, [=](int b, int i, int c, float* out) {
        char* drow = reinterpret_cast<char*>(d) + (int64_t)b * ld * ES;
        uint32_t u[NC];
        const uint32_t vm = load_bits8<BF16, VEC>(drow, c, width, u);
        const uint32_t dropped = vm & ~(uint32_t)bits[(int64_t)b * ld_bits + (c >> 3)];
#pragma unroll
        for (int k = 0; k < NC; ++k)
            if ((dropped >> k) & 1u) u[k] = 0u;                // +0, whatever the gradient held
        store_bits8<BF16, VEC>(drow, c, u, dropped);
#pragma unroll
        for (int k = 0; k < NC; ++k) out[k] = __uint_as_float(BF16 ? u[k] << 16 : u[k]);      // (a column past the width: 0)
    });
}

}  // namespace

int launch_sparse_code_fwd(void* y, int bf16, int64_t ld, int B, int width, int keep, uint8_t* bits, int64_t ld_bits, hipStream_t s) {
    CODAE_REQUIRE(y != nullptr, "codae_sparse_code_fwd: null matrix");
    CODAE_REQUIRE(B > 0 && width > 0 && ld >= width, "codae_sparse_code_fwd: B %d, width %d, ld %lld", B, width, (long long)ld);
    CODAE_REQUIRE(keep >= 1 && keep <= width, "codae_sparse_code_fwd: keep %d outside [1, %d]", keep, width);
    CODAE_REQUIRE(bits == nullptr || ld_bits >= (width + 7) / 8, "codae_sparse_code_fwd: ld_bits %lld for %d columns", (long long)ld_bits, width);
    int blocks = (B + FWD_WAVES - 1) / FWD_WAVES;
    if (blocks > 4096) blocks = 4096;
    dispatch_bf16_vec(bf16, rows_vec16(bf16, width, {{y, ld}}), [&](auto BF, auto V) {
        hipLaunchKernelGGL((sparse_code_fwd_kernel<decltype(BF)::value, decltype(V)::value>), dim3(blocks), dim3(FWD_NT), 0, s, y, ld, B, width,
                           keep, bits, ld_bits);
    });
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_sparse_code_bwd(void* d, int bf16, int64_t ld, int B, int width, const uint8_t* bits, int64_t ld_bits, float* colsum_part,
                           hipStream_t s) {
    CODAE_REQUIRE(d != nullptr && bits != nullptr, "codae_sparse_code_bwd: null matrix or bits");
    CODAE_REQUIRE(B > 0 && width > 0 && ld >= width, "codae_sparse_code_bwd: B %d, width %d, ld %lld", B, width, (long long)ld);
    CODAE_REQUIRE(ld_bits >= (width + 7) / 8, "codae_sparse_code_bwd: ld_bits %lld for %d columns", (long long)ld_bits, width);
    dispatch_bf16_vec(bf16, rows_vec16(bf16, width, {{d, ld}}), [&](auto BF, auto V) {
        hipLaunchKernelGGL((sparse_code_bwd_kernel<decltype(BF)::value, decltype(V)::value>), dim3(row_sweep_blocks(B)), dim3(SWEEP_NT), 0, s, d,
                           ld, B, width, bits, ld_bits, colsum_part);
    });
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

}  // namespace codae
