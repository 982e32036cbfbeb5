// State digest (include/codae_hip.h, "State digest"): one pass over a buffer that hashes every 16-byte group and, when asked, stores
// it to a second buffer on the way - the snapshot copy of a checkpoint.  Integer arithmetic only: the per-group hashes are combined
// by a 64-bit sum and a 64-bit xor, both associative and commutative, so lanes, waves and workgroups may combine in any order and the
// result has the same bits every run.  This is why integer atomics are allowed here and nowhere in the training step.
#include "codae_common.h"

namespace codae {
namespace {

constexpr uint64_t DG_G = 0x9E3779B97F4A7C15ull;

__host__ __device__ __forceinline__ uint64_t dg_mix(uint64_t x) {
    uint64_t z = x + DG_G;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ void dg_group(u32x4 w, uint64_t g, uint64_t& sum, uint64_t& xr) {
    const uint64_t a = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
    const uint64_t b = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
    const uint64_t h = dg_mix(a ^ dg_mix(b + g * DG_G));
    sum += h;
    xr ^= dg_mix(h ^ g);
}

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int lane_mask) {
    const uint32_t lo = __shfl_xor((uint32_t)v, lane_mask, 64), hi = __shfl_xor((uint32_t)(v >> 32), lane_mask, 64);
    return (uint64_t)lo | ((uint64_t)hi << 32);
}

constexpr int DG_UNROLL = 4;     // 16-byte loads a lane has in flight before it hashes the first

// VEC: src (and dst) 16-byte aligned - one 16-byte load (and store) per group; else four dword accesses per group.
// COPY: every group is stored to dst as it is read.  FINAL: the launch is one workgroup, which writes out[] itself; else every
// workgroup adds / xors its pair into the zeroed out[] and digest_finish_kernel folds the length in.
// Words at and beyond n_words are never read or written: the last, partial group is padded with zeros in registers.
template <bool VEC, bool COPY, bool FINAL>
__global__ __launch_bounds__(GRID_NT) void state_digest_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int64_t n_words,
                                                               uint64_t len_mix, unsigned long long* __restrict__ out) {
    const int64_t n_full = n_words >> 2;                       // whole groups
    const int64_t stride = (int64_t)gridDim.x * GRID_NT;
    uint64_t sum = 0, xr = 0;
    int64_t g = (int64_t)blockIdx.x * GRID_NT + threadIdx.x;
    if (VEC) {
        const u32x4* s4 = reinterpret_cast<const u32x4*>(src);
        u32x4* d4 = reinterpret_cast<u32x4*>(dst);
        for (; g + (DG_UNROLL - 1) * stride < n_full; g += DG_UNROLL * stride) {
            u32x4 w[DG_UNROLL];
#pragma unroll
            for (int u = 0; u < DG_UNROLL; ++u) w[u] = s4[g + u * stride];
#pragma unroll
            for (int u = 0; u < DG_UNROLL; ++u) {
                if (COPY) d4[g + u * stride] = w[u];
                dg_group(w[u], (uint64_t)(g + u * stride), sum, xr);
            }
        }
        for (; g < n_full; g += stride) {
            const u32x4 w = s4[g];
            if (COPY) d4[g] = w;
            dg_group(w, (uint64_t)g, sum, xr);
        }
    } else {
        for (; g < n_full; g += stride) {
            u32x4 w;
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = src[4 * g + j];
            if (COPY) {
#pragma unroll
                for (int j = 0; j < 4; ++j) dst[4 * g + j] = w[j];
            }
            dg_group(w, (uint64_t)g, sum, xr);
        }
    }
    // the partial last group (1 .. 3 words): whichever lane the stride hands group n_full to
    if ((n_words & 3) != 0 && g == n_full) {
        u32x4 w = {0u, 0u, 0u, 0u};
        const int rest = (int)(n_words & 3);
        for (int j = 0; j < rest; ++j) {
            w[j] = src[4 * n_full + j];
            if (COPY) dst[4 * n_full + j] = w[j];
        }
        dg_group(w, (uint64_t)n_full, sum, xr);
    }
    // wave64, then the workgroup's four waves through LDS
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        sum += shfl_xor64(sum, m);
        xr ^= shfl_xor64(xr, m);
    }
    __shared__ uint64_t part[2][GRID_NT / 64];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { part[0][wave] = sum; part[1][wave] = xr; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t s = 0, x = 0;
#pragma unroll
        for (int i = 0; i < GRID_NT / 64; ++i) { s += part[0][i]; x ^= part[1][i]; }
        if (FINAL) {
            out[0] = s ^ len_mix;
            out[1] = x;
        } else {
            atomicAdd(out + 0, (unsigned long long)s);
            atomicXor(out + 1, (unsigned long long)x);
        }
    }
}

__global__ void digest_finish_kernel(unsigned long long* out, uint64_t len_mix) { out[0] ^= len_mix; }

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <bool VEC, bool COPY>
int launch_digest(const uint32_t* src, uint32_t* dst, int64_t n_words, uint64_t len_mix, unsigned long long* out, hipStream_t s) {
    const int64_t n_groups = (n_words + 3) / 4;
    // up to DG_UNROLL groups per lane before the grid grows past one workgroup; grid_for caps it at what fills the chip
    const int grid = grid_for((n_groups + DG_UNROLL - 1) / DG_UNROLL);
    if (grid == 1) {
        hipLaunchKernelGGL((state_digest_kernel<VEC, COPY, true>), dim3(1), dim3(GRID_NT), 0, s, src, dst, n_words, len_mix, out);
        CODAE_LAUNCH_CHECK();
        return CODAE_OK;
    }
    CODAE_HIP_CHECK(hipMemsetAsync(out, 0, 2 * sizeof(uint64_t), s));
    hipLaunchKernelGGL((state_digest_kernel<VEC, COPY, false>), dim3(grid), dim3(GRID_NT), 0, s, src, dst, n_words, len_mix, out);
    CODAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(digest_finish_kernel, dim3(1), dim3(1), 0, s, out, len_mix);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

}  // namespace
}  // namespace codae

extern "C" {

int codae_state_digest(const void* src, void* dst, int64_t n_bytes, uint64_t* out, void* stream) {
    using namespace codae;
    CODAE_REQUIRE(n_bytes >= 0, "codae_state_digest: n_bytes %lld is negative", (long long)n_bytes);
    CODAE_REQUIRE(n_bytes % 4 == 0, "codae_state_digest: n_bytes %lld is not a multiple of 4", (long long)n_bytes);
    CODAE_REQUIRE(out != nullptr, "codae_state_digest: out is NULL");
    CODAE_REQUIRE(n_bytes == 0 || src != nullptr, "codae_state_digest: src is NULL with n_bytes %lld", (long long)n_bytes);
    CODAE_REQUIRE((reinterpret_cast<uintptr_t>(src) & 3u) == 0 && (reinterpret_cast<uintptr_t>(dst) & 3u) == 0 &&
                  (reinterpret_cast<uintptr_t>(out) & 7u) == 0, "codae_state_digest: src and dst must be 4-byte aligned, out 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const uint32_t* sp = static_cast<const uint32_t*>(src);
    uint32_t* dp = n_bytes == 0 ? nullptr : static_cast<uint32_t*>(dst);
    unsigned long long* op = reinterpret_cast<unsigned long long*>(out);
    const int64_t n_words = n_bytes / 4;
    const uint64_t len_mix = dg_mix((uint64_t)n_bytes);
    const bool vec = aligned16(sp) && aligned16(dp);
    if (dp != nullptr) return vec ? launch_digest<true, true>(sp, dp, n_words, len_mix, op, s) : launch_digest<false, true>(sp, dp, n_words, len_mix, op, s);
    return vec ? launch_digest<true, false>(sp, nullptr, n_words, len_mix, op, s) : launch_digest<false, false>(sp, nullptr, n_words, len_mix, op, s);
}

}  // extern "C"
