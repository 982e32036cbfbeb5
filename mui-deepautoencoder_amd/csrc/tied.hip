// Tied encoder / decoder weights (include/codae_hip.h, "Tied weights"): the two kernels that sit between the backward and the
// update of a tied stack.  Both walk the ENCODER matrix W [rows][cols] of every pair in 64 x 64 tiles; the decoder matrix
// W' [cols][rows] = W^T is reached through a transposed tile in LDS, so both sides are read and written in whole rows of the
// tile, 16 bytes per lane.  Every element has exactly one writer: no atomics.  Partial tiles are predicated.
#include "codae_common.h"

namespace codae {
namespace {

constexpr int NT = GRID_NT;
constexpr int TT = 64;                 // tile edge
constexpr int TIE_MAX = 64;            // pairs per launch

struct TieJobs {
    int n;
    int64_t enc[TIE_MAX], dec[TIE_MAX];     // element offsets of W and W'
    int rows[TIE_MAX], cols[TIE_MAX];       // W is [rows][cols]
    int tile_begin[TIE_MAX + 1];            // prefix sum of tiles per pair
};

// which pair and which tile of it this workgroup owns
__device__ __forceinline__ void tie_locate(const TieJobs& jobs, int& m, int& r0, int& c0) {
    m = 0;
    while (m + 1 < jobs.n && (int)blockIdx.x >= jobs.tile_begin[m + 1]) ++m;
    const int t = blockIdx.x - jobs.tile_begin[m];
    const int tiles_c = (jobs.cols[m] + TT - 1) / TT;
    r0 = (t / tiles_c) * TT;
    c0 = (t % tiles_c) * TT;
}

// g[W][i][j] <- g[W][i][j] + g[W'][j][i];  g[W'] <- +0.   VEC: rows, cols and both offsets are multiples of 4
template <bool VEC>
__global__ __launch_bounds__(NT) void tie_fold_kernel(float* g, TieJobs jobs) {
    __shared__ float t[TT][TT + 1];          // t[c][r]: the decoder tile as it lies in memory
    int m, r0, c0;
    tie_locate(jobs, m, r0, c0);
    const int R = jobs.rows[m], C = jobs.cols[m];
    float* E = g + jobs.enc[m];
    float* D = g + jobs.dec[m];
    if constexpr (VEC) {
#pragma unroll
        for (int it = 0; it < TT * TT / 4 / NT; ++it) {
            const int q = threadIdx.x + it * NT;
            const int c = q >> 4, r4 = (q & 15) * 4;          // decoder row c0 + c, its columns r0 + r4 ..
            if (c0 + c < C && r0 + r4 < R) {
                float4* src = reinterpret_cast<float4*>(D + (int64_t)(c0 + c) * R + r0 + r4);
                const float4 v = *src;
                t[c][r4 + 0] = v.x; t[c][r4 + 1] = v.y; t[c][r4 + 2] = v.z; t[c][r4 + 3] = v.w;
                *src = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < TT * TT / 4 / NT; ++it) {
            const int q = threadIdx.x + it * NT;
            const int r = q >> 4, c4 = (q & 15) * 4;
            if (r0 + r < R && c0 + c4 < C) {
                float4* dst = reinterpret_cast<float4*>(E + (int64_t)(r0 + r) * C + c0 + c4);
                float4 e = *dst;
                e.x = e.x + t[c4 + 0][r]; e.y = e.y + t[c4 + 1][r]; e.z = e.z + t[c4 + 2][r]; e.w = e.w + t[c4 + 3][r];
                *dst = e;
            }
        }
    } else {
        for (int q = threadIdx.x; q < TT * TT; q += NT) {
            const int c = q >> 6, r = q & 63;
            if (c0 + c < C && r0 + r < R) {
                float* src = D + (int64_t)(c0 + c) * R + r0 + r;
                t[c][r] = *src;
                *src = 0.f;
            }
        }
        __syncthreads();
        for (int q = threadIdx.x; q < TT * TT; q += NT) {
            const int r = q >> 6, c = q & 63;
            if (r0 + r < R && c0 + c < C) {
                float* dst = E + (int64_t)(r0 + r) * C + c0 + c;
                *dst = *dst + t[c][r];
            }
        }
    }
}

__device__ __forceinline__ uint4 pack_bf16x8(const float* v) {
    return make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
}

// p[W'][j][i] <- p[W][i][j];  shadow[W'] <- bf16 of it;  shadow_t[W'] (= W'^T, laid out as W) <- bf16(p[W])
// VEC: rows, cols and both offsets are multiples of 8
template <bool VEC>
__global__ __launch_bounds__(NT) void tie_mirror_kernel(float* p, bf16_t* __restrict__ shadow, bf16_t* __restrict__ shadow_t,
                                                        TieJobs jobs) {
    __shared__ float t[TT][TT + 1];          // t[r][c]: the encoder tile as it lies in memory
    int m, r0, c0;
    tie_locate(jobs, m, r0, c0);
    const int R = jobs.rows[m], C = jobs.cols[m];
    const float* E = p + jobs.enc[m];
    const int64_t dec = jobs.dec[m];
    if constexpr (VEC) {
#pragma unroll
        for (int it = 0; it < TT * TT / 8 / NT; ++it) {
            const int q = threadIdx.x + it * NT;
            const int r = q >> 3, c8 = (q & 7) * 8;
            if (r0 + r < R && c0 + c8 < C) {
                const int64_t e = (int64_t)(r0 + r) * C + c0 + c8;
                const float4 a = *reinterpret_cast<const float4*>(E + e), b = *reinterpret_cast<const float4*>(E + e + 4);
                const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
                for (int k = 0; k < 8; ++k) t[r][c8 + k] = v[k];
                if (shadow_t != nullptr) *reinterpret_cast<uint4*>(shadow_t + dec + e) = pack_bf16x8(v);
            }
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < TT * TT / 8 / NT; ++it) {
            const int q = threadIdx.x + it * NT;
            const int c = q >> 3, r8 = (q & 7) * 8;           // decoder row c0 + c, its columns r0 + r8 ..
            if (c0 + c < C && r0 + r8 < R) {
                float v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = t[r8 + k][c];
                const int64_t d = dec + (int64_t)(c0 + c) * R + r0 + r8;
                *reinterpret_cast<float4*>(p + d) = make_float4(v[0], v[1], v[2], v[3]);
                *reinterpret_cast<float4*>(p + d + 4) = make_float4(v[4], v[5], v[6], v[7]);
                if (shadow != nullptr) *reinterpret_cast<uint4*>(shadow + d) = pack_bf16x8(v);
            }
        }
    } else {
        for (int q = threadIdx.x; q < TT * TT; q += NT) {
            const int r = q >> 6, c = q & 63;
            if (r0 + r < R && c0 + c < C) {
                const int64_t e = (int64_t)(r0 + r) * C + c0 + c;
                const float v = E[e];
                t[r][c] = v;
                if (shadow_t != nullptr) shadow_t[dec + e] = f32_to_bf16(v);
            }
        }
        __syncthreads();
        for (int q = threadIdx.x; q < TT * TT; q += NT) {
            const int c = q >> 6, r = q & 63;
            if (c0 + c < C && r0 + r < R) {
                const int64_t d = dec + (int64_t)(c0 + c) * R + r0 + r;
                const float v = t[r][c];
                p[d] = v;
                if (shadow != nullptr) shadow[d] = f32_to_bf16(v);
            }
        }
    }
}

inline bool a16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the largest of 8, 4, 2, 1 that divides every offset and extent of the list
int tie_multiple(const codae_tie_pair* pairs, int n) {
    int mm = 8;
    for (int i = 0; i < n; ++i) {
        const codae_tie_pair& a = pairs[i];
        while (mm > 1 && (a.rows % mm || a.cols % mm || a.enc_off % mm || a.dec_off % mm)) mm /= 2;
    }
    return mm;
}

}  // namespace

// A caller-supplied list (the two C entries): shapes, offsets, no two ranges overlapping.  The engine's own list is built by
// codae_set_tied_weights from its layout and goes to the launchers unchecked.
int check_tie_pairs(const codae_tie_pair* pairs, int n, const char* who) {
    CODAE_REQUIRE(pairs != nullptr && n >= 1, "%s: no pairs", who);
    for (int i = 0; i < n; ++i) {
        const codae_tie_pair& a = pairs[i];
        CODAE_REQUIRE(a.rows > 0 && a.cols > 0 && a.enc_off >= 0 && a.dec_off >= 0, "%s: pair %d: %d x %d at %lld / %lld", who, i, a.rows,
                      a.cols, (long long)a.enc_off, (long long)a.dec_off);
    }
    // every encoder and decoder range against every other one
    for (int i = 0; i < 2 * n; ++i) {
        const codae_tie_pair& a = pairs[i / 2];
        const int64_t alo = (i & 1) ? a.dec_off : a.enc_off, ahi = alo + (int64_t)a.rows * a.cols;
        for (int j = i + 1; j < 2 * n; ++j) {
            const codae_tie_pair& b = pairs[j / 2];
            const int64_t blo = (j & 1) ? b.dec_off : b.enc_off, bhi = blo + (int64_t)b.rows * b.cols;
            CODAE_REQUIRE(ahi <= blo || bhi <= alo, "%s: the ranges of pairs %d and %d overlap", who, i / 2, j / 2);
        }
    }
    return CODAE_OK;
}

namespace {

TieJobs tie_jobs(const codae_tie_pair* pairs, int n) {
    TieJobs jobs;
    jobs.n = n;
    int total = 0;
    for (int i = 0; i < n; ++i) {
        jobs.enc[i] = pairs[i].enc_off; jobs.dec[i] = pairs[i].dec_off; jobs.rows[i] = pairs[i].rows; jobs.cols[i] = pairs[i].cols;
        jobs.tile_begin[i] = total;
        total += ((pairs[i].rows + TT - 1) / TT) * ((pairs[i].cols + TT - 1) / TT);
    }
    jobs.tile_begin[n] = total;
    return jobs;
}

}  // namespace

int launch_tie_fold(float* g, const codae_tie_pair* pairs, int n, hipStream_t s) {
    CODAE_REQUIRE(g != nullptr && pairs != nullptr && n >= 1, "tie_fold: null gradients or no pairs");
    const int mult = tie_multiple(pairs, n);
    const bool vec = mult >= 4 && a16(g);
    for (int base = 0; base < n; base += TIE_MAX) {
        const TieJobs jobs = tie_jobs(pairs + base, n - base < TIE_MAX ? n - base : TIE_MAX);
        const int total = jobs.tile_begin[jobs.n];
        if (vec) hipLaunchKernelGGL(tie_fold_kernel<true>, dim3(total), dim3(NT), 0, s, g, jobs);
        else hipLaunchKernelGGL(tie_fold_kernel<false>, dim3(total), dim3(NT), 0, s, g, jobs);
        CODAE_LAUNCH_CHECK();
    }
    return CODAE_OK;
}

int launch_tie_mirror(float* p, bf16_t* shadow, bf16_t* shadow_t, const codae_tie_pair* pairs, int n, hipStream_t s) {
    CODAE_REQUIRE(p != nullptr && pairs != nullptr && n >= 1, "tie_mirror: null parameters or no pairs");
    const int mult = tie_multiple(pairs, n);
    const bool shadows = shadow != nullptr || shadow_t != nullptr;
    CODAE_REQUIRE(!shadows || (mult == 8 && a16(shadow) && a16(shadow_t)),
                  "tie_mirror: with a bf16 shadow every offset, rows and cols must be multiples of 8 and the shadows 16-byte aligned");
    const bool vec = mult == 8 && a16(p);
    for (int base = 0; base < n; base += TIE_MAX) {
        const TieJobs jobs = tie_jobs(pairs + base, n - base < TIE_MAX ? n - base : TIE_MAX);
        const int total = jobs.tile_begin[jobs.n];
        if (vec) hipLaunchKernelGGL(tie_mirror_kernel<true>, dim3(total), dim3(NT), 0, s, p, shadow, shadow_t, jobs);
        else hipLaunchKernelGGL(tie_mirror_kernel<false>, dim3(total), dim3(NT), 0, s, p, shadow, shadow_t, jobs);
        CODAE_LAUNCH_CHECK();
    }
    return CODAE_OK;
}

}  // namespace codae

extern "C" {

int codae_tie_fold(float* grads, const codae_tie_pair* pairs, int32_t n_pairs, void* stream) {
    int rc = codae::check_tie_pairs(pairs, n_pairs, "tie_fold");
    if (rc) return rc;
    return codae::launch_tie_fold(grads, pairs, n_pairs, (hipStream_t)stream);
}

int codae_tie_mirror(float* params, void* shadow_w, void* shadow_wt, const codae_tie_pair* pairs, int32_t n_pairs, void* stream) {
    int rc = codae::check_tie_pairs(pairs, n_pairs, "tie_mirror");
    if (rc) return rc;
    return codae::launch_tie_mirror(params, reinterpret_cast<codae::bf16_t*>(shadow_w), reinterpret_cast<codae::bf16_t*>(shadow_wt), pairs,
                                    n_pairs, (hipStream_t)stream);
}

}  // extern "C"
