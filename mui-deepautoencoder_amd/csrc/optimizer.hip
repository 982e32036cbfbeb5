// The parameter update of the DAE step: sum g^2 and the clip_grad_norm_ coefficient, clip folded into Adam / AdamW / SGD with the
// learning-rate schedule, the bf16 shadow refresh (flat, or tiled with the transposed shadow in the same pass).
#include "loss_sweep.h"

namespace codae {
namespace {

constexpr int NT = GRID_NT;

// ---- a7: sum g^2 (clip_grad_norm_, train_dae_on_embedding.py:213) ---------------------------
__global__ __launch_bounds__(NT) void sumsq_kernel(const float* __restrict__ g, int64_t n, double* out) {
    __shared__ float red[4];
    float s = 0.f;
    const int64_t n4 = n / 4;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n4; e += (int64_t)gridDim.x * NT) {
        const float4 v = reinterpret_cast<const float4*>(g)[e];
        s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    for (int64_t e = n4 * 4 + (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT)
        s += g[e] * g[e];
    const float b = block_sum(s, red);
    // `out` points at scalars[GRAD_SQ]; scatter over the slot array that follows the named scalars
    if (threadIdx.x == 0)
        atomicAdd(out + (CODAE_S_GRAD_SQ_SLOTS - CODAE_S_GRAD_SQ) + (blockIdx.x & (CODAE_S_N_SLOTS - 1)), (double)b);
}

// *acc += sum g^2 with at most 64 blocks (a rank's parameter shard in the sharded update): one address, few adders
__global__ __launch_bounds__(NT) void sumsq_to_kernel(const float* __restrict__ g, int64_t n, double* acc) {
    __shared__ float red[4];
    float s = 0.f;
    const int64_t n4 = n / 4;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n4; e += (int64_t)gridDim.x * NT) {
        const float4 v = reinterpret_cast<const float4*>(g)[e];
        s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    for (int64_t e = n4 * 4 + (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT) s += g[e] * g[e];
    const float b = block_sum(s, red);
    if (threadIdx.x == 0) atomicAdd(acc, (double)b);
}

// clip_grad_norm_'s coefficient from a total sum g^2 (train_dae_on_embedding.py:213): min(1, max_norm / (norm + 1e-6))
// as torch.clamp(max=1): a NaN norm gives a NaN coefficient (fminf would give 1), an infinite one gives 0
__device__ __forceinline__ float clip_coef(float max_norm, float total) {
    const float r = max_norm / (total + 1e-6f);
    return r > 1.f ? 1.f : r;
}
__global__ void clip_coef_kernel(const double* total_sq, float max_norm, double* coef_out) {
    const float total = sqrtf((float)*total_sq);
    *coef_out = (double)clip_coef(max_norm, total);
}

// ---- a7 + a8: clip scale folded into Adam (torch.optim.Adam, amsgrad off, L2 decay) ----------
struct AdamConst {
    float lr_over_bc1, inv_sqrt_bc2, beta1, beta2, eps, wd, max_norm;
    float lr;                // graph replay: the bias corrections are rebuilt on the device from *step_dev
};

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float coef, const AdamConst& c) {
    g = g * coef + c.wd * p;
    m = c.beta1 * m + (1.f - c.beta1) * g;
    v = c.beta2 * v + (1.f - c.beta2) * g * g;
    const float denom = sqrtf(v) * c.inv_sqrt_bc2 + c.eps;
    p = p - c.lr_over_bc1 * (m / denom);
}

// ---- optimizer kinds and the learning-rate schedule (codae_optimizer, include/codae_hip.h) ----
// Both update kernels are templated on (KIND, AMS, SCHED); <CODAE_OPT_ADAM, false, false> is the code above, untouched.  Every other
// instantiation rebuilds lr_t and the bias corrections in its prologue, in double, from the step count - the kernel argument in a
// plain step, the device scalar under graph replay: the same code, so a replayed step has the bits of a plain one.
struct OptConst {
    float mu;                // SGD momentum
    int nesterov;
    int sched, warmup, total, period;
    float min_factor, gamma;
    int step;                // hyper->step (a plain step's t)
    float decay;             // ADAMW: lr_t wd, filled by the prologue
};

// f(t) of include/codae_hip.h ("Optimizer and schedule"), in double
__device__ __forceinline__ double lr_factor(const OptConst& o, double t) {
    const double W = (double)o.warmup;
    const double w = (o.warmup > 0 && t <= W) ? t / W : 1.0;
    double f = 1.0;
    if (o.sched == CODAE_SCHED_COSINE || o.sched == CODAE_SCHED_LINEAR) {
        double q = (t - W) / ((double)o.total - W);
        q = q < 0.0 ? 0.0 : (q > 1.0 ? 1.0 : q);
        const double mf = (double)o.min_factor;
        f = o.sched == CODAE_SCHED_COSINE ? mf + (1.0 - mf) * (1.0 + cos(M_PI * q)) / 2.0 : 1.0 - (1.0 - mf) * q;
    } else if (o.sched == CODAE_SCHED_STEP) {
        f = pow((double)o.gamma, floor((t - 1.0) / (double)o.period));
    }
    return w * f;
}

// c.lr <- lr_t, the bias-correction factors from it (ADAM / ADAMW), o.decay (ADAMW)
template <int KIND, bool SCHED>
__device__ __forceinline__ void opt_prologue(AdamConst& c, OptConst& o, const double* __restrict__ step_dev) {
    const double t = step_dev != nullptr ? *step_dev : (double)o.step;
    if constexpr (SCHED) c.lr = (float)((double)c.lr * lr_factor(o, t));
    if constexpr (KIND != CODAE_OPT_SGD && KIND != CODAE_OPT_LARS) {
        c.lr_over_bc1 = (float)((double)c.lr / (1.0 - pow((double)c.beta1, t)));
        c.inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)c.beta2, t)));
    }
    o.decay = c.lr * c.wd;
}

// ---- layer-wise trust ratios: LAMB and LARS (include/codae_hip.h, "Layer-wise trust ratios") ----
// The update kernels carry a last argument TrustConst and a per-launch TrustStep; every instantiation of another kind ignores both.
// A block works on ONE matrix or on the bias block (the tiled kernel by its tile table, the flat kernel by its launch).
template <int KIND> constexpr bool IS_TRUST = KIND == CODAE_OPT_LAMB || KIND == CODAE_OPT_LARS;
struct TrustConst {
    const float* ratio;      // [64] fp32, the finish's output (head of the work space)
    int mat;                 // flat kernel: the matrix this launch walks, -1 = the bias block; the tiled kernel finds its own
    int decay_bias;
};
struct TrustStep { float ratio, wd, inv_bc1; };      // this block: wave-uniform

// mat >= 0: that matrix (its ratio, or 1 in the norms pass, which passes ratio == nullptr), < 0: the bias block
template <int KIND>
__device__ __forceinline__ TrustStep trust_begin(const TrustConst& tr, int mat, const AdamConst& c, const OptConst& o,
                                                 const double* __restrict__ step_dev) {
    TrustStep ts{1.f, c.wd, 1.f};
    if constexpr (IS_TRUST<KIND>) {
        if (mat >= 0) ts.ratio = tr.ratio != nullptr ? tr.ratio[mat] : 1.f;
        else if (!tr.decay_bias) ts.wd = 0.f;
        if constexpr (KIND == CODAE_OPT_LAMB) {
            const double t = step_dev != nullptr ? *step_dev : (double)o.step;
            ts.inv_bc1 = (float)(1.0 / (1.0 - pow((double)c.beta1, t)));
        }
    }
    return ts;
}

// What the norm beside P is taken of, and the moments on the way - LAMB: u (m, v <- m', v');  LARS: g' (m, v untouched).
// The norms pass and the update both call this: one operand order, every operation rounded on its own.
template <int KIND>
__device__ __forceinline__ float trust_dir(float p, float g, float& m, float& v, float coef, const AdamConst& c, const TrustStep& ts) {
#pragma clang fp contract(off)
    const float g1 = g * coef;
    if constexpr (KIND == CODAE_OPT_LARS) return g1;
    // (each sum's first product through an opaque copy: two products of one sum are otherwise packed into a v_pk_mul_f32 and added
    //  across the halves of the pair with op_sel - the form DESIGN.md section 5d rules out and tools/check_isa.py rejects)
    float bm = c.beta1 * m, bv = c.beta2 * v;
    asm volatile("" : "+v"(bm), "+v"(bv));
    m = bm + (1.f - c.beta1) * g1;
    v = bv + ((1.f - c.beta2) * g1) * g1;
    const float denom = sqrtf(v) * c.inv_sqrt_bc2 + c.eps;
    float r = (m / denom) * ts.inv_bc1;
    asm volatile("" : "+v"(r));
    return r + ts.wd * p;
}

// p <- p' from the direction above and the block's ratio (LARS: m <- m' here)
template <int KIND>
__device__ __forceinline__ void trust_apply(float& p, float dir, float& m, const AdamConst& c, const OptConst& o, const TrustStep& ts) {
#pragma clang fp contract(off)
    if constexpr (KIND == CODAE_OPT_LAMB) {
        p = p - (c.lr * ts.ratio) * dir;
    } else {
        const float d = ts.ratio * (dir + ts.wd * p);
        m = o.mu * m + d;
        const float u = o.nesterov ? d + o.mu * m : m;
        p = p - c.lr * u;
    }
}

template <int KIND, bool AMS>
__device__ __forceinline__ void opt_one(float& p, float g, float& m, float& v, float& vm, float coef, const AdamConst& c,
                                        const OptConst& o, const TrustStep& ts) {
    if constexpr (IS_TRUST<KIND>) {
        const float dir = trust_dir<KIND>(p, g, m, v, coef, c, ts);
        trust_apply<KIND>(p, dir, m, c, o, ts);
    } else if constexpr (KIND == CODAE_OPT_SGD) {
        g = g * coef + c.wd * p;
        m = o.mu * m + g;
        const float u = o.nesterov ? g + o.mu * m : m;
        p = p - c.lr * u;
    } else if constexpr (KIND == CODAE_OPT_ADAM && !AMS) {
        adam_one(p, g, m, v, coef, c);
    } else {
        if constexpr (KIND == CODAE_OPT_ADAMW) { g = g * coef; p = p - o.decay * p; }     // p (1 - lr_t wd), rounded once at p's size
        else g = g * coef + c.wd * p;
        m = c.beta1 * m + (1.f - c.beta1) * g;
        v = c.beta2 * v + (1.f - c.beta2) * g * g;
        float d = v;
        if constexpr (AMS) { vm = (v > vm || v != v) ? v : vm; d = vm; }       // torch.maximum: a NaN on either side stays
        const float denom = sqrtf(d) * c.inv_sqrt_bc2 + c.eps;
        p = p - c.lr_over_bc1 * (m / denom);
    }
}

// What both update kernels do first: the step's constants (c, o) and the clip coefficient, which is returned - *coef_in when
// given, else from sum g^2 = scalars[GRAD_SQ] + its 64 partial slots (one wave adds them up, LDS broadcasts), 1 without clipping
template <int KIND, bool AMS, bool SCHED>
__device__ __forceinline__ float opt_begin(AdamConst& c, OptConst& o, const double* __restrict__ step_dev,
                                           const double* __restrict__ grad_sq, const double* __restrict__ coef_in) {
    if constexpr (KIND != CODAE_OPT_ADAM || AMS || SCHED) {
        opt_prologue<KIND, SCHED>(c, o, step_dev);
    } else if (step_dev != nullptr) {
        // replayed from a hipGraph: the step count lives in device memory (kernel arguments are frozen at capture)
        const double t = *step_dev;
        c.lr_over_bc1 = (float)((double)c.lr / (1.0 - pow((double)c.beta1, t)));
        c.inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)c.beta2, t)));
    }
    if (coef_in != nullptr) return (float)(*coef_in);
    if (!(c.max_norm > 0.f)) return 1.f;
    __shared__ double total_sq;
    if (threadIdx.x < 64) {
        double v = grad_sq[(CODAE_S_GRAD_SQ_SLOTS - CODAE_S_GRAD_SQ) + threadIdx.x];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
        if (threadIdx.x == 0) total_sq = v + grad_sq[0];
    }
    __syncthreads();
    return clip_coef(c.max_norm, sqrtf((float)total_sq));
}

// ---- weight average (codae_weight_average, include/codae_hip.h "Weight average") --------------
// Both update kernels carry a fourth template flag AVG; the AVG = false instantiations are the code above and below without a line
// of this.  AVG = true: the prologue decides from the step count - the same source the schedule reads - whether this step samples
// and with which weight, and every element's new parameter goes into the average on its way to memory.
struct AvgConst {
    float* avg;              // at the same offset as p (a span passes avg + lo)
    int kind, debias, start, every;
    float decay;
};
struct AvgStep { float* avg; float w; bool sample; };      // this launch: wave-uniform, all of it

// w32 of step t, in double; false: the step does not sample
__host__ __device__ inline bool avg_weight(int kind, float decay, int debias, int start, int every, int64_t t, float* w32) {
    if (t < (int64_t)start || (t - start) % every != 0) return false;
    const int64_t n = (t - start) / every;
    double w = 1.0;
    if (kind == CODAE_AVG_SWA) w = 1.0 / (double)(n + 1);
    else if (n > 0) {
        double d = (double)decay;
        if (debias) { const double r = (1.0 + (double)n) / (10.0 + (double)n); d = d < r ? d : r; }
        w = 1.0 - d;
    }
    *w32 = (float)w;
    return true;
}

template <bool AVG>
__device__ __forceinline__ AvgStep avg_begin(const AvgConst& a, const OptConst& o, const double* __restrict__ step_dev) {
    AvgStep st{nullptr, 1.f, false};
    if constexpr (AVG) {
        const double t = step_dev != nullptr ? *step_dev : (double)o.step;
        st.avg = a.avg;
        st.sample = avg_weight(a.kind, a.decay, a.debias, a.start, a.every, (int64_t)t, &st.w);
    }
    return st;
}

__device__ __forceinline__ float avg_one(float a, float p, float w) { return a + w * (p - a); }
// one element / four elements (16-B accesses) of the average at offset e; w == 1: a bit copy, the old average is not read
__device__ __forceinline__ void avg_put(const AvgStep& st, int64_t e, float p) {
    st.avg[e] = st.w == 1.f ? p : avg_one(st.avg[e], p, st.w);
}
__device__ __forceinline__ void avg_put4(const AvgStep& st, int64_t e, const float4& pp) {
    float4 aa = pp;
    if (st.w != 1.f) {
        aa = *reinterpret_cast<const float4*>(st.avg + e);
        aa.x = avg_one(aa.x, pp.x, st.w); aa.y = avg_one(aa.y, pp.y, st.w);
        aa.z = avg_one(aa.z, pp.z, st.w); aa.w = avg_one(aa.w, pp.w, st.w);
    }
    *reinterpret_cast<float4*>(st.avg + e) = aa;
}

// the update of the four elements at offset e of the flat vectors (16-B accesses; SGD neither reads nor writes v, only AMSGrad
// touches vmax; AVG: one more float4 load and store on a sampling step, none otherwise); returns the new parameters, for the
// caller's shadows
template <int KIND, bool AMS, bool AVG>
__device__ __forceinline__ float4 opt_four(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                           float* __restrict__ vmax, int64_t e, float coef, const AdamConst& c, const OptConst& o,
                                           const AvgStep& av, const TrustStep& ts) {
    constexpr bool HAS_V = KIND != CODAE_OPT_SGD && KIND != CODAE_OPT_LARS;
    float4 pp = *reinterpret_cast<float4*>(p + e);
    const float4 gg = *reinterpret_cast<const float4*>(g + e);
    float4 mm = *reinterpret_cast<float4*>(m + e);
    float4 vv = make_float4(0.f, 0.f, 0.f, 0.f), xx = vv;
    if constexpr (HAS_V) vv = *reinterpret_cast<float4*>(v + e);
    if constexpr (AMS) xx = *reinterpret_cast<float4*>(vmax + e);
    opt_one<KIND, AMS>(pp.x, gg.x, mm.x, vv.x, xx.x, coef, c, o, ts);
    opt_one<KIND, AMS>(pp.y, gg.y, mm.y, vv.y, xx.y, coef, c, o, ts);
    opt_one<KIND, AMS>(pp.z, gg.z, mm.z, vv.z, xx.z, coef, c, o, ts);
    opt_one<KIND, AMS>(pp.w, gg.w, mm.w, vv.w, xx.w, coef, c, o, ts);
    *reinterpret_cast<float4*>(p + e) = pp;
    *reinterpret_cast<float4*>(m + e) = mm;
    if constexpr (HAS_V) *reinterpret_cast<float4*>(v + e) = vv;
    if constexpr (AMS) *reinterpret_cast<float4*>(vmax + e) = xx;
    if constexpr (AVG) {
        if (av.sample) {
            // the average takes p' through an opaque copy: the update's own arithmetic must be selected, packed and contracted exactly
            // as without the average (its bits are pinned), so nothing of the average's may be visible to the passes that shape it
            float4 q = pp;
            asm volatile("" : "+v"(q.x), "+v"(q.y), "+v"(q.z), "+v"(q.w));
            avg_put4(av, e, q);
        }
    }
    return pp;
}

template <int KIND, bool AMS, bool SCHED, bool AVG>
__global__ __launch_bounds__(NT) void clip_adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                       float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                       AdamConst c, const double* __restrict__ grad_sq,
                                                       bf16_t* __restrict__ shadow, const double* __restrict__ coef_in,
                                                       const double* __restrict__ step_dev, float* __restrict__ vmax, OptConst o,
                                                       AvgConst a, TrustConst tr) {
    constexpr bool HAS_V = KIND != CODAE_OPT_SGD && KIND != CODAE_OPT_LARS;          // SGD and LARS neither read nor write v
    const float coef = opt_begin<KIND, AMS, SCHED>(c, o, step_dev, grad_sq, coef_in);
    const AvgStep av = avg_begin<AVG>(a, o, step_dev);
    const TrustStep ts = trust_begin<KIND>(tr, tr.mat, c, o, step_dev);
    const int64_t n4 = n / 4;  // n is padded to a multiple of 64 by the engine; tail handled below anyway
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n4; e += (int64_t)gridDim.x * NT) {
        const float4 pp = opt_four<KIND, AMS, AVG>(p, g, m, v, vmax, 4 * e, coef, c, o, av, ts);
        if (shadow) reinterpret_cast<uint2*>(shadow)[e] = pack_bf16x4(pp.x, pp.y, pp.z, pp.w);
    }
    for (int64_t e = n4 * 4 + (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT) {
        float pp = p[e], mm = m[e], vv = 0.f, xx = 0.f;
        if constexpr (HAS_V) vv = v[e];
        if constexpr (AMS) xx = vmax[e];
        opt_one<KIND, AMS>(pp, g[e], mm, vv, xx, coef, c, o, ts);
        p[e] = pp; m[e] = mm;
        if constexpr (HAS_V) v[e] = vv;
        if constexpr (AMS) vmax[e] = xx;
        if (shadow) shadow[e] = f32_to_bf16(pp);
    }
    // (the tail's average in a sweep of its own, every thread over the elements it has just written: inside the loop above it
    //  changed which of that loop's products the compiler packs and contracts, and with that the pinned bits of p)
    if constexpr (AVG) {
        if (av.sample)
            for (int64_t e = n4 * 4 + (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT) avg_put(av, e, p[e]);
    }
}

// Tiled form of clip_adam for the bf16 engine: the weight matrices are walked in 64 x 128 tiles so that the same
// pass can also write the TRANSPOSED bf16 shadow (Wt_l [in][out], what the data-gradient GEMM reads) through LDS;
// the blocks past the last tile do the flat bias block.  Replaces clip_adam_kernel + transpose_bf16_kernel: 85 MB
// less traffic per step at C3 and no cross-stream hand-off for the transposes.
struct AdamTiles {
    int n_layers;
    int64_t off[64];          // element offset of W_l in the flat vectors (same in the shadows)
    int rows[64], cols[64];   // W_l is [rows = out][cols = in]
    int tile_begin[65];       // prefix sum of 64 x 128 tiles per layer
    int transposed_from;      // layers >= this also get the transposed shadow
    int64_t bias_off, bias_n; // flat tail
};
constexpr int AT_R = 64, AT_C = 128;

template <int KIND, bool AMS, bool SCHED, bool AVG>
__global__ __launch_bounds__(NT) void clip_adam_tiled_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                             float* __restrict__ m, float* __restrict__ v, AdamConst c,
                                                             const double* __restrict__ grad_sq, bf16_t* __restrict__ shadow,
                                                             bf16_t* __restrict__ shadow_t, AdamTiles jobs,
                                                             const double* __restrict__ step_dev, float* __restrict__ vmax, OptConst o,
                                                             AvgConst a, TrustConst tr) {
    constexpr bool HAS_V = KIND != CODAE_OPT_SGD && KIND != CODAE_OPT_LARS;
    __shared__ bf16_t tt[AT_C][AT_R + 8];          // transposed tile: [col][row], rows stay 16-byte aligned
    const float coef = opt_begin<KIND, AMS, SCHED>(c, o, step_dev, grad_sq, nullptr);
    const AvgStep av = avg_begin<AVG>(a, o, step_dev);
    const int n_tiles = jobs.tile_begin[jobs.n_layers];
    if ((int)blockIdx.x >= n_tiles) {
        // flat bias block, grid-strided over the remaining blocks
        const TrustStep ts = trust_begin<KIND>(tr, -1, c, o, step_dev);
        const int64_t nb = (int64_t)gridDim.x - n_tiles;
        for (int64_t e = ((int64_t)blockIdx.x - n_tiles) * NT + threadIdx.x; e < jobs.bias_n; e += nb * NT) {
            const int64_t i = jobs.bias_off + e;
            float pp = p[i], mm = m[i], vv = 0.f, xx = 0.f;
            if constexpr (HAS_V) vv = v[i];
            if constexpr (AMS) xx = vmax[i];
            opt_one<KIND, AMS>(pp, g[i], mm, vv, xx, coef, c, o, ts);
            p[i] = pp; m[i] = mm;
            if constexpr (HAS_V) v[i] = vv;
            if constexpr (AMS) vmax[i] = xx;
            shadow[i] = f32_to_bf16(pp);
        }
        // (the bias block's average in a sweep of its own, as in clip_adam_kernel's tail)
        if constexpr (AVG) {
            if (av.sample)
                for (int64_t e = ((int64_t)blockIdx.x - n_tiles) * NT + threadIdx.x; e < jobs.bias_n; e += nb * NT)
                    avg_put(av, jobs.bias_off + e, p[jobs.bias_off + e]);
        }
        return;
    }
    int l = 0;
    while (l + 1 < jobs.n_layers && (int)blockIdx.x >= jobs.tile_begin[l + 1]) ++l;
    const int t = blockIdx.x - jobs.tile_begin[l];
    const int R = jobs.rows[l], C = jobs.cols[l];
    const int tiles_c = (C + AT_C - 1) / AT_C;
    const int r0 = (t / tiles_c) * AT_R, c0 = (t % tiles_c) * AT_C;
    const int64_t base = jobs.off[l];
    const bool want_t = shadow_t != nullptr && l >= jobs.transposed_from;
    const TrustStep ts = trust_begin<KIND>(tr, l, c, o, step_dev);
#pragma unroll
    for (int it = 0; it < AT_R * AT_C / 4 / NT; ++it) {
        const int q = threadIdx.x + it * NT;          // float4 index inside the tile
        const int r = q / (AT_C / 4), cc = (q % (AT_C / 4)) * 4;
        if (r0 + r < R && c0 + cc < C) {
            const int64_t e = base + (int64_t)(r0 + r) * C + c0 + cc;
            const float4 pp = opt_four<KIND, AMS, AVG>(p, g, m, v, vmax, e, coef, c, o, av, ts);
            const uint2 sh = pack_bf16x4(pp.x, pp.y, pp.z, pp.w);
            *reinterpret_cast<uint2*>(shadow + e) = sh;
            if (want_t) {
                tt[cc + 0][r] = (bf16_t)(sh.x & 0xffff); tt[cc + 1][r] = (bf16_t)(sh.x >> 16);
                tt[cc + 2][r] = (bf16_t)(sh.y & 0xffff); tt[cc + 3][r] = (bf16_t)(sh.y >> 16);
            }
        }
    }
    if (!want_t) return;
    __syncthreads();
    // Wt[c0 + c][r0 .. r0 + 63]: 128-B row segments, 16 B per lane
#pragma unroll
    for (int it = 0; it < AT_C * (AT_R / 8) / NT; ++it) {
        const int q = threadIdx.x + it * NT;
        const int cidx = q / (AT_R / 8), r8 = (q % (AT_R / 8)) * 8;
        if (c0 + cidx < C && r0 + r8 < R)
            *reinterpret_cast<uint4*>(shadow_t + base + (int64_t)(c0 + cidx) * R + r0 + r8) =
                *reinterpret_cast<const uint4*>(&tt[cidx][r8]);
    }
}

// ---- trust ratios: the norms pass and the finish ---------------------------------------------
// One (sum p^2, sum d^2) double pair per block, d = trust_dir of the element (LAMB: u, LARS: g'): each square formed in fp32, widened,
// added in double - a lane over its elements in order, an xor butterfly per wave (both partners add the same two values, so every
// lane holds the same sum), the four waves in order.  No atomics: the order is the block shape's alone.
struct NormAcc { double pp = 0.0, dd = 0.0; };
__device__ __forceinline__ void norm_add(NormAcc& a, float p, float d) {
#pragma clang fp contract(off)
    const float p2 = p * p, d2 = d * d;
    a.pp += (double)p2; a.dd += (double)d2;
}
__device__ __forceinline__ void norm_block_store(NormAcc a, double* __restrict__ pair) {
    __shared__ double red[2][NT / 64];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { a.pp += __shfl_xor(a.pp, d); a.dd += __shfl_xor(a.dd, d); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a.pp; red[1][threadIdx.x >> 6] = a.dd; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sp = red[0][0], sd = red[1][0];
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) { sp += red[0][w]; sd += red[1][w]; }
        pair[0] = sp; pair[1] = sd;
    }
}
template <int KIND>
__device__ __forceinline__ void norm_four(NormAcc& a, const float* __restrict__ p, const float* __restrict__ g, const float* __restrict__ m,
                                          const float* __restrict__ v, int64_t e, float coef, const AdamConst& c, const TrustStep& ts) {
    const float4 pp = *reinterpret_cast<const float4*>(p + e);
    const float4 gg = *reinterpret_cast<const float4*>(g + e);
    float4 mm = make_float4(0.f, 0.f, 0.f, 0.f), vv = mm;
    if constexpr (KIND == CODAE_OPT_LAMB) { mm = *reinterpret_cast<const float4*>(m + e); vv = *reinterpret_cast<const float4*>(v + e); }
    norm_add(a, pp.x, trust_dir<KIND>(pp.x, gg.x, mm.x, vv.x, coef, c, ts));
    norm_add(a, pp.y, trust_dir<KIND>(pp.y, gg.y, mm.y, vv.y, coef, c, ts));
    norm_add(a, pp.z, trust_dir<KIND>(pp.z, gg.z, mm.z, vv.z, coef, c, ts));
    norm_add(a, pp.w, trust_dir<KIND>(pp.w, gg.w, mm.w, vv.w, coef, c, ts));
}

// Both norms kernels run opt_begin<KIND, false, false>: the schedule is never evaluated here.  That is right only as long as what
// trust_dir returns does not depend on lr_t - LAMB's u and LARS's g' do not; lr_t enters in trust_apply alone.  A trust_dir that
// reads c.lr needs the SCHED flag here too, or the two passes form different directions.
constexpr int TRUST_CHUNK = CODAE_TRUST_CHUNK;          // elements per block of the flat norms pass: NT lanes x 4 float4
static_assert(TRUST_CHUNK % (4 * NT) == 0, "a chunk is whole float4 rounds of a block");

// flat: block b over the elements [b CHUNK, (b + 1) CHUNK) of ONE matrix of n elements; grid = ceil(n / CHUNK), from n alone
template <int KIND>
__global__ __launch_bounds__(NT) void trust_norms_kernel(const float* __restrict__ p, const float* __restrict__ g, const float* __restrict__ m,
                                                         const float* __restrict__ v, int64_t n, AdamConst c,
                                                         const double* __restrict__ grad_sq, const double* __restrict__ coef_in,
                                                         const double* __restrict__ step_dev, OptConst o, double* __restrict__ parts) {
    const float coef = opt_begin<KIND, false, false>(c, o, step_dev, grad_sq, coef_in);
    const TrustStep ts = trust_begin<KIND>(TrustConst{nullptr, 0, 0}, 0, c, o, step_dev);
    NormAcc a;
    const int64_t n4 = n / 4, q0 = (int64_t)blockIdx.x * (TRUST_CHUNK / 4);
#pragma unroll
    for (int it = 0; it < TRUST_CHUNK / 4 / NT; ++it) {
        const int64_t q = q0 + it * NT + threadIdx.x;
        if (q < n4) norm_four<KIND>(a, p, g, m, v, 4 * q, coef, c, ts);
    }
    // the last block: the n % 4 elements behind the float4 body, one lane each
    if (blockIdx.x == gridDim.x - 1 && n4 * 4 + threadIdx.x < n) {
        const int64_t e = n4 * 4 + threadIdx.x;
        float mm = 0.f, vv = 0.f;
        if constexpr (KIND == CODAE_OPT_LAMB) { mm = m[e]; vv = v[e]; }
        norm_add(a, p[e], trust_dir<KIND>(p[e], g[e], mm, vv, coef, c, ts));
    }
    norm_block_store(a, parts + 2 * (int64_t)blockIdx.x);
}

// tiled: block = one 64 x 128 tile of the tiled update's table (the bias block belongs to no norm)
template <int KIND>
__global__ __launch_bounds__(NT) void trust_norms_tiled_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                               const float* __restrict__ m, const float* __restrict__ v, AdamConst c,
                                                               const double* __restrict__ grad_sq, AdamTiles jobs,
                                                               const double* __restrict__ step_dev, OptConst o, double* __restrict__ parts) {
    const float coef = opt_begin<KIND, false, false>(c, o, step_dev, grad_sq, nullptr);
    const TrustStep ts = trust_begin<KIND>(TrustConst{nullptr, 0, 0}, 0, c, o, step_dev);
    int l = 0;
    while (l + 1 < jobs.n_layers && (int)blockIdx.x >= jobs.tile_begin[l + 1]) ++l;
    const int t = blockIdx.x - jobs.tile_begin[l];
    const int R = jobs.rows[l], C = jobs.cols[l];
    const int tiles_c = (C + AT_C - 1) / AT_C;
    const int r0 = (t / tiles_c) * AT_R, c0 = (t % tiles_c) * AT_C;
    const int64_t base = jobs.off[l];
    NormAcc a;
#pragma unroll
    for (int it = 0; it < AT_R * AT_C / 4 / NT; ++it) {
        const int q = threadIdx.x + it * NT;
        const int r = q / (AT_C / 4), cc = (q % (AT_C / 4)) * 4;
        if (r0 + r < R && c0 + cc < C) norm_four<KIND>(a, p, g, m, v, base + (int64_t)(r0 + r) * C + c0 + cc, coef, c, ts);
    }
    norm_block_store(a, parts + 2 * (int64_t)blockIdx.x);
}

// finish: lane l adds matrix l's pairs [begin[l], begin[l + 1]) in index order and writes its fp32 ratio
struct TrustParts { int n_mats; int begin[CODAE_TRUST_MAX_MATRICES + 1]; };
__global__ __launch_bounds__(64) void trust_finish_kernel(const double* __restrict__ parts, TrustParts tp, float* __restrict__ ratio, int kind,
                                                          float trust_clip, float trust_coef, float wd, float eps) {
    const int l = threadIdx.x;
    if (l >= tp.n_mats) return;
    double sp = 0.0, sd = 0.0;
    for (int i = tp.begin[l]; i < tp.begin[l + 1]; ++i) { sp += parts[2 * i]; sd += parts[2 * i + 1]; }
    const double P = sqrt(sp), D = sqrt(sd);
    double r = 1.0;
    if (P > 0.0 && D > 0.0) r = kind == CODAE_OPT_LAMB ? P / D : (double)trust_coef * P / (D + (double)wd * P + (double)eps);
    if (trust_clip > 0.f && r > (double)trust_clip) r = (double)trust_clip;
    ratio[l] = (float)r;
}

// The average alone, behind somebody else's update (codae_weight_average_update): the host has decided that the step samples
__global__ __launch_bounds__(NT) void weight_average_kernel(float* __restrict__ avg, const float* __restrict__ p, int64_t n, float w) {
    const AvgStep av{avg, w, true};
    const int64_t n4 = n / 4;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n4; e += (int64_t)gridDim.x * NT)
        avg_put4(av, 4 * e, *reinterpret_cast<const float4*>(p + 4 * e));
    for (int64_t e = n4 * 4 + (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT) avg_put(av, e, p[e]);
}

__global__ void set_scalar_kernel(double* dst, double value) { *dst = value; }

// ---- the optimizer setting on the host: kernel constants, instantiation ----------------------
AdamConst adam_const(const codae_hyper* hp) {
    AdamConst c;
    const double bc1 = 1.0 - pow((double)hp->beta1, (double)hp->step);
    const double bc2 = 1.0 - pow((double)hp->beta2, (double)hp->step);
    c.lr_over_bc1 = (float)((double)hp->lr / bc1);
    c.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
    c.beta1 = hp->beta1; c.beta2 = hp->beta2; c.eps = hp->eps; c.wd = hp->weight_decay;
    c.max_norm = hp->max_grad_norm; c.lr = hp->lr;
    return c;
}

OptConst opt_const(const codae_optimizer* opt, const codae_hyper* hp) {
    OptConst o{};
    o.step = hp->step;
    if (!optimizer_is_default(opt)) {
        o.mu = opt->momentum; o.nesterov = opt->nesterov; o.sched = opt->sched; o.warmup = opt->warmup; o.total = opt->total;
        o.period = opt->period; o.min_factor = opt->min_factor; o.gamma = opt->gamma;
    }
    return o;
}

AvgConst avg_const(const codae_weight_average* wa, float* avg) {
    AvgConst a{};
    if (!weight_average_is_off(wa)) {
        a.avg = avg; a.kind = wa->kind; a.debias = wa->debias; a.start = wa->start; a.every = wa->every; a.decay = wa->decay;
    }
    return a;
}

// mat: the matrix a flat launch walks, -1 = the bias block (the tiled kernel finds its own); all zero for the other kinds
TrustConst trust_const(const codae_optimizer* opt, int mat) {
    TrustConst t{nullptr, -1, 0};
    if (opt != nullptr && (opt->kind == CODAE_OPT_LAMB || opt->kind == CODAE_OPT_LARS)) {
        t.ratio = reinterpret_cast<const float*>(opt->trust_ws); t.mat = mat; t.decay_bias = opt->decay_bias;
    }
    return t;
}
// the partial pairs of the norms pass, behind the 64 ratios
double* trust_parts(void* ws) { return reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + CODAE_TRUST_MAX_MATRICES * sizeof(float)); }

// f(std::integral_constant<int, KIND>, std::bool_constant<AMS>, std::bool_constant<SCHED>, std::bool_constant<AVG>) for the
// settings' instantiation
template <typename F>
void opt_dispatch(const codae_optimizer* opt, bool avg, F&& f) {
    const bool dflt = optimizer_is_default(opt);
    const int kind = dflt ? CODAE_OPT_ADAM : opt->kind;
    const bool ams = !dflt && opt->amsgrad != 0;
    const bool sched = !dflt && (opt->sched != CODAE_SCHED_CONSTANT || opt->warmup > 0);
    auto with_sched = [&](auto k, auto a) {
        if (sched) { if (avg) f(k, a, std::true_type{}, std::true_type{}); else f(k, a, std::true_type{}, std::false_type{}); }
        else { if (avg) f(k, a, std::false_type{}, std::true_type{}); else f(k, a, std::false_type{}, std::false_type{}); }
    };
    if (kind == CODAE_OPT_SGD) with_sched(std::integral_constant<int, CODAE_OPT_SGD>{}, std::false_type{});
    else if (kind == CODAE_OPT_LAMB) with_sched(std::integral_constant<int, CODAE_OPT_LAMB>{}, std::false_type{});
    else if (kind == CODAE_OPT_LARS) with_sched(std::integral_constant<int, CODAE_OPT_LARS>{}, std::false_type{});
    else if (kind == CODAE_OPT_ADAMW) { if (ams) with_sched(std::integral_constant<int, CODAE_OPT_ADAMW>{}, std::true_type{}); else with_sched(std::integral_constant<int, CODAE_OPT_ADAMW>{}, std::false_type{}); }
    else { if (ams) with_sched(std::integral_constant<int, CODAE_OPT_ADAM>{}, std::true_type{}); else with_sched(std::integral_constant<int, CODAE_OPT_ADAM>{}, std::false_type{}); }
}

// f(std::integral_constant<int, KIND>) for the two trust kinds
template <typename F>
void trust_dispatch(const codae_optimizer* opt, F&& f) {
    if (opt->kind == CODAE_OPT_LAMB) f(std::integral_constant<int, CODAE_OPT_LAMB>{});
    else f(std::integral_constant<int, CODAE_OPT_LARS>{});
}

// the tile table of the tiled update and of the tiled norms pass; the number of tiles, or -1 after set_error
int adam_tiles(const UpdateTiles& t, AdamTiles* jobs) {
    jobs->n_layers = t.n_layers; jobs->transposed_from = t.transposed_from; jobs->bias_off = t.bias_off; jobs->bias_n = t.bias_n;
    int total = 0;
    for (int l = 0; l < t.n_layers; ++l) {
        if (!(t.rows[l] % 8 == 0 && t.cols[l] % 4 == 0 && t.w_off[l] % 8 == 0)) {
            set_error("clip_adam_tiled: layer %d shape %d x %d", l, t.rows[l], t.cols[l]);
            return -1;
        }
        jobs->off[l] = t.w_off[l]; jobs->rows[l] = t.rows[l]; jobs->cols[l] = t.cols[l];
        jobs->tile_begin[l] = total;
        total += ((t.rows[l] + AT_R - 1) / AT_R) * ((t.cols[l] + AT_C - 1) / AT_C);
    }
    jobs->tile_begin[t.n_layers] = total;
    return total;
}

int launch_trust_finish(const UpdateLaunch& u, const TrustParts& tp, hipStream_t s) {
    float* ws = reinterpret_cast<float*>(u.opt->trust_ws);
    hipLaunchKernelGGL(trust_finish_kernel, dim3(1), dim3(64), 0, s, trust_parts(u.opt->trust_ws), tp, ws, u.opt->kind, u.opt->trust_clip,
                       u.opt->trust_coef, u.hp->weight_decay, u.hp->eps);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

}  // namespace

int launch_sumsq(const float* g, int64_t n, double* out, hipStream_t s) {
    CODAE_REQUIRE(g && out && n > 0 && a16(g), "sumsq: bad args");
    hipLaunchKernelGGL(sumsq_kernel, dim3(grid_for(n / 4 + 1)), dim3(NT), 0, s, g, n, out);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_sumsq_to(const float* g, int64_t n, double* acc, hipStream_t s) {
    CODAE_REQUIRE(g && acc && n > 0, "sumsq_to: bad args");
    int grid = grid_for(n / 4 + 1);
    if (grid > 64) grid = 64;
    hipLaunchKernelGGL(sumsq_to_kernel, dim3(grid), dim3(NT), 0, s, g, n, acc);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_clip_coef(const double* total_sq, float max_norm, double* coef_out, hipStream_t s) {
    hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(1), 0, s, total_sq, max_norm, coef_out);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_set_scalar(double* dst, double value, hipStream_t s) {
    CODAE_REQUIRE(dst != nullptr, "set_scalar: null destination");
    hipLaunchKernelGGL(set_scalar_kernel, dim3(1), dim3(1), 0, s, dst, value);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

bool optimizer_is_default(const codae_optimizer* o) {
    return o == nullptr || (o->kind == CODAE_OPT_ADAM && o->amsgrad == 0 && o->sched == CODAE_SCHED_CONSTANT && o->warmup == 0);
}

int check_optimizer(const codae_optimizer* o) {
    if (o == nullptr) return CODAE_OK;
    CODAE_REQUIRE(o->kind >= CODAE_OPT_ADAM && o->kind <= CODAE_OPT_LARS, "optimizer: unknown kind %d", o->kind);
    CODAE_REQUIRE(o->amsgrad == 0 || o->amsgrad == 1, "optimizer: amsgrad %d is neither 0 nor 1", o->amsgrad);
    CODAE_REQUIRE(o->nesterov == 0 || o->nesterov == 1, "optimizer: nesterov %d is neither 0 nor 1", o->nesterov);
    CODAE_REQUIRE(!(o->kind == CODAE_OPT_SGD && o->amsgrad), "optimizer: amsgrad belongs to adam / adamw, not to sgd");
    if (is_trust_kind(o)) {
        CODAE_REQUIRE(!o->amsgrad, "optimizer: amsgrad belongs to adam / adamw, not to %s", o->kind == CODAE_OPT_LAMB ? "lamb" : "lars");
        CODAE_REQUIRE(finite_f(o->trust_clip) && o->trust_clip >= 0.f, "optimizer: trust_clip %g is negative or not finite", (double)o->trust_clip);
        CODAE_REQUIRE(o->kind != CODAE_OPT_LARS || (finite_f(o->trust_coef) && o->trust_coef > 0.f), "optimizer: trust_coef %g is not a finite value > 0",
                      (double)o->trust_coef);
        CODAE_REQUIRE(o->decay_bias == 0 || o->decay_bias == 1, "optimizer: decay_bias %d is neither 0 nor 1", o->decay_bias);
        CODAE_REQUIRE(o->trust_ws != nullptr && a16(o->trust_ws), "optimizer: lamb / lars need a 16-byte aligned trust_ws");
    }
    CODAE_REQUIRE(finite_f(o->momentum) && o->momentum >= 0.f && o->momentum < 1.f, "optimizer: momentum %g outside [0, 1)", (double)o->momentum);
    CODAE_REQUIRE(!o->nesterov || o->momentum > 0.f, "optimizer: nesterov needs momentum > 0");
    CODAE_REQUIRE(o->sched >= CODAE_SCHED_CONSTANT && o->sched <= CODAE_SCHED_STEP, "optimizer: unknown schedule %d", o->sched);
    CODAE_REQUIRE(o->warmup >= 0, "optimizer: warmup %d < 0", o->warmup);
    if (o->sched == CODAE_SCHED_COSINE || o->sched == CODAE_SCHED_LINEAR) {
        CODAE_REQUIRE(o->total > o->warmup, "optimizer: total %d must exceed warmup %d", o->total, o->warmup);
        CODAE_REQUIRE(finite_f(o->min_factor) && o->min_factor >= 0.f && o->min_factor <= 1.f, "optimizer: min_factor %g outside [0, 1]",
                      (double)o->min_factor);
    }
    if (o->sched == CODAE_SCHED_STEP) {
        CODAE_REQUIRE(o->period >= 1, "optimizer: period %d < 1", o->period);
        CODAE_REQUIRE(finite_f(o->gamma) && o->gamma > 0.f && o->gamma <= 1.f, "optimizer: gamma %g outside (0, 1]", (double)o->gamma);
    }
    CODAE_REQUIRE(!o->amsgrad || (o->vmax != nullptr && a16(o->vmax)), "optimizer: amsgrad needs a 16-byte aligned vmax");
    return CODAE_OK;
}

// Only the fields the kind and the schedule read, everything else zero: the setter stores this form, and the graph key compares its bytes
codae_optimizer optimizer_canonical(const codae_optimizer* o) {
    codae_optimizer c{};
    if (optimizer_is_default(o)) return c;
    c.kind = o->kind; c.sched = o->sched; c.warmup = o->warmup;
    if (o->kind == CODAE_OPT_SGD || o->kind == CODAE_OPT_LARS) { c.momentum = o->momentum; c.nesterov = o->nesterov; }
    else if (o->amsgrad) { c.amsgrad = 1; c.vmax = o->vmax; }
    if (o->sched == CODAE_SCHED_COSINE || o->sched == CODAE_SCHED_LINEAR) { c.total = o->total; c.min_factor = o->min_factor; }
    if (o->sched == CODAE_SCHED_STEP) { c.period = o->period; c.gamma = o->gamma; }
    if (is_trust_kind(o)) {
        c.trust_clip = o->trust_clip; c.decay_bias = o->decay_bias; c.trust_ws = o->trust_ws;
        if (o->kind == CODAE_OPT_LARS) c.trust_coef = o->trust_coef;
    }
    return c;
}

bool weight_average_is_off(const codae_weight_average* w) { return w == nullptr || w->kind == CODAE_AVG_OFF; }

int check_weight_average(const codae_weight_average* w, bool need_avg) {
    if (weight_average_is_off(w)) return CODAE_OK;
    CODAE_REQUIRE(w->kind == CODAE_AVG_EMA || w->kind == CODAE_AVG_SWA, "weight average: unknown kind %d", w->kind);
    if (w->kind == CODAE_AVG_EMA) {
        CODAE_REQUIRE(finite_f(w->decay) && w->decay >= 0.f && w->decay < 1.f, "weight average: decay %g outside [0, 1)", (double)w->decay);
        CODAE_REQUIRE(w->debias == 0 || w->debias == 1, "weight average: debias %d is neither 0 nor 1", w->debias);
    }
    CODAE_REQUIRE(w->start >= 1, "weight average: start %d < 1", w->start);
    CODAE_REQUIRE(w->every >= 1, "weight average: every %d < 1", w->every);
    CODAE_REQUIRE(!need_avg || (w->avg != nullptr && a16(w->avg)), "weight average: avg must be a 16-byte aligned device vector");
    return CODAE_OK;
}

// Only the fields the kind reads, everything else zero: the setter stores this form, and the graph key compares its bytes
codae_weight_average weight_average_canonical(const codae_weight_average* w) {
    codae_weight_average c{};
    if (weight_average_is_off(w)) return c;
    c.kind = w->kind; c.start = w->start; c.every = w->every; c.avg = w->avg;
    if (w->kind == CODAE_AVG_EMA) { c.decay = w->decay; c.debias = w->debias; }
    return c;
}

int launch_weight_average(float* avg, const float* p, int64_t n, const codae_weight_average* wa, int32_t step, hipStream_t s) {
    CODAE_REQUIRE(wa != nullptr, "weight_average_update: null setting");
    int rc = check_weight_average(wa, false);
    if (rc) return rc;
    CODAE_REQUIRE(avg && p && n > 0 && a16(avg) && a16(p), "weight_average_update: avg and p must be 16-byte aligned, n > 0");
    CODAE_REQUIRE(step >= 1, "weight_average_update: step must be >= 1");
    float w = 1.f;
    if (weight_average_is_off(wa) || !avg_weight(wa->kind, wa->decay, wa->debias, wa->start, wa->every, step, &w)) return CODAE_OK;
    hipLaunchKernelGGL(weight_average_kernel, dim3(grid_for(n / 4 + 1)), dim3(NT), 0, s, avg, p, n, w);
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int launch_grad_sumsq(const float* g, int64_t n, double* scalars, bool clear, hipStream_t s) {
    if (clear) {
        CODAE_HIP_CHECK(hipMemsetAsync(scalars + CODAE_S_GRAD_SQ, 0, sizeof(double), s));
        CODAE_HIP_CHECK(hipMemsetAsync(scalars + CODAE_S_GRAD_SQ_SLOTS, 0, CODAE_S_N_SLOTS * sizeof(double), s));
    }
    return launch_sumsq(g, n, scalars + CODAE_S_GRAD_SQ, s);
}

int check_update_launch(const char* who, const UpdateLaunch& u) {
    const ParamVectors& x = u.x;
    const bool sgd = !optimizer_is_default(u.opt) && (u.opt->kind == CODAE_OPT_SGD || u.opt->kind == CODAE_OPT_LARS);    // (no v)
    const bool ams = !optimizer_is_default(u.opt) && u.opt->amsgrad != 0;
    CODAE_REQUIRE(x.p && x.g && x.m && (x.v || sgd) && u.hp && u.n > 0, "%s: bad args", who);
    CODAE_REQUIRE(weight_average_is_off(u.wa) || (x.avg != nullptr && a16(x.avg)), "%s: the weight average needs a 16-byte aligned avg", who);
    CODAE_REQUIRE(a16(x.p) && a16(x.g) && a16(x.m) && (sgd || a16(x.v)), "%s: buffers must be 16-byte aligned", who);
    CODAE_REQUIRE(!ams || (x.vmax != nullptr && a16(x.vmax)), "%s: amsgrad needs a 16-byte aligned vmax", who);
    CODAE_REQUIRE(u.hp->step >= 1, "%s: step must be >= 1", who);
    CODAE_REQUIRE(u.hp->max_grad_norm <= 0.f || u.grad_sq || u.coef_in, "%s: clipping needs the grad_sq scalar", who);
    CODAE_REQUIRE(!is_trust_kind(u.opt) || (u.opt->trust_ws != nullptr && a16(u.opt->trust_ws)), "%s: lamb / lars need a 16-byte aligned trust_ws", who);
    return CODAE_OK;
}

int launch_update(const UpdateLaunch& u, hipStream_t s) {
    int rc = check_update_launch("clip_adam", u);
    if (rc) return rc;
    const ParamVectors& x = u.x;
    const AdamConst c = adam_const(u.hp);
    const OptConst o = opt_const(u.opt, u.hp);
    const AvgConst ac = avg_const(u.wa, x.avg);
    const TrustConst tr = trust_const(u.opt, u.trust_mat);
    opt_dispatch(u.opt, !weight_average_is_off(u.wa), [&](auto K, auto A, auto S, auto V) {
        hipLaunchKernelGGL((clip_adam_kernel<decltype(K)::value, decltype(A)::value, decltype(S)::value, decltype(V)::value>),
                           dim3(grid_for(u.n / 4 + 1)), dim3(NT), 0, s, x.p, x.g, x.m, x.v, u.n, c, u.grad_sq, x.shadow, u.coef_in, u.step_dev, x.vmax, o, ac, tr);
    });
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

int64_t trust_parts_flat(int64_t n) { return (n + TRUST_CHUNK - 1) / TRUST_CHUNK; }
int64_t trust_parts_tiled(int rows, int cols) { return (int64_t)((rows + AT_R - 1) / AT_R) * ((cols + AT_C - 1) / AT_C); }

// the flat norms pass over the matrices [off[l], off[l] + len[l]) of x and the finish: ratios of matrices 0 .. n_mats - 1
int launch_trust_norms(const UpdateLaunch& u, int n_mats, const int64_t* off, const int64_t* len, hipStream_t s) {
    int rc = check_update_launch("trust_norms", u);
    if (rc) return rc;
    CODAE_REQUIRE(is_trust_kind(u.opt) && n_mats >= 1 && n_mats <= CODAE_TRUST_MAX_MATRICES, "trust_norms: %d matrices (at most %d)", n_mats,
                  CODAE_TRUST_MAX_MATRICES);
    const AdamConst c = adam_const(u.hp);
    const OptConst o = opt_const(u.opt, u.hp);
    double* parts = trust_parts(u.opt->trust_ws);
    TrustParts tp{};
    tp.n_mats = n_mats;
    int64_t total = 0;
    for (int l = 0; l < n_mats; ++l) {
        CODAE_REQUIRE(len[l] > 0 && off[l] % 4 == 0, "trust_norms: matrix %d at %lld, %lld elements", l, (long long)off[l], (long long)len[l]);
        const int64_t blocks = trust_parts_flat(len[l]);
        CODAE_REQUIRE(total + blocks < (int64_t)1 << 30, "trust_norms: too many partial sums");
        tp.begin[l] = (int)total;
        const ParamVectors x = u.x.at(off[l]);
        double* out = parts + 2 * total;
        const int64_t n = len[l];
        trust_dispatch(u.opt, [&](auto K) {
            hipLaunchKernelGGL((trust_norms_kernel<decltype(K)::value>), dim3((unsigned)blocks), dim3(NT), 0, s, x.p, x.g, x.m, x.v, n, c, u.grad_sq,
                               u.coef_in, u.step_dev, o, out);
        });
        CODAE_LAUNCH_CHECK();
        total += blocks;
    }
    tp.begin[n_mats] = (int)total;
    return launch_trust_finish(u, tp, s);
}

// the same over the tile table of the tiled update: one launch for every matrix, then the finish
int launch_trust_norms_tiled(const UpdateLaunch& u, const UpdateTiles& t, hipStream_t s) {
    int rc = check_update_launch("trust_norms_tiled", u);
    if (rc) return rc;
    CODAE_REQUIRE(is_trust_kind(u.opt) && t.n_layers >= 1 && t.n_layers <= CODAE_TRUST_MAX_MATRICES && u.coef_in == nullptr, "trust_norms_tiled: bad args");
    const AdamConst c = adam_const(u.hp);
    const OptConst o = opt_const(u.opt, u.hp);
    AdamTiles jobs;
    const int total = adam_tiles(t, &jobs);
    if (total < 0) return CODAE_E_INVALID;
    TrustParts tp{};
    tp.n_mats = t.n_layers;
    for (int l = 0; l <= t.n_layers; ++l) tp.begin[l] = jobs.tile_begin[l];
    const ParamVectors& x = u.x;
    double* parts = trust_parts(u.opt->trust_ws);
    trust_dispatch(u.opt, [&](auto K) {
        hipLaunchKernelGGL((trust_norms_tiled_kernel<decltype(K)::value>), dim3(total), dim3(NT), 0, s, x.p, x.g, x.m, x.v, c, u.grad_sq, jobs,
                           u.step_dev, o, parts);
    });
    CODAE_LAUNCH_CHECK();
    return launch_trust_finish(u, tp, s);
}

int launch_update_tiled(const UpdateLaunch& u, const UpdateTiles& t, hipStream_t s) {
    int rc = check_update_launch("clip_adam_tiled", u);
    if (rc) return rc;
    const ParamVectors& x = u.x;
    CODAE_REQUIRE(x.shadow && t.n_layers > 0 && t.n_layers <= 64 && u.coef_in == nullptr, "clip_adam_tiled: bad args");
    const AdamConst c = adam_const(u.hp);
    const OptConst o = opt_const(u.opt, u.hp);
    AdamTiles jobs;
    const int total = adam_tiles(t, &jobs);
    if (total < 0) return CODAE_E_INVALID;
    const TrustConst tr = trust_const(u.opt, -1);
    const int bias_blocks = (int)((t.bias_n + NT * 8 - 1) / (NT * 8)) > 0 ? (int)((t.bias_n + NT * 8 - 1) / (NT * 8)) : 1;
    const AvgConst ac = avg_const(u.wa, x.avg);
    opt_dispatch(u.opt, !weight_average_is_off(u.wa), [&](auto K, auto A, auto S, auto V) {
        hipLaunchKernelGGL((clip_adam_tiled_kernel<decltype(K)::value, decltype(A)::value, decltype(S)::value, decltype(V)::value>),
                           dim3(total + bias_blocks), dim3(NT), 0, s, x.p, x.g, x.m, x.v, c, u.grad_sq, x.shadow, t.shadow_t, jobs, u.step_dev, x.vmax, o, ac, tr);
    });
    CODAE_LAUNCH_CHECK();
    return CODAE_OK;
}

}  // namespace codae
