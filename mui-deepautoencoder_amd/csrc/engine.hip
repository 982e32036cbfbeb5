// The per-model engine of libcodae_hip.so and its C-ABI entry points: it chains the kernels
// into the DAE training step (script/train_dae_on_embedding.py:198-215 of the reference).
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "layer_gemm.h"
#include <dlfcn.h>
#include <rccl/rccl.h>      // types and prototypes only: the library is dlopen()ed (codae_dp_init), libcodae_hip.so does not link it

namespace codae {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static EnvToggles g_env;
static bool g_env_loaded = false;

void env_reload() {
    EnvToggles e;
    if (const char* t = getenv("CODAE_GEMM_TILE")) {
        switch (t[0]) { case 's': e.gemm_tile = 0; break; case 'q': e.gemm_tile = 3; break; case 'x': e.gemm_tile = 6; break; case 'm': e.gemm_tile = 7; break; default: break; }
    }
    if (const char* k = getenv("CODAE_WGRAD_SPLITK")) e.wgrad_splitk = atoi(k) > 0 ? atoi(k) : 0;
    if (const char* k = getenv("CODAE_GROUP_TILE")) e.group_tile = (k[0] >= '0' && k[0] <= '2') ? k[0] - '0' : -1;
    if (const char* pr = getenv("CODAE_SIDE_PRIORITY")) { e.side_priority_set = true; e.side_priority = atoi(pr); }
    e.no_wt = getenv("CODAE_NO_WT") != nullptr;
    e.single_stream = getenv("CODAE_SINGLE_STREAM") != nullptr;
    e.tail_on_side = getenv("CODAE_TAIL_ON_SIDE") != nullptr;
    e.no_fused_loss = getenv("CODAE_NO_FUSED_LOSS") != nullptr;
    e.flat_adam = getenv("CODAE_FLAT_ADAM") != nullptr;
    e.no_fused_norm = getenv("CODAE_NO_FUSED_NORM") != nullptr;
    e.no_chain = getenv("CODAE_NO_CHAIN") != nullptr;
    e.no_deep_small = getenv("CODAE_NO_DEEP_SMALL") != nullptr;
    e.no_defer_wgrad = getenv("CODAE_NO_DEFER_WGRAD") != nullptr;
    e.no_prefetch = getenv("CODAE_NO_PREFETCH") != nullptr;
    e.no_relu_bits = getenv("CODAE_NO_RELU_BITS") != nullptr;
    e.no_folded_loss_finish = getenv("CODAE_NO_FOLDED_LOSS_FINISH") != nullptr;
    e.no_dataset_image = getenv("CODAE_NO_DATASET_IMAGE") != nullptr;
    e.no_folded_bias_finish = getenv("CODAE_NO_FOLDED_BIAS_FINISH") != nullptr;
    if (const char* k = getenv("CODAE_STORE_POLICY"))
        e.store_policy = !strcmp(k, "plain") ? STORE_PLAIN : (!strcmp(k, "wt") ? STORE_WT : -1);
    if (const char* k = getenv("CODAE_F32_GEMM")) e.f32_gemm = k[0] == 'n' ? 1 : (k[0] == 'x' ? 2 : 0);
    if (const char* k = getenv("CODAE_SMALL_TILE_MAX")) e.small_tile_max = atoi(k);
    if (const char* k = getenv("CODAE_SMALL_STAGES")) e.small_stages = atoi(k) == 2 ? 2 : 4;
    g_env = e;
    g_env_loaded = true;
}

const EnvToggles& env() {
    if (!g_env_loaded) env_reload();
    return g_env;
}

}  // namespace codae

using namespace codae;

// Flat parameter layout: [W_0 | W_1 | ... | W_{L-1} | b_0 | ... | b_{L-1}], every tensor padded to
// a multiple of 64 floats (256 B) so each starts 16-B aligned and the whole vector can be swept
// 16 B per lane by the norm / Adam kernels.  Padding stays zero under Adam (g = 0, p = 0).
constexpr int CODAE_MAX_DACT = 16;

struct codae_engine {
    int L = 0;
    std::vector<int> in, out;
    // row strides of the activation / activation-gradient buffers: bf16 mode pads every width to a multiple of 64 (the K extent of
    // the GEMM that reads the buffer walks whole 64-deep tiles) with ZERO pad columns - allocated zeroed, never written - so that
    // whatever the weight operand holds past a row's real width (the head of its next row) is multiplied by 0.  fp32: the width.
    std::vector<int> in_ld, out_ld;
    std::vector<uint8_t> relu;       // 1: ReLU after layer l (the ReLU code: 1-bit masks, clamp_below, the chain kernel)
    std::vector<uint8_t> act;        // CODAE_ACT_* after layer l when it is neither NONE nor RELU (the generic-activation kernels), else 0
    std::vector<float> act_p;        // [L][3] its parameters
    int max_batch = 0, max_rows = 0;  // max_rows = max_batch rounded up to 64
    int prec = CODAE_PREC_F32;
    std::vector<int64_t> w_off, b_off;
    int64_t n_param = 0, bias_begin = 0;
    int maxw = 0;
    std::vector<int64_t> act_off;  // byte offsets of act[0..L-1] and y (index L) inside bufs->acts
    int64_t act_bytes = 0, dact_one = 0, slab_bytes = 0;
    std::vector<int64_t> bits_off;   // byte offset inside bufs->acts of the 1-bit ReLU mask of act[l] ([max_rows][in_ld[l] / 8]), or -1
    int n_dact = 3;          // rotating activation-gradient buffers: min(L + 1, CODAE_MAX_DACT)
    std::vector<int> split_k;
    // bias gradients: per layer a block of partial column-sum rows in bufs->bias_parts, filled by whichever kernel
    // produces that layer's activation gradient; parts_pending[l] = rows waiting for finish_bias (0 = none)
    std::vector<int64_t> part_off;
    int64_t part_floats = 0;
    int64_t loss_part_off = 0;       // (floats, 8-byte aligned) per-workgroup metric sums of the loss kernels
    int loss_part_cap = 0;
    bool chain_ok = false;           // narrow bf16 stack: codae_train_step may take the persistent fused chain
    // Every setting of the training steps, in the canonical form its setter builds field by field from zero: the graph key
    // compares the whole block byte by byte (padding included: zeroed at codae_create), so a setting added here reaches the key.
    struct PresCfg { const uint8_t* table; int64_t n_rows; int32_t n_slots; int32_t reserved; };
    struct DropCfg { float p[64]; uint64_t seed; int32_t on; int32_t reserved; };
    struct ImageCfg { const float* data; const void* image; int64_t n_rows; int32_t io; int32_t reserved; };
    struct ResCfg { uint8_t on[64]; void* ws; int64_t ws_bytes; int32_t any; int32_t reserved; };
    struct NormCfg { uint8_t on[64]; void* ws; int64_t ws_bytes; int32_t any; int32_t kind; float eps; int32_t reserved; };
    struct SparseCfg { void* ws; int64_t ws_bytes; int32_t on; int32_t m; int32_t keep; int32_t reserved; };
    struct VarCfg { void* ws; int64_t ws_bytes; int32_t n_var; int32_t on; };
    struct TrainCfg {
        codae_noise noise;               // input noise (codae_set_input_noise); kind NONE = off
        codae_swap swap;                 // slots and pool of CODAE_NOISE_SWAP (codae_set_swap_pool); n_slots 0 = not set
        codae_emphasis emph;             // loss emphasis (codae_set_loss_emphasis), meaningful while emph_on
        int32_t emph_on, reserved;       // (stored: {alpha 0, beta 0} is a legal "on")
        codae_recon_loss recon;          // training criterion (codae_set_recon_loss); kind MSE (all zero) = off
        codae_slot_contrast contrast;    // slot contrast on top of the criterion (codae_set_slot_contrast); weight 0 (all zero) = off
        PresCfg pres;                    // per-row slot presence (codae_set_slot_presence): table null = off
        DropCfg drop;                    // hidden dropout (codae_set_hidden_dropout): p[l] of layer l's output, all zero = off
        codae_optimizer opt;             // optimizer and schedule of the update (codae_set_optimizer); all zero = the default
        int32_t tied, tied_reserved;     // tied encoder / decoder weights (codae_set_tied_weights); 0 = off
        ImageCfg img;                    // bf16 image of the dataset (codae_set_dataset_image): image null = none
        codae_weight_average avg;        // average of the iterates kept by the update (codae_set_weight_average); all zero = off
        ResCfg res;                      // residual connections (codae_set_residual): on[l] = a skip around layer l, all zero = off
        NormCfg norm;                    // normalisation (codae_set_norm): on[l] = layer l's output is normalised, all zero = off
        SparseCfg sparse;                // sparse code (codae_set_sparse_code): the `keep` first-ranked units of layer m's output, all zero = off
        VarCfg var;                      // mixed-variable criterion (codae_set_variable_loss): the table lives at the head of ws, all zero = off
    } tc;
    bool recon_on() const { return tc.recon.kind != CODAE_LOSS_MSE; }
    bool contrast_on() const { return tc.contrast.weight != 0.f; }
    bool variable_on() const { return tc.var.on != 0; }
    // tied weights: the layers [0, n_free()) own their matrices, layer L-1-l mirrors layer l < L / 2 (tie_pairs: those pairs)
    int n_free() const { return (L + 1) / 2; }
    std::vector<codae_tie_pair> tie_pairs;
    // the loss is the plain MSE of every slot: what the chain kernel and the last forward GEMM's epilogue compute
    bool plain_mse() const { return !tc.emph_on && !recon_on() && !contrast_on() && tc.pres.table == nullptr && !variable_on(); }
    int graph_captures = 0;          // captures of codae_train_step_graph since codae_create
    // hidden dropout: the backward entry points take no batch, so a training forward leaves what they need behind: drop_live = the
    // activations in the workspace were dropped (an evaluation or drop-in forward clears it), with the batch rows, row indices and
    // step of that forward
    bool drop_live = false;
    int drop_B = 0;
    const int32_t* drop_rows = nullptr;
    int32_t drop_step = 0;
    // residual connections: where the setting's work space keeps G (offset 0, [rows][width of the skipped layer] fp32) and the
    // 1-bit mask of every skipped layer that has a ReLU or a LeakyReLU (byte offset, rows ld_bits apart; -1: none); res_bits_live =
    // the last forward was a training forward and wrote them; res_B = the rows of the backward in flight
    std::vector<int64_t> res_bits_off;
    bool res_bits_live = false;
    int res_B = 0;
    // normalisation: where the setting's work space keeps r of every normalised layer ([max_batch] fp32; byte offset, -1: none) and
    // the 1-bit mask of every normalised layer that has a ReLU or a LeakyReLU (written only when the layer has no skip: a skipped
    // layer's mask is the residual kernel's); norm_bits_live = the last forward was a training forward and wrote them
    std::vector<int64_t> norm_r_off, norm_bits_off;
    bool norm_bits_live = false;
    // sparse code: the setting's work space is the 1-bit keep mask of layer m ([max_batch] rows, ceil(out[m] / 8) bytes apart);
    // sparse_bits_live = the last forward was a training forward and wrote it
    bool sparse_bits_live = false;
    std::vector<int> parts_pending;
    // backward on two streams: the weight-gradient GEMMs (+ slab reduce) run on `side`, concurrently with
    // the data-gradient chain on the caller's stream (they only share the read-only dA_l)
    hipStream_t side = nullptr;
    hipEvent_t ev_ready[CODAE_MAX_DACT] = {}, ev_join = nullptr, ev_w[CODAE_MAX_DACT] = {};
    unsigned ready_turn = 0;        // ev_ready is used round robin: an event is re-recorded 16 hand-offs later at the earliest
    // dA buffer i is still being read by a side-stream wgrad (event ev_w[i]); kept across calls so that a backward
    // issued bucket by bucket without joins (codae_step_backward_async) stays ordered
    bool w_pending[CODAE_MAX_DACT] = {};
    bool side_dirty = false;      // side-stream work not yet joined into the caller's stream
    bool norm_scalars_zero = false;   // finish_loss of this step zeroed GRAD_SQ + its slots and nothing added since
    // optional per-launch hipEvent pairs (codae_profile_begin / _end)
    bool prof_on = false;
    uint32_t prof_mask = 0;
    int prof_n = 0;
    int prof_every = 1, prof_step = 0;   // launches are timed in every prof_every-th training step only
    // codae_train_step_graph: the captured step and what it was captured for
    hipGraphExec_t graph_exec = nullptr;
    bool capturing = false;          // inside stream capture: device-side Adam step, everything joined at the end
    struct GraphKey { codae_batch batch; codae_hyper hyper; codae_buffers bufs; TrainCfg tc; } graph_key{};
    std::vector<hipEvent_t> prof_start, prof_stop;
    std::vector<int> prof_kind;
    std::vector<int> prof_count;    // launches covered by the record (a GroupScope spans several); -1: prof_rides_along, no events
    bool prof_group = false;        // inside a GroupScope of the forward class: no per-launch pairs
    EnvToggles cfg;                         // the CODAE_* toggles as they stood at codae_create
    struct DpState* dp = nullptr;           // data parallel with a library-owned RCCL communicator (codae_dp_init), else null
    int esize() const { return prec == CODAE_PREC_BF16 ? 2 : 4; }
    int rows_for(int B) const { return prec == CODAE_PREC_BF16 ? (int)round_up(B, 64) : B; }
};

// ---- library-owned RCCL communicator ("the library owns ... (DP) the ncclComm_t") -------------------------
// RCCL is resolved at run time - the copy torch already loaded when there is one (soname librccl.so.1), else the system's - so
// that libcodae_hip.so loads on a box without it and a process never holds two RCCLs.
struct RcclApi {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
static RcclApi g_rccl;

static int rccl_load() {
    if (g_rccl.lib != nullptr) return CODAE_OK;
    void* lib = nullptr;
    for (const char* name : {"librccl.so.1", "librccl.so"}) {
        lib = dlopen(name, RTLD_NOW | RTLD_NOLOAD | RTLD_LOCAL);            // already in the process (torch's)
        if (lib != nullptr) break;
    }
    if (lib == nullptr)
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (lib != nullptr) break;
        }
    if (lib == nullptr) { codae::set_error("codae_dp: librccl.so not found (%s)", dlerror()); return CODAE_E_UNSUPPORTED; }
    RcclApi a;
    a.lib = lib;
    a.GetUniqueId = reinterpret_cast<decltype(a.GetUniqueId)>(dlsym(lib, "ncclGetUniqueId"));
    a.CommInitRank = reinterpret_cast<decltype(a.CommInitRank)>(dlsym(lib, "ncclCommInitRank"));
    a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(dlsym(lib, "ncclCommDestroy"));
    a.AllReduce = reinterpret_cast<decltype(a.AllReduce)>(dlsym(lib, "ncclAllReduce"));
    a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
    if (!a.GetUniqueId || !a.CommInitRank || !a.CommDestroy || !a.AllReduce || !a.GetErrorString) {
        codae::set_error("codae_dp: librccl.so lacks an entry point");
        return CODAE_E_UNSUPPORTED;
    }
    g_rccl = a;
    return CODAE_OK;
}

#define CODAE_RCCL_CHECK(expr)                                                                         \
    do {                                                                                               \
        ncclResult_t r_ = (expr);                                                                      \
        if (r_ != ncclSuccess) {                                                                       \
            codae::set_error("%s failed: %s (%s:%d)", #expr, g_rccl.GetErrorString(r_), __FILE__, __LINE__); \
            return CODAE_E_HIP;                                                                        \
        }                                                                                              \
    } while (0)

constexpr int CODAE_DP_MAX_BUCKETS = 64;
struct DpState {
    ncclComm_t comm = nullptr;
    int rank = 0, world = 1;
    hipStream_t stream = nullptr;                       // the collectives' own stream (highest priority: its own queue pool)
    hipEvent_t ev_bucket[CODAE_DP_MAX_BUCKETS + 1] = {};   // bucket i's gradients complete (+ the bias block)
    hipEvent_t ev_done = nullptr;                       // every collective of the step complete
};

namespace {

// the next record of the launch profile for a launch of class `kind`, counted as `count` launches; -1: not profiled
int prof_take_slot(codae_engine* e, int kind, int count) {
    if (!(e->prof_on && ((e->prof_mask >> kind) & 1u) && (e->prof_step % e->prof_every) == 0 && e->prof_n < (int)e->prof_start.size())) return -1;
    const int slot = e->prof_n++;
    e->prof_kind[slot] = kind;
    e->prof_count[slot] = count;
    return slot;
}

// records a start/stop event pair around the launches made while it is alive
struct ProfScope {
    codae_engine* e;
    hipStream_t s;
    int slot = -1;
    ProfScope(codae_engine* e_, int kind, hipStream_t s_) : e(e_), s(s_) {
        if (e->prof_group && kind == CODAE_K_GEMM_FWD) return;
        slot = prof_take_slot(e, kind, 1);
        if (slot >= 0) (void)hipEventRecord(e->prof_start[slot], s);
    }
    // the launches made inside count as `n` of this class (a grouped launch: one record, reported as n launches of elapsed / n)
    void counts_as(int n) { if (slot >= 0) e->prof_count[slot] = n; }
    ~ProfScope() {
        if (slot >= 0) (void)hipEventRecord(e->prof_stop[slot], s);
    }
};

// One event pair around a run of back-to-back launches of one class on one stream (the forward layers of a
// step: dependent kernels, zero gap between them): the pair's own cost (2-4 us of stream time) is paid once per run
// instead of once per launch, and the per-launch figure (elapsed / launches) is within 0.3 us of rocprofv3's.
struct GroupScope {
    codae_engine* e;
    hipStream_t s;
    int slot = -1;
    GroupScope(codae_engine* e_, int kind, hipStream_t s_) : e(e_), s(s_) {
        slot = prof_take_slot(e, kind, 0);
        if (slot >= 0) { e->prof_group = true; (void)hipEventRecord(e->prof_start[slot], s); }
    }
    void launched() { if (slot >= 0) ++e->prof_count[slot]; }
    void close() {
        if (slot >= 0) { (void)hipEventRecord(e->prof_stop[slot], s); e->prof_group = false; slot = -1; }
    }
    ~GroupScope() { close(); }
};

// A class of work that has no launch of its own in this step because it rides in the launch recorded just before it (the bias finish
// inside the grouped weight-gradient launch): one record of that class with 0 ms and no event pair, where the host would have issued
// the launch - the profile keeps listing every class of the step in issue order, and the carrying launch keeps its whole time.
void prof_rides_along(codae_engine* e, int kind) { (void)prof_take_slot(e, kind, -1); }

// exact-fp32 weight gradient (128 x 128 tiles, two workgroups per CU): enough K ranges for ~1.5 workgroups per CU - a
// 1536 x 1536 gradient is 144 tiles, whose 8192-row reductions were the critical path of the whole backward (0.97 ms per
// layer on the side stream); never for batches of <= 1024 rows
int choose_split_k_f32(int N, int K, int rows) {
    if (env().wgrad_splitk > 0) return env().wgrad_splitk <= rows / 32 ? env().wgrad_splitk : 1;
    if (rows <= 1024) return 1;
    const int tiles = tile_count(N, K, TILE_128x128);
    if (env().f32_gemm != 1 && N % 4 == 0 && K % 4 == 0) {
        // the bf16-plane kernel (gemm_f32x3.hip) runs ONE workgroup per CU: the split that leaves the last round of 256 fullest
        // (1536 x 1536: 144 tiles x 7 = 1008 of 1024 slots), at least 8 K-tiles per range, the smallest such split on a tie
        int best = 1;
        double best_fill = 0.0;
        for (int s = 1; s <= 8 && s <= rows / 256; ++s) {
            const int wgs = tiles * s, rounds = ceil_div(wgs, 256);
            const double fill = (double)wgs / (256.0 * rounds);
            if (fill > best_fill + 0.02) { best_fill = fill; best = s; }
        }
        return best;
    }
    int s = (384 + tiles / 2) / tiles;
    if (s > 8) s = 8;
    if (s > rows / 256) s = rows / 256;
    return s < 1 ? 1 : s;
}

inline void* act_ptr(codae_engine* e, const codae_buffers* b, int l) {
    return reinterpret_cast<char*>(b->acts) + e->act_off[l];
}
inline float* part_ptr(codae_engine* e, const codae_buffers* b, int l) { return b->bias_parts + e->part_off[l]; }
inline double* loss_parts_ptr(codae_engine* e, const codae_buffers* b) {
    return reinterpret_cast<double*>(b->bias_parts + e->loss_part_off);
}
inline void* dact_ptr(codae_engine* e, const codae_buffers* b, int l) {
    return reinterpret_cast<char*>(b->dacts) + (int64_t)(l % e->n_dact) * e->dact_one;   // see backward_range
}

// 1 / (rows x io) of the MSE mean: the global batch rows when a data-parallel caller gives them, else this batch's
double loss_inv_n(const codae_hyper* hyper, const codae_batch* batch) {
    const float rows = hyper != nullptr && hyper->loss_scale_rows > 0.f ? hyper->loss_scale_rows : (float)batch->B;
    return 1.0 / ((double)rows * batch->io);
}

// the step's metric sums and loss (this batch's own mean) from the `parts` per-workgroup sums of its loss kernel
int finish_loss(codae_engine* e, const codae_buffers* b, const codae_batch* batch, int parts, hipStream_t s) {
    return launch_finish_loss(b->scalars, 1.0 / ((double)batch->B * batch->io), s, loss_parts_ptr(e, b), parts);
}

// layer l's GEMMs on the engine's buffers (layer_gemm.h)
// forward: K = the PADDED input width: the extra k columns are zeros in x (see in_ld) times the head of W's next row
GemmBf16 layer_fwd_bf16(codae_engine* e, const codae_buffers* b, int l, const void* x, void* y, int64_t ldy, bool y_f32, int rows) {
    return fwd_gemm_bf16(x, e->in_ld[l], reinterpret_cast<const bf16_t*>(b->shadow_w) + e->w_off[l], e->in[l], y, ldy, y_f32 ? 1 : 0, rows,
                         e->out[l], e->in_ld[l], b->params + e->b_off[l]);
}
// weight gradient dW_l = dA_l^T act[l] over `rows` batch rows, unsplit, into grads
GemmBf16 layer_wgrad_bf16(codae_engine* e, const codae_buffers* b, int l, int rows) {
    return wgrad_gemm_bf16(dact_ptr(e, b, l), e->out_ld[l], act_ptr(e, b, l), e->in_ld[l], b->grads + e->w_off[l], rows, e->out[l], e->in[l]);
}
GemmF32 layer_wgrad_f32(codae_engine* e, const codae_buffers* b, int l, int rows) {
    return wgrad_gemm_f32(reinterpret_cast<const float*>(dact_ptr(e, b, l)), reinterpret_cast<const float*>(act_ptr(e, b, l)),
                          b->grads + e->w_off[l], rows, e->out[l], e->in[l]);
}

int check_common(codae_handle h, const codae_buffers* b, int B) {
    CODAE_REQUIRE(h != nullptr && b != nullptr, "null handle or buffers");
    CODAE_REQUIRE(B > 0 && B <= h->max_batch, "batch %d outside (0, %d]", B, h->max_batch);
    CODAE_REQUIRE(b->params && b->acts, "params/acts buffer missing");
    CODAE_REQUIRE(h->prec != CODAE_PREC_BF16 || b->shadow_w, "bf16 mode needs shadow_w");
    return CODAE_OK;
}

// The pending bias-finish jobs of the layers from `from` on, at most `cap` of them, into t - BiasFinishJobs or BiasFold: the same
// members, two structs because the second travels in a kernel-argument block.  The rows taken are no longer pending; returns the
// layer the walk stopped at.
template <typename Table>
int take_bias_jobs(codae_engine* e, const codae_buffers* b, int from, int cap, Table& t) {
    t.n = 0;
    int cols = 0, l = from;
    for (; l < e->L && t.n < cap; ++l) {
        if (e->parts_pending[l] <= 0) continue;
        t.parts[t.n] = part_ptr(e, b, l);
        t.out[t.n] = b->grads + e->b_off[l];
        t.rows[t.n] = e->parts_pending[l];
        t.cols[t.n] = e->out[l];
        t.col_begin[t.n] = cols;
        cols += e->out[l];
        ++t.n;
        e->parts_pending[l] = 0;
    }
    t.col_begin[t.n] = cols;
    return l;
}

bool bias_pending_from(const codae_engine* e, int from) {
    for (int l = from; l < e->L; ++l)
        if (e->parts_pending[l] > 0) return true;
    return false;
}

// db_l = sum of layer l's pending partial column-sum rows, in row order (every layer with pending rows, one launch);
// with_norm: += sum db^2 into the clip_grad_norm_ slots
int finish_bias(codae_engine* e, const codae_buffers* b, hipStream_t s, bool with_norm, const LossFinish* loss = nullptr) {
    double* sumsq = with_norm ? b->scalars + CODAE_S_GRAD_SQ : nullptr;
    BiasFinishJobs jobs;
    for (int l = take_bias_jobs(e, b, 0, 64, jobs); bias_pending_from(e, l); l = take_bias_jobs(e, b, l, 64, jobs)) {
        int rc = launch_bias_finish(jobs, sumsq, s);              // (more than 64 layers pending: several launches)
        if (rc) return rc;
    }
    if (jobs.n == 0) return CODAE_OK;
    ProfScope prof(e, CODAE_K_BIAS_FINISH, s);
    return launch_bias_finish(jobs, sumsq, s, loss);
}

// The same finish (with_norm / loss as finish_bias takes them) as the job table of the pipelined grouped weight-gradient launch;
// false - nothing taken, finish_bias runs as always - when there is nothing pending or more than fits
bool fold_bias_finish(codae_engine* e, const codae_buffers* b, bool with_norm, const LossFinish* loss, BiasFold* f) {
    int n = 0;
    for (int l = 0; l < e->L; ++l) n += e->parts_pending[l] > 0 ? 1 : 0;
    if (n == 0 || n > CODAE_GROUP_MAX) return false;
    *f = BiasFold{};
    take_bias_jobs(e, b, 0, CODAE_GROUP_MAX, *f);
    f->sumsq = with_norm ? b->scalars + CODAE_S_GRAD_SQ : nullptr;
    if (loss != nullptr) f->loss = *loss;
    return true;
}

// ---- the step plan: which launches a call makes, decided once ----------------------------------------------------------------
// Every entry point that issues a step, or a part of one, describes its call (StepCall) and asks step_plan; the code below it reads the
// answer and decides nothing again.  Not in the plan: whether the gather reads the bf16 image - that depends on the batch's pointers
// and alignment (gathers_from_image) - and what one call leaves behind for the next, which stays state in the handle:
// parts_pending, norm_scalars_zero, drop_live, w_pending.  The plan is derived per call, never stored (the graph key does not see it).
// (include/codae_hip.h, codae_debug_step_plan, says what every value means; the weight-gradient values are the ones they always had)
enum StepKind { STEP_TRAIN = 0, STEP_FORWARD_LOSS = 1, STEP_EVAL = 2, STEP_BACKWARD = 3, STEP_DROPIN_BACKWARD = 4, STEP_UPDATE = 5 };
struct StepCall {
    int kind, B;
    int layer_lo, layer_hi;          // the backward's range [lo, hi)
    bool join;                       // the call returns with the caller's stream waiting for the side stream
    bool want_dx, has_out_y;         // drop-in backward: an input gradient is asked for; forward: the caller takes y
    bool clip;                       // max_grad_norm > 0
};
enum { PATH_LAYERS = 0, PATH_CHAIN = 1 };
enum { LOSS_NONE = 0, LOSS_STANDALONE = 1, LOSS_FUSED = 2, LOSS_IN_CHAIN = 3 };
enum { LOSS_FINISH_NONE = 0, LOSS_FINISH_OWN = 1, LOSS_FINISH_CARRIED = 2 };
enum { WGRAD_PER_LAYER = 0, WGRAD_GROUPED_PIPE = 1, WGRAD_GROUPED_ONE_BARRIER = 2, WGRAD_GROUPED_F32 = 3 };
enum { BIAS_FINISH_NONE = 0, BIAS_FINISH_OWN = 1, BIAS_FINISH_FOLDED = 2 };
enum { NORM_NONE = 0, NORM_FROM_BACKWARD = 1, NORM_FLAT = 2 };
enum { UPDATE_NONE = 0, UPDATE_FLAT = 1, UPDATE_TILED = 2 };
struct StepPlan {
    int rows;                // rows_for(B)
    int path, loss, loss_finish, wgrad;
    int streams;             // 2: the call's per-layer weight gradients go to the side stream (a grouped schedule keeps to the caller's)
    int tail_on_caller;      // layer 0's weight gradient runs on the caller's stream (third slab buffer)
    int bias_finish, norm, update;
};

// Every 16 rows stream all the weights from L2.  Up to 128 workgroups (16 per XCD) that costs nothing extra per row: 3 x 128
// stack, ms / step chain vs per-layer: 1024 rows 0.158 / 0.31, 2048 rows 0.161 / 0.31.  With every CU streaming (4096 rows:
// 0.83 / 0.34, 8192: 1.71 / 0.40) the XCDs' L2s cannot feed them and the per-layer GEMMs (weights read once per 256 rows) win.
constexpr int CHAIN_MAX_ROWS = 2048;

bool two_streams(const codae_engine* e) { return !e->cfg.single_stream; }

// Wide bf16 stack, single-GPU fused step: every layer's weight gradient in ONE launch of 256 x 192 tiles with K = the whole batch
// (no split-K slabs, no reduce pass; sum g^2 from the epilogue), issued AFTER the data-gradient chain, which then has the chip to
// itself.  Needs dA_l of every layer alive at once (n_dact > L) and enough tiles in total to fill the chip (C3: 48 tiles per
// layer -> round 2 split K five ways: 47 MB of fp32 slabs written and read back per layer, 0.28 ms of reduce launches per step;
// all ten together: 480 tiles on 256 CUs).  Small batches gain even more: their per-layer launches are all fixed cost (3 x 512 at the
// reference's stock batch 128: 0.436 -> 0.402 ms/step; batch 512: 0.663 -> 0.433).
// Stacks too narrow to fill the chip with the big tile take the one-barrier kernel's grouped launch instead.
int grouped_wgrad_strategy(const codae_engine* e, int rows) {
    if (e->prec == CODAE_PREC_F32) {
        // the exact-fp32 engine on the bf16-plane GEMMs - every weight gradient in one launch of gemm_f32x3_grouped_kernel, K unsplit
        // (what the pipelined grouped launch is to the bf16 engine: per layer it is 144 tiles, split 7 ways into fp32 slabs and reduced:
        // 0.2 ms of reduce launches per C3 step and a prologue / epilogue per 37 K-tiles)
        if (env().f32_gemm == 1 || e->cfg.no_defer_wgrad || e->cfg.single_stream || e->L > CODAE_GROUP_MAX || e->n_dact <= e->L || rows < 256 ||
            rows % 32 != 0)
            return WGRAD_PER_LAYER;
        int total = 0;
        for (int l = 0; l < e->L; ++l) {
            if (e->in[l] % 4 != 0 || e->out[l] % 4 != 0) return WGRAD_PER_LAYER;
            total += tile_count(e->out[l], e->in[l], TILE_128x128);
        }
        return total >= 256 ? WGRAD_GROUPED_F32 : WGRAD_PER_LAYER;
    }
    if (e->prec != CODAE_PREC_BF16 || e->cfg.no_defer_wgrad || e->cfg.single_stream || e->L > CODAE_GROUP_MAX || e->n_dact <= e->L || rows < 64)
        return WGRAD_PER_LAYER;
    int total = 0, total_small = 0;
    for (int l = 0; l < e->L; ++l) {
        total += tile_count(e->out[l], e->in[l], TILE_256x192);        // (gemm_bf16_pipe_grouped)
        total_small += tile_count(e->out[l], e->in[l], TILE_64x64);     // (gemm_bf16_grouped, its smallest tile)
        if ((int64_t)rows * e->out_ld[l] * 2 >= (int64_t)1 << 32 || (int64_t)rows * e->in_ld[l] * 2 >= (int64_t)1 << 32) return WGRAD_PER_LAYER;
    }
    // (round 3 first kept the per-layer backward when one layer alone fills the chip - C5: 31.2 ms/step against 32.9 grouped; with
    //  the 4 x 8 tile order of the pipelined kernel the grouped launch wins there too: 29.5 against 30.2)
    if (total >= 200) return WGRAD_GROUPED_PIPE;
    return total_small >= 128 ? WGRAD_GROUPED_ONE_BARRIER : WGRAD_PER_LAYER;
}

// The one place that reads the engine's cfg toggles and tc settings to choose launches.  Pure: no HIP call, nothing written; the
// buffers are only tested for null (shadow_wt here; slabs and bias_parts by the launches that need them).
StepPlan step_plan(const codae_engine* e, const codae_buffers* b, const StepCall& c) {
    StepPlan p{};
    p.rows = e->rows_for(c.B);
    p.streams = 1;
    const bool bf = e->prec == CODAE_PREC_BF16;
    const bool forward = c.kind == STEP_TRAIN || c.kind == STEP_FORWARD_LOSS || c.kind == STEP_EVAL;
    const bool backward = c.kind == STEP_TRAIN || c.kind == STEP_BACKWARD || c.kind == STEP_DROPIN_BACKWARD;
    const bool training = c.kind == STEP_TRAIN || c.kind == STEP_FORWARD_LOSS;       // (the forward has a hyper)
    // (the chain kernel fuses the plain gather and the unweighted loss and keeps the activations to itself: a noised input, an
    //  emphasised loss, another criterion, hidden dropout, a skip, a norm, a sparse code or a slot-presence table takes the per-layer
    //  launches)
    if (c.kind == STEP_TRAIN && e->chain_ok && e->plain_mse() && e->tc.noise.kind == CODAE_NOISE_NONE && !e->tc.drop.on &&
        !e->tc.res.any && !e->tc.norm.any && !e->tc.sparse.on && b->shadow_wt != nullptr && p.rows <= CHAIN_MAX_ROWS) {
        // narrow stack: persistent fused chain + grouped weight gradients (4 launches for the whole step)
        p.path = PATH_CHAIN;
        p.loss = LOSS_IN_CHAIN; p.loss_finish = LOSS_FINISH_CARRIED;
        p.wgrad = WGRAD_GROUPED_ONE_BARRIER; p.bias_finish = BIAS_FINISH_OWN;
    } else {
        if (forward) {
            // bf16 training step: the loss is folded into the last forward GEMM's epilogue (y never stored)
            // (not with loss emphasis or a criterion other than the MSE: those live in stand-alone kernels)
            // (nor with a slot-presence table: the stand-alone kernels carry the predicate, the GEMM epilogue does not)
            const bool fused = bf && training && !c.has_out_y && !e->cfg.no_fused_loss && e->plain_mse();
            p.loss = fused ? LOSS_FUSED : LOSS_STANDALONE;
            // the fused step leaves the fused loss's finish - 5 us of a one-block launch plus a launch boundary between the loss GEMM
            // and the first data gradient - to the bias-finish launch that ends its backward, as the chain path does
            p.loss_finish = fused && c.kind == STEP_TRAIN && !e->cfg.no_folded_loss_finish ? LOSS_FINISH_CARRIED : LOSS_FINISH_OWN;
        }
        if (backward) {
            const bool step_mode = c.kind != STEP_DROPIN_BACKWARD;
            const bool whole = c.layer_lo == 0 && c.layer_hi == e->L;
            p.streams = two_streams(e) ? 2 : 1;
            // (the drop-in backward over the whole stack without an input gradient takes the step's schedule)
            if ((step_mode || !c.want_dx) && c.join && whole && e->L >= 2) p.wgrad = grouped_wgrad_strategy(e, p.rows);
            if (p.wgrad != WGRAD_PER_LAYER) {
                // (the pipelined grouped launch carries the bias finish - and the loss finish left to it - as trailing workgroups)
                p.bias_finish = p.wgrad == WGRAD_GROUPED_PIPE && !e->cfg.no_folded_bias_finish ? BIAS_FINISH_FOLDED : BIAS_FINISH_OWN;
            } else {
                // tail: the side stream still owes wgrad_1 when the dgrad chain ends, and the caller's stream has nothing left to do:
                // the last weight gradient runs there, beside wgrad_1
                p.tail_on_caller = p.streams == 2 && c.join && step_mode && c.layer_lo == 0 && c.layer_hi - c.layer_lo >= 3 && !e->cfg.tail_on_side;
                // A backward issued bucket by bucket without joins (data parallel: one bucket per layer) leaves the partial rows
                // pending until its LAST range (lo == 0) - one finish launch per step instead of one per bucket (10 x 6 us at C3)
                p.bias_finish = c.join || c.layer_lo == 0 ? BIAS_FINISH_OWN : BIAS_FINISH_NONE;
            }
        }
    }
    if (c.kind == STEP_TRAIN || c.kind == STEP_UPDATE) {
        // single GPU fused bf16 step: nothing happens to the gradients between backward and update, so every weight gradient leaves its
        // sum g^2 behind - split ones in the slab reduce, unsplit and grouped ones in the GEMM epilogue - and the bias finish adds db^2.
        // Tied weights: the norm is that of the FOLDED gradients - the flat pass
        const bool from_backward = c.kind == STEP_TRAIN && bf && !e->cfg.no_fused_norm && !e->tc.tied;
        p.norm = !c.clip ? NORM_NONE : (from_backward ? NORM_FROM_BACKWARD : NORM_FLAT);
        p.update = bf && b->shadow_wt != nullptr && e->L <= 64 && !e->cfg.flat_adam ? UPDATE_TILED : UPDATE_FLAT;
    }
    return p;
}

StepCall update_call(const codae_hyper* hyper) { return StepCall{STEP_UPDATE, 0, 0, 0, true, false, false, hyper->max_grad_norm > 0.f}; }

// gather + forward chain + loss + data-gradient chain of a narrow stack: one launch.  The loss finish is left to the caller's
// bias-finish launch - *loss_out describes it - and the kernel zeroes the norm accumulators.
int run_chain(codae_engine* e, const codae_buffers* b, const codae_batch* batch, const codae_hyper* hyper, hipStream_t s, LossFinish* loss_out) {
    const int B = batch->B, L = e->L, rows = e->rows_for(B);
    ChainArgs a{};
    a.L = L; a.rows = rows; a.B = B;
    for (int l = 0; l < L; ++l) {
        a.width[l] = e->in[l];
        if (e->relu[l]) a.relu_flags |= 1u << l;
        a.W[l] = reinterpret_cast<const bf16_t*>(b->shadow_w) + e->w_off[l];
        a.Wt[l] = reinterpret_cast<const bf16_t*>(b->shadow_wt) + e->w_off[l];
        a.bias[l] = b->params + e->b_off[l];
        a.act[l] = reinterpret_cast<bf16_t*>(act_ptr(e, b, l));
        a.dact[l] = reinterpret_cast<bf16_t*>(dact_ptr(e, b, l));
        a.colsum_part[l] = part_ptr(e, b, l);
    }
    a.width[L] = e->out[L - 1];
    a.data = batch->data; a.row_idx = batch->row_idx; a.mask_id = batch->mask_id; a.mask_table = batch->mask_table;
    a.mask_to_use = batch->mask_to_use; a.nb_run = batch->nb_run; a.run = batch->run;
    a.inv_n = (float)loss_inv_n(hyper, batch);
    a.loss_parts = loss_parts_ptr(e, b);
    a.do_backward = 1;
    a.scalars = b->scalars;
    const int n_wg = rows / chain_rows_per_workgroup();
    CODAE_REQUIRE(n_wg <= e->loss_part_cap, "chain: %d workgroups exceed the partial-sum rows (%d)", n_wg, e->loss_part_cap);
    int rc;
    {
        ProfScope prof(e, CODAE_K_CHAIN, s);
        rc = launch_chain_step(a, s);
    }
    if (rc) return rc;
    for (int l = 0; l < L; ++l) e->parts_pending[l] = n_wg;
    e->norm_scalars_zero = true;
    loss_out->scalars = b->scalars; loss_out->inv_n = 1.0 / ((double)B * batch->io);
    loss_out->parts = loss_parts_ptr(e, b); loss_out->n_parts = n_wg;
    return CODAE_OK;
}

// Every layer's weight gradient dW_l = dA_l^T H_l, K unsplit, fp32 straight into grads, in one grouped launch per CODAE_GROUP_MAX layers
// of the kernel p.wgrad names.  NORM_FROM_BACKWARD: each bf16 tile also adds its sum g^2 to the clip_grad_norm_ slots.  The one-barrier
// kernel takes the layers in ascending order, one profile record per launch; the other two in backward order (the layers whose operands
// were touched last come first), a launch reported as one record per layer.  fold: the bias finish riding in the pipelined launch.
int run_wgrad_grouped(codae_engine* e, const codae_buffers* b, const StepPlan& p, hipStream_t s, const BiasFold* fold = nullptr) {
    const bool ascending = p.wgrad == WGRAD_GROUPED_ONE_BARRIER;
    double* sumsq_slots = p.norm == NORM_FROM_BACKWARD ? b->scalars + CODAE_S_GRAD_SQ_SLOTS : nullptr;
    for (int base = 0; base < e->L; base += CODAE_GROUP_MAX) {
        const int n = e->L - base < CODAE_GROUP_MAX ? e->L - base : CODAE_GROUP_MAX;
        auto layer = [&](int i) { return ascending ? base + i : e->L - 1 - base - i; };
        int rc;
        if (p.wgrad == WGRAD_GROUPED_F32) {
            GemmF32Group grp{};
            for (grp.n = 0; grp.n < n; ++grp.n) grp.g[grp.n] = layer_wgrad_f32(e, b, layer(grp.n), p.rows);
            ProfScope prof(e, CODAE_K_GEMM_WGRAD, s);
            prof.counts_as(n);
            rc = gemm_f32x3_grouped(grp, s);
        } else {
            GemmBf16Group grp{};
            for (grp.n = 0; grp.n < n; ++grp.n) {
                grp.g[grp.n] = layer_wgrad_bf16(e, b, layer(grp.n), p.rows);
                grp.g[grp.n].sumsq_slots = sumsq_slots;
            }
            ProfScope prof(e, CODAE_K_GEMM_WGRAD, s);
            if (!ascending) prof.counts_as(n);
            rc = ascending ? gemm_bf16_grouped(grp, s) : gemm_bf16_pipe_grouped(grp, s, fold);
        }
        if (rc) return rc;
    }
    return CODAE_OK;
}

// What ends a backward whose data gradients are complete on s (the chain kernel's, or the per-layer chain of a grouped schedule): the
// grouped weight gradients, then the bias finish - with the loss finish left to it - in that launch or behind it
int run_grouped_tail(codae_engine* e, const codae_buffers* b, const StepPlan& p, hipStream_t s, const LossFinish* loss) {
    const bool with_norm = p.norm == NORM_FROM_BACKWARD;
    BiasFold fold;
    const bool folded = p.bias_finish == BIAS_FINISH_FOLDED && fold_bias_finish(e, b, with_norm, loss, &fold);
    int rc = run_wgrad_grouped(e, b, p, s, folded ? &fold : nullptr);
    if (rc) return rc;
    if (folded) { prof_rides_along(e, CODAE_K_BIAS_FINISH); return CODAE_OK; }
    return finish_bias(e, b, s, with_norm, loss);
}
// Exact-fp32 GEMM of a launch too small to fill the chip (forward / data gradient of a small batch): K split over
// workgroups into fp32 slabs (slab slot 2: the caller's stream), then the reduce that applies the GEMM's epilogue.  Same
// fp32 arithmetic in another summation order.  3 x 512 at batch 128, whole parity-mode step: 3.09 -> see DESIGN.md.
int gemm_f32_small(codae_engine* e, const codae_buffers* b, const GemmF32& g, hipStream_t s) {
    const int tiles = tile_count(g.M, g.N, TILE_128x128);
    const int kt = (g.K + 31) / 32;
    int S = tiles >= 128 ? 1 : (256 + tiles / 2) / tiles;
    if (S > kt / 4) S = kt / 4;                       // at least 4 K-tiles per range
    if (S > 16) S = 16;
    while (S > 1 && (int64_t)S * g.M * g.N * 4 > e->slab_bytes) --S;
    if (S <= 1 || b->slabs == nullptr || e->cfg.no_deep_small || (g.N % 4) != 0 || (g.ldc % 4) != 0 || g.m_dev != nullptr ||
        (g.relu_src != nullptr && (g.ld_relu % 4) != 0))
        return gemm_f32(g, s);
    float* slab = reinterpret_cast<float*>(reinterpret_cast<char*>(b->slabs) + 2 * e->slab_bytes);
    GemmF32 p = g;
    p.C = slab; p.ldc = g.N; p.bias = nullptr; p.relu = 0; p.relu_src = nullptr; p.ld_relu = 0; p.colsum_part = nullptr; p.split_k = S;
    p.act = CODAE_ACT_NONE;
    int rc = gemm_f32(p, s);
    if (rc) return rc;
    return launch_reduce_slabs_epi(slab, S, (int64_t)g.M * g.N, g.M, g.N, g.C, g.ldc, g.bias, g.relu, g.relu_src, g.ld_relu, g.colsum_part, s,
                                   g.act, g.act_p);
}

// y = act(x W^T + b) for layer l
int run_linear(codae_engine* e, const codae_buffers* b, int l, const void* x, void* y, bool y_f32, int rows,
               hipStream_t s) {
    const int N = e->out[l], K = e->in[l];
    ProfScope prof(e, CODAE_K_GEMM_FWD, s);
    if (e->prec == CODAE_PREC_BF16) {
        GemmBf16 g = layer_fwd_bf16(e, b, l, x, y, y_f32 ? N : e->out_ld[l], y_f32, rows);
        set_activation(g, e->relu[l], e->act[l], &e->act_p[3 * l]);
        if (!y_f32 && l + 1 < e->L && e->bits_off[l + 1] >= 0 && e->relu[l] && y == act_ptr(e, b, l + 1) && gemm_bf16_takes_relu_bits(rows, N)) {
            g.relu_bits_out = reinterpret_cast<uint8_t*>(b->acts) + e->bits_off[l + 1];
            g.ld_bits = e->in_ld[l + 1] / 8;
        }
        if (l + 1 < e->L && !e->cfg.no_prefetch) {        // the next layer's weights, touched under this launch's epilogue
            g.prefetch = reinterpret_cast<const bf16_t*>(b->shadow_w) + e->w_off[l + 1];
            g.prefetch_bytes = (int64_t)e->in[l + 1] * e->out[l + 1] * 2;
        }
        return gemm_bf16(g, s);
    }
    GemmF32 g = fwd_gemm_f32(reinterpret_cast<const float*>(x), b->params + e->w_off[l], reinterpret_cast<float*>(y), rows, N, K,
                             b->params + e->b_off[l]);
    set_activation(g, e->relu[l], e->act[l], &e->act_p[3 * l]);
    return gemm_f32_small(e, b, g, s);
}

// dW_l = dA_l^T act[l] on stream s.  bf16: split-K partial slabs (slab buffer `slot`), then the reduce on the same stream.
// with_norm (bf16): the launch that produces the final values - the slab reduce, or the unsplit GEMM's epilogue - also adds their
// sum g^2 to the clip_grad_norm_ accumulators
int run_wgrad(codae_engine* e, const codae_buffers* b, int l, int rows, bool with_norm, hipStream_t s, int slot = 0) {
    const int N = e->out[l], K = e->in[l];
    float* dW = b->grads + e->w_off[l];
    if (e->prec == CODAE_PREC_BF16) {
        const int S = e->split_k[l] <= rows / 64 ? e->split_k[l] : rows / 64;
        GemmBf16 g = layer_wgrad_bf16(e, b, l, rows);
        g.split_k = S;
        if (S > 1) {
            g.store_policy = store_policy_for((int64_t)S * N * K * 4);       // (the launch writes S slabs)
            CODAE_REQUIRE(b->slabs != nullptr, "bf16 wgrad needs the slab workspace");
            char* slab = reinterpret_cast<char*>(b->slabs) + (int64_t)slot * e->slab_bytes;
            g.C = slab;
            int rc;
            {
                ProfScope prof(e, CODAE_K_GEMM_WGRAD, s);
                rc = gemm_bf16(g, s);
            }
            if (rc) return rc;
            ProfScope prof(e, CODAE_K_SLAB_REDUCE, s);
            return launch_reduce_slabs(reinterpret_cast<const float*>(slab), S, (int64_t)N * K, dW, (int64_t)N * K,
                                       with_norm ? b->scalars + CODAE_S_GRAD_SQ : nullptr, s);
        }
        if (with_norm) g.sumsq_slots = b->scalars + CODAE_S_GRAD_SQ_SLOTS;    // (unsplit: the epilogue sees the final values)
        ProfScope prof(e, CODAE_K_GEMM_WGRAD, s);
        return gemm_bf16(g, s);
    }
    GemmF32 g = layer_wgrad_f32(e, b, l, rows);
    int S = e->split_k[l];
    if (S > rows / 32) S = rows / 32;
    if (S > 1 && b->slabs != nullptr) {
        // K split over workgroups: fp32 slabs, added in slab order by the reduce (same fp32 arithmetic, another summation order)
        float* slab = reinterpret_cast<float*>(reinterpret_cast<char*>(b->slabs) + (int64_t)slot * e->slab_bytes);
        g.C = slab; g.split_k = S;
        int rc;
        {
            ProfScope prof(e, CODAE_K_GEMM_WGRAD, s);
            rc = gemm_f32(g, s);
        }
        if (rc) return rc;
        ProfScope prof(e, CODAE_K_SLAB_REDUCE, s);
        return launch_reduce_slabs(slab, S, (int64_t)N * K, dW, (int64_t)N * K, nullptr, s);
    }
    ProfScope prof(e, CODAE_K_GEMM_WGRAD, s);
    return gemm_f32(g, s);
}

// dA_{l-1} = (dA_l W_l) * [act[l] > 0]  (+ column sums -> db_{l-1});  l == 0 with dx: plain dX in fp32
// coscheduled: another stream's weight gradients run beside this launch (GemmBf16::coscheduled)
// unmasked: dA_{l-1} = dA_l W_l alone (relu_src == relu_bits == nullptr) - the residual kernel behind it applies the derivative
int run_dgrad_gemm(codae_engine* e, const codae_buffers* b, int l, int rows, bool coscheduled, float* dx_f32, hipStream_t s,
                   bool unmasked = false) {
    const int N = e->out[l], K = e->in[l];
    const bool to_dx = (dx_f32 != nullptr);
    ProfScope prof(e, CODAE_K_GEMM_DGRAD, s);
    if (e->prec == CODAE_PREC_BF16) {
        const bool wt = b->shadow_wt != nullptr && l >= 1 && !e->cfg.no_wt;      // the transposed shadow: the forward-form kernel
        const bf16_t* W = reinterpret_cast<const bf16_t*>(wt ? b->shadow_wt : b->shadow_w) + e->w_off[l];
        // (k runs over the padded output width: zero pad columns of dA)
        GemmBf16 g = dgrad_gemm_bf16(dact_ptr(e, b, l), e->out_ld[l], W, wt ? N : K, wt, to_dx ? (void*)dx_f32 : dact_ptr(e, b, l - 1),
                                     to_dx ? K : e->out_ld[l - 1], to_dx ? 1 : 0, rows, K, e->out_ld[l]);
        g.coscheduled = coscheduled ? 1 : 0;
        if (!to_dx) {
            if (unmasked) {
                // (no mask, no derivative: the write-out the layer behind a code layer takes; the column sums it leaves are
                //  rewritten by the residual kernel)
            } else if (e->act[l - 1] != CODAE_ACT_NONE) {
                // another activation than ReLU: its derivative from the saved activation (no 1-bit masks for these layers)
                g.relu_src = reinterpret_cast<const bf16_t*>(act_ptr(e, b, l)); g.ld_relu = e->in_ld[l];
                set_activation(g, 0, e->act[l - 1], &e->act_p[3 * (l - 1)]);
            } else if (e->relu[l - 1]) {
                g.relu_src = reinterpret_cast<const bf16_t*>(act_ptr(e, b, l)); g.ld_relu = e->in_ld[l];
                // (the forward launch that wrote act[l] had this output shape: rows x in[l]; same predicate on both sides)
                if (e->bits_off[l] >= 0 && gemm_bf16_takes_relu_bits(rows, K)) {
                    g.relu_bits = reinterpret_cast<const uint8_t*>(b->acts) + e->bits_off[l];
                    g.ld_bits = e->in_ld[l] / 8;
                }
            }
            g.colsum_part = part_ptr(e, b, l - 1);
            e->parts_pending[l - 1] = gemm_bf16_colsum_rows(g);
            if (b->shadow_wt != nullptr && l >= 2 && !e->cfg.no_wt && !e->cfg.no_prefetch) {      // the next data gradient's operand
                g.prefetch = reinterpret_cast<const bf16_t*>(b->shadow_wt) + e->w_off[l - 1];
                g.prefetch_bytes = (int64_t)e->in[l - 1] * e->out[l - 1] * 2;
            }
        }
        return gemm_bf16(g, s);
    }
    GemmF32 g = dgrad_gemm_f32(reinterpret_cast<const float*>(dact_ptr(e, b, l)), b->params + e->w_off[l],
                               to_dx ? dx_f32 : reinterpret_cast<float*>(dact_ptr(e, b, l - 1)), rows, N, K);
    if (!to_dx) {
        if (!unmasked && (e->relu[l - 1] || e->act[l - 1] != CODAE_ACT_NONE)) {
            g.relu_src = reinterpret_cast<const float*>(act_ptr(e, b, l)); g.ld_relu = K;
            set_activation(g, 0, e->act[l - 1], &e->act_p[3 * (l - 1)]);
        }
        g.colsum_part = part_ptr(e, b, l - 1);
        e->parts_pending[l - 1] = gemm_f32_colsum_rows(rows);
    }
    return gemm_f32_small(e, b, g, s);
}

// step of the dropout counter: the forward's, or under graph capture the device scalar the replay refreshes
// the step count as the kernels of a captured step read it: from the device scalar (kernel arguments are frozen at capture)
inline const double* step_dev(codae_engine* e, const codae_buffers* b) { return e->capturing ? b->scalars + CODAE_S_ADAM_STEP : nullptr; }
inline bool drops_layer(codae_engine* e, int l) { return e->drop_live && e->tc.drop.on && l >= 0 && l + 1 < e->L && e->tc.drop.p[l] > 0.f; }

// act[l + 1] <- act[l + 1] * f behind the forward GEMM of a dropped layer l (its 1-bit ReLU masks stay "pre-dropout y > 0": the
// backward multiplies by f after the mask)
int run_dropout_fwd(codae_engine* e, const codae_buffers* b, int l, hipStream_t s) {
    ProfScope prof(e, CODAE_K_DROPOUT, s);
    return launch_dropout_fwd(act_ptr(e, b, l + 1), e->prec == CODAE_PREC_BF16, e->in_ld[l + 1], e->drop_B, e->out[l], e->drop_rows, l,
                              e->drop_step, step_dev(e, b), e->tc.drop.p[l], e->tc.drop.seed, s);
}

inline bool skips_layer(const codae_engine* e, int l) { return e->tc.res.any && l >= 0 && l + 1 < e->L && e->tc.res.on[l] != 0; }

// act[l + 1] <- act[l + 1] + act[l] behind the forward GEMM of a skipped layer l (and behind its dropout kernel); training: the
// 1-bit mask of the value before the add goes to the setting's work space first.
int run_residual_fwd(codae_engine* e, const codae_buffers* b, int l, int B, bool training, hipStream_t s) {
    uint8_t* bits = training && e->res_bits_off[l] >= 0 ? reinterpret_cast<uint8_t*>(e->tc.res.ws) + e->res_bits_off[l] : nullptr;
    ProfScope prof(e, CODAE_K_DROPOUT, s);
    return launch_residual_fwd(act_ptr(e, b, l + 1), act_ptr(e, b, l), e->prec == CODAE_PREC_BF16, e->in_ld[l + 1], e->in_ld[l], B, e->out[l], bits,
                               (e->out[l] + 7) / 8, s);
}

inline bool norms_layer(const codae_engine* e, int l) { return e->tc.norm.any && l >= 0 && l + 1 < e->L && e->tc.norm.on[l] != 0; }

// act[l + 1] <- N(act[l + 1]) in place behind the forward GEMM of a normalised layer l, behind its dropout and skip kernels; r goes
// to the setting's work space; training, ReLU / LeakyReLU and no skip: the 1-bit mask of the value before the norm goes there first
// (a skipped layer's residual kernel has written that mask already).
int run_norm_fwd(codae_engine* e, const codae_buffers* b, int l, int B, bool training, hipStream_t s) {
    char* ws = reinterpret_cast<char*>(e->tc.norm.ws);
    uint8_t* bits = training && !skips_layer(e, l) && e->norm_bits_off[l] >= 0 ? reinterpret_cast<uint8_t*>(ws + e->norm_bits_off[l]) : nullptr;
    ProfScope prof(e, CODAE_K_DROPOUT, s);
    return launch_norm_fwd(act_ptr(e, b, l + 1), e->prec == CODAE_PREC_BF16, e->in_ld[l + 1], B, e->out[l], e->tc.norm.kind, e->tc.norm.eps,
                           reinterpret_cast<float*>(ws + e->norm_r_off[l]), bits, (e->out[l] + 7) / 8, s);
}

inline bool sparse_layer(const codae_engine* e, int l) { return e->tc.sparse.on && l >= 0 && l + 1 < e->L && l == e->tc.sparse.m; }

// act[m + 1] <- its `keep` first-ranked units per row, +0 elsewhere, in place behind the forward GEMM of the layer m that produces
// the code (behind its dropout kernel; layer m has neither skip nor norm); training: the 1-bit keep mask goes to the setting's work space
int run_sparse_fwd(codae_engine* e, const codae_buffers* b, int l, int B, bool training, hipStream_t s) {
    ProfScope prof(e, CODAE_K_DROPOUT, s);
    return launch_sparse_code_fwd(act_ptr(e, b, l + 1), e->prec == CODAE_PREC_BF16, e->in_ld[l + 1], B, e->out[l], e->tc.sparse.keep,
                                  training ? reinterpret_cast<uint8_t*>(e->tc.sparse.ws) : nullptr, (e->out[l] + 7) / 8, s);
}

// What a forward leaves for the backward entry points, which take no batch: a training forward (hyper not null) of a stack with
// dropout, skips, a norm or a sparse code says that the activations were dropped - with the batch rows, row indices and step of that
// forward - and that the skips', the norm's and the sparse code's 1-bit masks were written; every other forward (evaluation, drop-in,
// scoring: batch and hyper null) clears the four flags.
void forward_leaves(codae_engine* e, const codae_batch* batch, const codae_hyper* hyper) {
    e->drop_live = hyper != nullptr && e->tc.drop.on;
    if (e->drop_live) { e->drop_B = batch->B; e->drop_rows = batch->row_idx; e->drop_step = hyper->step; }
    e->res_bits_live = hyper != nullptr && e->tc.res.any;
    e->norm_bits_live = hyper != nullptr && e->tc.norm.any;
    e->sparse_bits_live = hyper != nullptr && e->tc.sparse.on;
}

// The drop-in entry points' refusal of what skips, a norm or a sparse code do not allow them: "<who>: residual connections are on:
// <what>", "<who>: a norm is on: <what>", or "<who>: a sparse code is on: <what>"
int refuse_skips_or_norm(const codae_engine* e, const char* who, const char* what) {
    if (!e->tc.res.any && !e->tc.norm.any && !e->tc.sparse.on) return CODAE_OK;
    set_error("%s: %s on: %s", who, e->tc.res.any ? "residual connections are" : (e->tc.norm.any ? "a norm is" : "a sparse code is"), what);
    return CODAE_E_UNSUPPORTED;
}

// Layer l of a forward - the MODEL, in the one place every forward loop calls: the linear layer into act[l + 1] (`rows` rows) or,
// y_f32 not null, into that fp32 tensor (B rows); then dropout, the skip and the norm, in that order, where the settings put one.
// Dropout is inert unless forward_leaves recorded a dropped forward; `training`: the skip and the norm leave their 1-bit masks.
// group: the caller's run of plain forward launches, told of the GEMM.
int run_forward_layer(codae_engine* e, const codae_buffers* b, int l, float* y_f32, int B, int rows, bool training, hipStream_t s,
                      GroupScope* group = nullptr) {
    int rc = y_f32 != nullptr ? run_linear(e, b, l, act_ptr(e, b, l), y_f32, true, B, s)
                              : run_linear(e, b, l, act_ptr(e, b, l), act_ptr(e, b, l + 1), false, rows, s);
    if (rc) return rc;
    if (group != nullptr) group->launched();
    if (drops_layer(e, l)) {
        rc = run_dropout_fwd(e, b, l, s);
        if (rc) return rc;
    }
    if (skips_layer(e, l)) {
        rc = run_residual_fwd(e, b, l, B, training, s);
        if (rc) return rc;
    }
    if (norms_layer(e, l)) {
        rc = run_norm_fwd(e, b, l, B, training, s);
        if (rc) return rc;
    }
    return sparse_layer(e, l) ? run_sparse_fwd(e, b, l, B, training, s) : CODAE_OK;
}

// the data gradient of layer l and, when layer l - 1 was dropped in the forward, dA_{l-1} <- dA_{l-1} * f right behind it on the same
// stream: the kernel writes layer l - 1's partial column sums again, from the final values, in place of the GEMM epilogue's (one row
// per 64 batch rows: within the rows the layer owns), before the caller records the event the side-stream weight gradient waits for
// With a skip around layer l or around layer l - 1 (codae_residual) the GEMM runs unmasked and the residual kernel sits between it and
// dropout's: G_l = U_l + skip_l G_{l+1}, kept for the next level when layer l - 1 is skipped too, dA_{l-1} <- G_l * act'_{l-1} and its
// partial column sums.  act'_{l-1} comes from the 1-bit mask the forward skip kernel wrote when layer l - 1 is skipped (act[l] then
// holds a_{l-1} + h_{l-1}), else from the saved activation act[l], as the GEMM epilogue takes it.
// With a norm on layer l - 1 (codae_norm) the GEMM runs unmasked as well and the norm backward kernel takes the residual kernel's place
// and does its whole job: Gh = U_l + skip_l G, Gs_{l-1} from Gh, xhat = act[l] and r, G <- Gs_{l-1} when layer l - 1 is skipped too,
// dA_{l-1} <- Gs_{l-1} * act'_{l-1} from the 1-bit mask (the residual's when layer l - 1 is skipped, else the norm's), the column sums.
int run_dgrad(codae_engine* e, const codae_buffers* b, int l, int rows, bool coscheduled, float* dx_f32, hipStream_t s) {
    const bool nrm = dx_f32 == nullptr && l >= 1 && norms_layer(e, l - 1);
    const bool res = dx_f32 == nullptr && l >= 1 && (nrm || skips_layer(e, l) || skips_layer(e, l - 1));
    int rc = run_dgrad_gemm(e, b, l, rows, coscheduled, dx_f32, s, res);
    if (rc || dx_f32 != nullptr) return rc;
    if (res) {
        // a streaming kernel takes over the derivative at this site: the norm's when layer m is normalised, else the residual's
        const bool bf = e->prec == CODAE_PREC_BF16;
        const int m = l - 1;                                     // the layer whose derivative is applied
        const int kind = e->relu[m] ? CODAE_ACT_RELU : (int)e->act[m];
        const bool from_skip = skips_layer(e, m);
        float* G = reinterpret_cast<float*>(e->tc.res.ws);
        StreamBwd c{};
        c.g_in = skips_layer(e, l) ? G : nullptr;
        c.g_out = from_skip && m >= 1 ? G : nullptr;             // (layer 0's input gradient is never formed)
        c.ld_g = e->in[l];
        c.act_kind = kind;
        c.slope = e->act_p[3 * m];
        // act' from the 1-bit mask a training forward left: the skip kernel's when layer m is skipped (act[l] then holds a_m + h_m),
        // else the norm kernel's (act[l] holds xhat); a layer with neither takes it from the saved activation act[l], as the GEMM
        // epilogue does
        if ((nrm || from_skip) && kind != CODAE_ACT_NONE) {
            CODAE_REQUIRE(from_skip ? e->res_bits_live : e->norm_bits_live, "backward through the %s of layer %d without a training forward before it",
                          nrm ? "norm" : "skip", m);
            const int64_t off = from_skip ? e->res_bits_off[m] : e->norm_bits_off[m];
            CODAE_REQUIRE(off >= 0, "backward through the %s of layer %d: no 1-bit mask for activation kind %d", nrm ? "norm" : "skip", m, kind);
            c.bits = reinterpret_cast<const uint8_t*>(from_skip ? e->tc.res.ws : e->tc.norm.ws) + off;
            c.ld_bits = (e->out[m] + 7) / 8;
        }
        const int64_t ld = bf ? e->out_ld[m] : e->out[m];
        {
            ProfScope prof(e, CODAE_K_DROPOUT, s);
            if (nrm) {
                const NormBwd n{c, act_ptr(e, b, l), e->in_ld[l], reinterpret_cast<const float*>(reinterpret_cast<const char*>(e->tc.norm.ws) + e->norm_r_off[m])};
                rc = launch_norm_bwd(dact_ptr(e, b, m), bf, ld, e->res_B, e->out[m], e->tc.norm.kind, n, part_ptr(e, b, m), s);
            } else {
                const bool from_act = !from_skip && kind != CODAE_ACT_NONE;
                const ResidualBwd r{c, from_act ? act_ptr(e, b, l) : nullptr, from_act ? e->in_ld[l] : 0,
                                    {e->act_p[3 * m], e->act_p[3 * m + 1], e->act_p[3 * m + 2]}};
                rc = launch_residual_bwd(dact_ptr(e, b, m), bf, ld, e->res_B, e->out[m], r, part_ptr(e, b, m), s);
            }
        }
        if (rc) return rc;
        e->parts_pending[m] = row_sweep_blocks(e->res_B);
    }
    if (sparse_layer(e, l - 1)) {
        // dA_m <- kept ? dA_m : +0 behind the GEMM (and behind the residual kernel of a skip around layer l: layer m itself has
        // neither skip nor norm, so that kernel's only outputs here are dA_m and its column sums, and the selection commutes with
        // the element-wise derivative), in front of dropout's kernel; the partial column sums are rewritten from the final values
        CODAE_REQUIRE(e->sparse_bits_live, "backward through the sparse code of layer %d without a training forward before it", l - 1);
        {
            ProfScope prof(e, CODAE_K_DROPOUT, s);
            rc = launch_sparse_code_bwd(dact_ptr(e, b, l - 1), e->prec == CODAE_PREC_BF16, e->prec == CODAE_PREC_BF16 ? e->out_ld[l - 1] : e->out[l - 1],
                                        e->res_B, e->out[l - 1], reinterpret_cast<const uint8_t*>(e->tc.sparse.ws), (e->out[l - 1] + 7) / 8,
                                        part_ptr(e, b, l - 1), s);
        }
        if (rc) return rc;
        e->parts_pending[l - 1] = row_sweep_blocks(e->res_B);
    }
    if (!drops_layer(e, l - 1)) return CODAE_OK;
    {
        ProfScope prof(e, CODAE_K_DROPOUT, s);
        rc = launch_dropout_bwd(dact_ptr(e, b, l - 1), e->prec == CODAE_PREC_BF16, e->prec == CODAE_PREC_BF16 ? e->out_ld[l - 1] : e->out[l - 1],
                                e->drop_B, e->out[l - 1], e->drop_rows, l - 1, e->drop_step, step_dev(e, b), e->tc.drop.p[l - 1], e->tc.drop.seed,
                                part_ptr(e, b, l - 1), s);
    }
    if (rc) return rc;
    e->parts_pending[l - 1] = row_sweep_blocks(e->drop_B);
    return CODAE_OK;
}

// Wt_l [in][out] <- W_l [out][in] (bf16) for every layer that has a data gradient (l >= 1)
int refresh_transposed(codae_engine* e, const codae_buffers* b, hipStream_t s, int l_lo = 1, int l_hi = -1) {
    if (e->prec != CODAE_PREC_BF16 || b->shadow_wt == nullptr || e->L < 2) return CODAE_OK;
    if (l_hi < 0) l_hi = e->L;
    for (int base = l_lo; base < l_hi; base += 64) {             // the launch carries at most 64 matrices
        int64_t off[64]; int rows[64], cols[64]; int n = 0;
        for (int l = base; l < l_hi && n < 64; ++l) { off[n] = e->w_off[l]; rows[n] = e->out[l]; cols[n] = e->in[l]; ++n; }
        int rc = launch_transpose_bf16(reinterpret_cast<const bf16_t*>(b->shadow_w), reinterpret_cast<bf16_t*>(b->shadow_wt),
                                       n, off, rows, cols, s);
        if (rc) return rc;
    }
    return CODAE_OK;
}

// rows [B, rows) of a [rows][width] working-precision matrix -> 0 (bf16 mode pads the batch to 64)
int zero_pad_rows(codae_engine* e, void* base, int B, int rows, int width, hipStream_t s) {
    if (rows > B) {
        char* p = reinterpret_cast<char*>(base) + (int64_t)B * width * e->esize();
        CODAE_HIP_CHECK(hipMemsetAsync(p, 0, (int64_t)(rows - B) * width * e->esize(), s));
    }
    return CODAE_OK;
}

int ensure_side_stream(codae_engine* h) {
    if (h->side != nullptr) return CODAE_OK;
    // The side streams must land on a hardware queue of their own: two streams that share one execute serially
    // with ~11 us between dependent kernels (seen with RCCL initialised: every stream of the process on one queue,
    // the whole backward serial).  The runtime keeps a separate queue pool per priority level, so the side streams
    // take the LOWEST priority: never the queue of the caller's normal-priority stream, nor of RCCL's
    // high-priority ones; and the dgrad chain (critical path, caller's stream) is dispatched first.
    int prio_least = 0, prio_greatest = 0;
    CODAE_HIP_CHECK(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
    const int prio = h->cfg.side_priority_set ? h->cfg.side_priority : prio_least;
    CODAE_HIP_CHECK(hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking, prio));
    for (int i = 0; i < CODAE_MAX_DACT; ++i) CODAE_HIP_CHECK(hipEventCreateWithFlags(&h->ev_ready[i], hipEventDisableTiming));
    CODAE_HIP_CHECK(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
    for (int i = 0; i < CODAE_MAX_DACT; ++i) CODAE_HIP_CHECK(hipEventCreateWithFlags(&h->ev_w[i], hipEventDisableTiming));
    return CODAE_OK;
}

// s waits for everything the backward put on the side streams
int join_side(codae_engine* h, hipStream_t s) {
    if (!h->side_dirty || h->side == nullptr) return CODAE_OK;
    CODAE_HIP_CHECK(hipEventRecord(h->ev_join, h->side));
    CODAE_HIP_CHECK(hipStreamWaitEvent(s, h->ev_join, 0));
    for (int i = 0; i < CODAE_MAX_DACT; ++i) h->w_pending[i] = false;
    h->side_dirty = false;
    return CODAE_OK;
}

// Backward over layers hi-1 ... lo.  Step path (dx == nullptr, step_mode): the chain continues
// below `lo` in a later call, so the dgrad of every layer > 0 runs.  Drop-in sub-chain: the dgrad
// of layer `lo` runs only when the caller wants dx, and then lands unmasked in fp32.
//
// Two streams: wgrad_l (+ its slab reduce) goes to the side stream as soon as dA_l exists, the
// dgrad chain stays on `s`; at K = 1536 a third of every GEMM launch is ramp + output drain with
// all CUs in the same phase, and the two kernels fill each other's bubbles.  dA lives in one buffer per
// layer (n_dact = L + 1, up to CODAE_MAX_DACT): nothing is overwritten within a step, so the dgrad chain never
// waits for the side stream; deeper stacks rotate (dgrad_l writes buffer (l-1) % n, which wgrad_{l-1+n} was
// reading, and waits for that wgrad's event).  The last weight gradient (layer 0) runs on `s` itself, beside
// wgrad_1 on the side stream.  With join the call returns with `s` waiting for every side-stream kernel.
// p.norm == NORM_FROM_BACKWARD: every launch that leaves final gradient values behind also adds their sum g^2 to the clip_grad_norm_
// accumulators.  loss: the step's loss finish, left to this call's bias-finish launch (codae_train_step)
int backward_range(codae_handle h, const codae_buffers* b, const StepCall& c, const StepPlan& p, float* dx, hipStream_t s,
                   const LossFinish* loss = nullptr) {
    const int B = c.B, lo = c.layer_lo, hi = c.layer_hi, rows = p.rows;
    const bool step_mode = c.kind != STEP_DROPIN_BACKWARD, join = c.join;
    const bool dual = p.streams == 2, with_norm = p.norm == NORM_FROM_BACKWARD;
    CODAE_REQUIRE(!(step_mode && h->drop_live && h->tc.drop.on) || B == h->drop_B, "backward of %d rows after a dropped forward of %d", B, h->drop_B);
    h->res_B = B;             // (the residual kernels behind the data gradients cover the batch's own rows)
    if (dual) {
        int rc = ensure_side_stream(h);
        if (rc) return rc;
    }
    // (Measured and dropped: the slab reduces on the caller's stream one layer late, or on a third stream - no
    // gain, 1.83 / 1.84 vs 1.82 ms at the time; every GEMM on the caller's stream with only the reduces beside
    // them - 0.27 ms slower: each cross-queue event costs ~10 us.)
    if (p.wgrad != WGRAD_PER_LAYER) {
        // data-gradient chain alone on the chip, then all weight gradients in one launch (see grouped_wgrad_strategy); one stream
        int rc = join_side(h, s);                  // (an earlier bucketed backward may have left work on the side stream)
        if (rc) return rc;
        for (int l = hi - 1; l >= 1; --l) {
            rc = run_dgrad(h, b, l, rows, false, nullptr, s);
            if (rc) return rc;
        }
        return run_grouped_tail(h, b, p, s, loss);
    }
    bool* w_pending = h->w_pending;
    const bool coscheduled = dual;         // the weight gradients run beside the data-gradient chain
    for (int l = hi - 1; l >= lo; --l) {
        int rc;
        if (!dual) {
            rc = run_wgrad(h, b, l, rows, with_norm, s);
        } else if (p.tail_on_caller && l == 0) {
            rc = run_wgrad(h, b, l, rows, with_norm, s, 2);           // (third slab buffer)
        } else {
            hipEvent_t ready = h->ev_ready[h->ready_turn++ % CODAE_MAX_DACT];
            CODAE_HIP_CHECK(hipEventRecord(ready, s));                      // dA_l (and act[l]) are complete on s
            CODAE_HIP_CHECK(hipStreamWaitEvent(h->side, ready, 0));
            rc = run_wgrad(h, b, l, rows, with_norm, h->side, l & 1);                 // two alternating slab buffers
            if (rc == CODAE_OK && h->n_dact <= h->L) {   // (with a buffer per layer nothing is overwritten within a step)
                CODAE_HIP_CHECK(hipEventRecord(h->ev_w[l % h->n_dact], h->side));
                w_pending[l % h->n_dact] = true;
            }
        }
        if (rc) return rc;
        const bool chain = step_mode ? (l > 0) : (l > lo);
        const bool to_dx = !chain && !step_mode && dx != nullptr;
        if (chain || to_dx) {
            // the buffer dgrad_l writes, (l-1) % n, was last read by wgrad_{l-1+n}
            const int wb = (l - 1 + h->n_dact) % h->n_dact;
            if (dual && chain && w_pending[wb]) {
                CODAE_HIP_CHECK(hipStreamWaitEvent(s, h->ev_w[wb], 0));
                w_pending[wb] = false;
            }
            rc = chain ? run_dgrad(h, b, l, rows, coscheduled, nullptr, s) : run_dgrad(h, b, l, B, coscheduled, dx, s);
            if (rc) return rc;
        }
    }
    // bias gradients of every layer whose activation gradient was produced since the last finish (this range's dgrads; the
    // loss, when the range starts at the top): partial rows -> grads' bias block, on the caller's stream.  codae_step_update
    // finishes whatever a caller that stopped short left behind.
    if (p.bias_finish != BIAS_FINISH_NONE) {
        int rc = finish_bias(h, b, s, with_norm, loss);
        if (rc) return rc;
    }
    if (dual) {
        h->side_dirty = true;
        if (join) return join_side(h, s);
    }
    return CODAE_OK;
}

// What the layouts of codae_residual and codae_norm share: the canonical flags of `flags` on this stack (all zero = off), the refusal
// of a layer that cannot take the setting - "a <adjective> layer", which "takes no <noun>" -, and the work space: `lead(on)` bytes
// of the setting's own first, then the 1-bit mask of every flagged layer with a ReLU or a LeakyReLU.
template <class Lead>
int stream_layout(codae_handle h, const char* who, int n, const uint8_t* flags, const char* noun, const char* adjective, bool equal_widths,
                  uint8_t* on, std::vector<int64_t>* bits_off, int64_t* bytes, Lead lead) {
    CODAE_REQUIRE(n == h->L, "%s: %d flags for %d layers", who, n, h->L);
    CODAE_REQUIRE(flags != nullptr, "%s: null on", who);
    bool any = false;
    for (int l = 0; l < h->L; ++l) {
        if (!flags[l]) continue;
        // (codae_create keeps a ReLU layer as relu[l] = 1 with act[l] = NONE: act[l] names the generic activations only, so NONE
        //  below is "no activation or ReLU" and kind 1 never appears)
        char why[96] = "";
        if (l == h->L - 1) snprintf(why, sizeof(why), "the last layer's output is the reconstruction and takes no %s", noun);
        else if (equal_widths && h->in[l] != h->out[l]) snprintf(why, sizeof(why), "an identity skip needs equal widths");
        else if (h->act[l] != CODAE_ACT_NONE && h->act[l] != CODAE_ACT_LEAKY)
            snprintf(why, sizeof(why), "a %s layer's activation must be none, ReLU or LeakyReLU", adjective);
        if (why[0] != 0) {
            set_error("%s: layer %d (%d -> %d, activation kind %d): %s", who, l, h->in[l], h->out[l], h->relu[l] ? CODAE_ACT_RELU : (int)h->act[l], why);
            return CODAE_E_UNSUPPORTED;
        }
        on[l] = 1;
        any = true;
    }
    if (!any) return CODAE_OK;
    int64_t off = lead(on);
    for (int l = 0; l < h->L; ++l) {
        if (!on[l] || !(h->relu[l] || h->act[l] == CODAE_ACT_LEAKY)) continue;
        if (bits_off) (*bits_off)[l] = off;
        off += round_up((int64_t)h->max_batch * ((h->out[l] + 7) / 8), 256);
    }
    *bytes = off;
    return CODAE_OK;
}

// codae_set_residual's and codae_set_norm's refusal of the layer a sparse code is on (codae_set_sparse_code refuses the other order)
int refuse_on_sparse_layer(codae_handle h, const char* who, const uint8_t* on, const char* noun) {
    if (!h->tc.sparse.on || !on[h->tc.sparse.m]) return CODAE_OK;
    const int m = h->tc.sparse.m;
    set_error("%s: layer %d (%d -> %d): a sparse code is on this layer and it takes no %s: name the layers and leave out layer %d", who, m, h->in[m],
              h->out[m], noun, m);
    return CODAE_E_UNSUPPORTED;
}

// the setters' check of the work space the caller brought
int check_stream_ws(const char* who, const void* ws, int64_t ws_bytes, int64_t need) {
    CODAE_REQUIRE(ws != nullptr && (reinterpret_cast<uintptr_t>(ws) & 15) == 0 && ws_bytes >= need,
                  "%s: the work space must be 16-byte aligned and hold %lld bytes (got %lld)", who, (long long)need, (long long)ws_bytes);
    return CODAE_OK;
}

}  // namespace

extern "C" {

const char* codae_last_error(void) { return g_err; }
int codae_abi_version(void) { return CODAE_ABI_VERSION; }

int codae_reload_env(void) {
    env_reload();
    return CODAE_OK;
}

int codae_struct_sizes(int32_t* out, int32_t capacity) {
    CODAE_REQUIRE(out != nullptr && capacity >= CODAE_N_STRUCTS, "codae_struct_sizes: need room for %d entries", CODAE_N_STRUCTS);
    out[0] = (int32_t)sizeof(codae_spec);
    out[1] = (int32_t)sizeof(codae_sizes);
    out[2] = (int32_t)sizeof(codae_buffers);
    out[3] = (int32_t)sizeof(codae_batch);
    out[4] = (int32_t)sizeof(codae_hyper);
    out[5] = CODAE_S_COUNT;
    out[6] = CODAE_K_COUNT;
    return CODAE_OK;
}

int codae_create(const codae_spec* spec, codae_handle* out) {
    CODAE_REQUIRE(spec && out, "codae_create: null argument");
    CODAE_REQUIRE(spec->n_layers > 0 && spec->n_layers <= 64, "codae_create: n_layers %d", spec->n_layers);
    CODAE_REQUIRE(spec->max_batch > 0, "codae_create: max_batch %d", spec->max_batch);
    CODAE_REQUIRE(spec->precision == CODAE_PREC_F32 || spec->precision == CODAE_PREC_BF16, "codae_create: precision");
    for (int l = 0; l < spec->n_layers; ++l) {
        CODAE_REQUIRE(spec->in_features[l] > 0 && spec->out_features[l] > 0, "codae_create: layer %d has an empty side", l);
        CODAE_REQUIRE(l == 0 || spec->in_features[l] == spec->out_features[l - 1],
                      "codae_create: layer %d input %d != previous output %d", l, spec->in_features[l], spec->out_features[l - 1]);
        if (spec->precision == CODAE_PREC_BF16) {
            // 16-byte rows (8 bf16) everywhere: vector loads / stores of the gather, the epilogues and the k-strided staging.  (Round 2
            // needed multiples of 64: every width is also a GEMM k extent; the activation buffers now carry that padding themselves.)
            if (spec->in_features[l] % 8 != 0 || spec->out_features[l] % 8 != 0) {
                set_error("codae_create: bf16 mode needs every layer width to be a multiple of 8 (layer %d is %d -> %d); use CODAE_PREC_F32",
                          l, spec->in_features[l], spec->out_features[l]);
                return CODAE_E_UNSUPPORTED;
            }
        }
    }
    if (spec->act_kind != nullptr) {
        for (int l = 0; l < spec->n_layers; ++l) {
            const int kind = spec->act_kind[l];
            const float* p = spec->act_param ? spec->act_param + 3 * l : nullptr;
            CODAE_REQUIRE(kind >= CODAE_ACT_NONE && kind <= CODAE_ACT_HARDSIGMOID, "codae_create: layer %d: unknown activation kind %d", l, kind);
            CODAE_REQUIRE(l + 1 < spec->n_layers || kind == CODAE_ACT_NONE || kind == CODAE_ACT_RELU,
                          "codae_create: the last layer takes no activation other than ReLU (kind %d)", kind);
            const bool needs_p = kind == CODAE_ACT_LEAKY || kind == CODAE_ACT_ELU || kind == CODAE_ACT_SOFTPLUS;
            CODAE_REQUIRE(!needs_p || p != nullptr, "codae_create: layer %d: activation kind %d needs act_param", l, kind);
            if (kind == CODAE_ACT_LEAKY)
                CODAE_REQUIRE(p[0] >= 0.f && std::isfinite(p[0]), "codae_create: layer %d: LeakyReLU slope %g (need >= 0)", l, p[0]);
            if (kind == CODAE_ACT_ELU)
                CODAE_REQUIRE(p[0] > 0.f && p[1] > 0.f && p[2] > 0.f && std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]),
                              "codae_create: layer %d: ELU parameters scale %g alpha %g 1/beta %g (need all > 0)", l, p[0], p[1], p[2]);
            if (kind == CODAE_ACT_SOFTPLUS)
                CODAE_REQUIRE(p[0] > 0.f && std::isfinite(p[0]) && !std::isnan(p[1]),
                              "codae_create: layer %d: Softplus beta %g threshold %g (need beta > 0)", l, p[0], p[1]);
        }
    }
    env_reload();                 // the one place (besides library load / codae_reload_env) the CODAE_* variables are read
    codae_engine* e = new codae_engine();
    e->cfg = env();
    memset(&e->tc, 0, sizeof(e->tc));       // (padding included: the graph key compares bytes)
    e->L = spec->n_layers;
    e->prec = spec->precision;
    e->max_batch = spec->max_batch;
    e->max_rows = (int)round_up(spec->max_batch, 64);
    int64_t off = 0;
    for (int l = 0; l < e->L; ++l) {
        e->in.push_back(spec->in_features[l]);
        e->out.push_back(spec->out_features[l]);
        const int kind = spec->act_kind ? spec->act_kind[l] : (spec->relu[l] ? CODAE_ACT_RELU : CODAE_ACT_NONE);
        e->relu.push_back(kind == CODAE_ACT_RELU ? 1 : 0);
        e->act.push_back(kind == CODAE_ACT_RELU ? CODAE_ACT_NONE : (uint8_t)kind);
        for (int k = 0; k < 3; ++k) e->act_p.push_back(spec->act_kind && spec->act_param ? spec->act_param[3 * l + k] : 0.f);
        e->in_ld.push_back(e->prec == CODAE_PREC_BF16 ? (int)round_up(e->in[l], 64) : e->in[l]);
        e->out_ld.push_back(e->prec == CODAE_PREC_BF16 ? (int)round_up(e->out[l], 64) : e->out[l]);
        e->w_off.push_back(off);
        off += round_up((int64_t)e->in[l] * e->out[l], 64);
        if (e->in_ld[l] > e->maxw) e->maxw = e->in_ld[l];
        if (e->out_ld[l] > e->maxw) e->maxw = e->out_ld[l];
    }
    e->bias_begin = off;
    for (int l = 0; l < e->L; ++l) {
        e->b_off.push_back(off);
        off += round_up(e->out[l], 64);
    }
    e->n_param = off;
    int64_t a = 0;
    for (int l = 0; l < e->L; ++l) {
        e->act_off.push_back(a);
        a += round_up((int64_t)e->max_rows * e->in_ld[l] * e->esize(), 256);
    }
    e->act_off.push_back(a);  // y, always fp32
    a += round_up((int64_t)e->max_rows * e->out[e->L - 1] * 4, 256);
    // 1 bit per element of every activation that a ReLU produced (the data gradient reads these instead of the activation)
    e->bits_off.assign(e->L, -1);
    if (e->prec == CODAE_PREC_BF16 && !e->cfg.no_relu_bits) {
        for (int l = 1; l < e->L; ++l) {
            if (!e->relu[l - 1]) continue;
            e->bits_off[l] = a;
            a += round_up((int64_t)e->max_rows * (e->in_ld[l] / 8), 256);
        }
    }
    e->act_bytes = a;
    e->dact_one = round_up((int64_t)e->max_rows * e->maxw * e->esize(), 256);
    // one activation-gradient buffer per layer when the stack is shallow enough (no write-after-read waits between the
    // two backward streams, whose barrier packets cost ~11 us each); deeper stacks rotate through CODAE_MAX_DACT
    e->n_dact = e->L + 1 <= CODAE_MAX_DACT ? e->L + 1 : CODAE_MAX_DACT;
    if (e->n_dact < 3) e->n_dact = 3;
    if (e->prec == CODAE_PREC_BF16 && e->n_dact <= e->L) {
        // rotating buffers are shared by layers of different widths: one layer's zero pad columns would be another's data
        for (int l = 0; l < e->L; ++l)
            if (e->in[l] % 64 != 0 || e->out[l] % 64 != 0) {
                set_error("codae_create: bf16 stacks deeper than %d layers need widths that are multiples of 64 (layer %d is %d -> %d)",
                          CODAE_MAX_DACT - 1, l, e->in[l], e->out[l]);
                delete e;
                return CODAE_E_UNSUPPORTED;
            }
    }
    bool generic_act = false;
    for (int l = 0; l < e->L; ++l) generic_act = generic_act || e->act[l] != CODAE_ACT_NONE;
    // the persistent chain knows ReLU only: a stack with another activation runs the per-layer launches
    e->chain_ok = e->prec == CODAE_PREC_BF16 && !e->cfg.no_chain && !generic_act && e->L + 1 <= CODAE_MAX_DACT &&
                  chain_supported(e->L, e->in.data(), e->out.data()) && e->in[0] == e->out[e->L - 1];
    // partial column-sum rows per layer: a producer writes at most one row per 64 batch rows (exact-fp32 GEMM, dense
    // colsum), the stand-alone loss kernel of the last layer one per 32, the persistent chain one per 16
    e->parts_pending.assign(e->L, 0);
    e->res_bits_off.assign(e->L, -1);
    e->norm_r_off.assign(e->L, -1);
    e->norm_bits_off.assign(e->L, -1);
    e->part_floats = 0;
    const int chain_rows = e->max_rows < CHAIN_MAX_ROWS ? e->max_rows : CHAIN_MAX_ROWS;
    for (int l = 0; l < e->L; ++l) {
        e->part_off.push_back(e->part_floats);
        int64_t rows_cap = (l == e->L - 1) ? (e->max_rows + 31) / 32 : (e->max_rows + 63) / 64;
        if (e->chain_ok && chain_rows / 16 > rows_cap) rows_cap = chain_rows / 16;
        e->part_floats += round_up(rows_cap * (int64_t)e->out[l], 64);
    }
    {   // + the loss kernels' per-workgroup metric sums: [workgroups][2] doubles ([..][3] from the emphasised loss kernel)
        const int io = e->out[e->L - 1];
        const int by_rows = (e->max_rows + 31) / 32;                                             // stand-alone loss kernel
        const int by_tiles = tile_count(e->max_rows, io, TILE_64x64);                          // fused into the last GEMM (smallest tile)
        e->loss_part_cap = by_rows > by_tiles ? by_rows : by_tiles;
        if (e->chain_ok && chain_rows / 16 > e->loss_part_cap) e->loss_part_cap = chain_rows / 16;
        e->loss_part_off = e->part_floats;
        e->part_floats += round_up((int64_t)e->loss_part_cap * 6, 64);
    }
    e->slab_bytes = 0;
    for (int l = 0; l < e->L; ++l) {
        int s = 1;
        if (e->prec == CODAE_PREC_BF16) s = choose_split_k(e->out[l], e->in[l], e->max_rows);
        else s = choose_split_k_f32(e->out[l], e->in[l], e->max_rows);
        e->split_k.push_back(s);
        if (s > 1) {
            const int64_t bytes = (int64_t)s * e->in[l] * e->out[l] * 4;
            if (bytes > e->slab_bytes) e->slab_bytes = bytes;
        }
    }
    if (e->prec == CODAE_PREC_F32 && e->max_rows <= 512) {
        // room for the split-K slabs of a small batch's forward / data-gradient launches (gemm_f32_small)
        const int64_t bytes = (int64_t)16 * e->max_rows * e->maxw * 4;
        if (bytes > e->slab_bytes) e->slab_bytes = bytes;
    }
    *out = e;
    return CODAE_OK;
}

static void profile_release(codae_handle h) {
    for (hipEvent_t ev : h->prof_start) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : h->prof_stop) (void)hipEventDestroy(ev);
    h->prof_start.clear(); h->prof_stop.clear(); h->prof_kind.clear(); h->prof_count.clear(); h->prof_group = false;
    h->prof_on = false; h->prof_n = 0;
}

int codae_destroy(codae_handle h) {
    if (h) profile_release(h);
    if (h && h->graph_exec) { (void)hipGraphExecDestroy(h->graph_exec); h->graph_exec = nullptr; }
    if (h && h->side) {
        (void)hipStreamSynchronize(h->side);
        for (int i = 0; i < CODAE_MAX_DACT; ++i) if (h->ev_ready[i]) (void)hipEventDestroy(h->ev_ready[i]);
        (void)hipEventDestroy(h->ev_join);
        for (int i = 0; i < CODAE_MAX_DACT; ++i) (void)hipEventDestroy(h->ev_w[i]);
        (void)hipStreamDestroy(h->side);
    }
    if (h && h->dp) (void)codae_dp_destroy(h);
    delete h;
    return CODAE_OK;
}

int codae_profile_begin(codae_handle h, uint32_t class_mask, int32_t max_records) {
    CODAE_REQUIRE(h && max_records > 0 && max_records <= (1 << 20), "codae_profile_begin: bad arguments");
    profile_release(h);
    h->prof_start.resize(max_records); h->prof_stop.resize(max_records); h->prof_kind.assign(max_records, -1); h->prof_count.assign(max_records, 1);
    for (int i = 0; i < max_records; ++i) {
        CODAE_HIP_CHECK(hipEventCreate(&h->prof_start[i]));
        CODAE_HIP_CHECK(hipEventCreate(&h->prof_stop[i]));
    }
    h->prof_mask = class_mask; h->prof_n = 0; h->prof_on = true; h->prof_step = 0;
    return CODAE_OK;
}

int codae_profile_stride(codae_handle h, int32_t every_n_steps) {
    CODAE_REQUIRE(h && every_n_steps >= 1, "codae_profile_stride: bad arguments");
    h->prof_every = every_n_steps;
    return CODAE_OK;
}

int codae_profile_end(codae_handle h, int32_t* kinds, float* ms, int32_t capacity, int32_t* n_out) {
    CODAE_REQUIRE(h && kinds && ms && n_out, "codae_profile_end: null argument");
    h->prof_on = false;
    int n = 0;
    for (int i = 0; i < h->prof_n && n < capacity; ++i) {
        if (h->prof_count[i] < 0) { kinds[n] = h->prof_kind[i]; ms[n] = 0.f; ++n; continue; }      // (prof_rides_along)
        CODAE_HIP_CHECK(hipEventSynchronize(h->prof_stop[i]));
        float t = 0.f;
        CODAE_HIP_CHECK(hipEventElapsedTime(&t, h->prof_start[i], h->prof_stop[i]));
        const int c = h->prof_count[i];
        // a group record is reported as `c` launches of elapsed / c each
        for (int k = 0; k < c && n < capacity; ++k) { kinds[n] = h->prof_kind[i]; ms[n] = t / (float)c; ++n; }
    }
    *n_out = n;
    profile_release(h);
    return CODAE_OK;
}

int codae_get_sizes(codae_handle h, codae_sizes* out) {
    CODAE_REQUIRE(h && out, "codae_get_sizes: null argument");
    out->n_param = h->n_param;
    // (+ 64 rows of slack behind the last matrix: a GEMM whose k extent is a padded width reads the weight operand up to 63
    //  elements / rows past a row's / the matrix's end - multiplied by the zero pad columns of the activations, see in_ld)
    out->n_weight = h->prec == CODAE_PREC_BF16 ? h->n_param + (int64_t)64 * h->maxw : 0;
    out->act_bytes = h->act_bytes;
    out->dact_bytes = h->n_dact * h->dact_one;
    out->slab_bytes = 3 * h->slab_bytes;   // side stream: two alternating slab buffers; caller's stream (tail wgrad): the third
    out->bias_part_bytes = h->part_floats * 4;
    out->n_scalars = CODAE_S_COUNT;
    return CODAE_OK;
}

int codae_param_offsets(codae_handle h, int32_t layer, int64_t* w_off, int64_t* b_off, int64_t* shadow_off) {
    CODAE_REQUIRE(h && layer >= 0 && layer < h->L, "codae_param_offsets: layer %d", layer);
    if (w_off) *w_off = h->w_off[layer];
    if (b_off) *b_off = h->b_off[layer];
    if (shadow_off) *shadow_off = h->w_off[layer];
    return CODAE_OK;
}

int codae_sync_shadows(codae_handle h, const codae_buffers* b, void* stream) {
    CODAE_REQUIRE(h && b && b->params, "codae_sync_shadows: null argument");
    if (h->tc.tied && !h->tie_pairs.empty()) {
        // the encoder is the truth: the decoder's fp32 image first, the cast and the transposes below then see a tied vector
        int rc = launch_tie_mirror(b->params, nullptr, nullptr, h->tie_pairs.data(), (int)h->tie_pairs.size(), (hipStream_t)stream);
        if (rc) return rc;
    }
    if (h->prec != CODAE_PREC_BF16) return CODAE_OK;
    CODAE_REQUIRE(b->shadow_w, "codae_sync_shadows: shadow_w missing");
    int rc = launch_cast_bf16(b->params, reinterpret_cast<bf16_t*>(b->shadow_w), h->n_param, (hipStream_t)stream);
    if (rc) return rc;
    return refresh_transposed(h, b, (hipStream_t)stream);
}

int codae_forward(codae_handle h, const codae_buffers* b, const float* x, float* y, int32_t B, int32_t layer_lo,
                  int32_t layer_hi, int32_t save_for_backward, void* stream) {
    int rc = check_common(h, b, B);
    if (rc) return rc;
    CODAE_REQUIRE(x && y, "codae_forward: null x or y");
    CODAE_REQUIRE(layer_lo >= 0 && layer_lo < layer_hi && layer_hi <= h->L, "codae_forward: layer range [%d, %d)", layer_lo, layer_hi);
    (void)save_for_backward;  // activations always live in the workspace; a later forward overwrites them
    if (!(layer_lo == 0 && layer_hi == h->L)) {
        char what[96];
        snprintf(what, sizeof(what), "a forward over the layer range [%d, %d) of %d layers is not supported", layer_lo, layer_hi, h->L);
        rc = refuse_skips_or_norm(h, "codae_forward", what);
        if (rc) return rc;
    }
    forward_leaves(h, nullptr, nullptr);      // (a drop-in forward never drops, nor writes the skips' and the norm's masks)
    hipStream_t s = (hipStream_t)stream;
    const int rows = h->rows_for(B);
    // ingest x into act[layer_lo] in working precision (no gather, no mask)
    codae_batch in{};
    in.data = x; in.B = B; in.io = h->in[layer_lo];
    rc = launch_gather_noise(&in, nullptr, 0, nullptr, act_ptr(h, b, layer_lo), h->prec == CODAE_PREC_BF16, s, h->in_ld[layer_lo]);
    if (rc) return rc;
    rc = zero_pad_rows(h, act_ptr(h, b, layer_lo), B, rows, h->in_ld[layer_lo], s);
    if (rc) return rc;
    for (int l = layer_lo; l < layer_hi; ++l) {
        // (the chain's result goes straight to the caller's fp32 tensor, B rows only)
        rc = run_forward_layer(h, b, l, l == layer_hi - 1 ? y : nullptr, B, rows, false, s);
        if (rc) return rc;
    }
    return CODAE_OK;
}

int codae_backward(codae_handle h, const codae_buffers* b, const float* dy, float* dx, int32_t B, int32_t layer_lo,
                   int32_t layer_hi, void* stream) {
    int rc = check_common(h, b, B);
    if (rc) return rc;
    CODAE_REQUIRE(dy && b->grads && b->dacts, "codae_backward: null dy / grads / dacts");
    CODAE_REQUIRE(layer_lo >= 0 && layer_lo < layer_hi && layer_hi <= h->L, "codae_backward: layer range [%d, %d)", layer_lo, layer_hi);
    // (the drop-in forward writes no masks; its sub-chains cut the sum G across the cut, and a sub-chain's forward does not normalise)
    rc = refuse_skips_or_norm(h, "codae_backward", "the drop-in backward is not supported (use the step entry points)");
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int rows = h->rows_for(B);
    const int top = layer_hi - 1;
    CODAE_REQUIRE(b->bias_parts, "codae_backward: bias_parts missing");
    // dA_top = dy in working precision; db_top = column sums of dy (per 64-row block here, added up after the chain)
    codae_batch in{};
    in.data = dy; in.B = B; in.io = h->out[top];
    rc = launch_gather_noise(&in, nullptr, 0, nullptr, dact_ptr(h, b, top), h->prec == CODAE_PREC_BF16, s, h->out_ld[top]);
    if (rc) return rc;
    rc = zero_pad_rows(h, dact_ptr(h, b, top), B, rows, h->out_ld[top], s);
    if (rc) return rc;
    rc = launch_colsum_parts_f32(dy, B, h->out[top], part_ptr(h, b, top), s);
    if (rc) return rc;
    h->parts_pending[top] = (B + 63) / 64;
    const StepCall call{STEP_DROPIN_BACKWARD, B, layer_lo, layer_hi, true, dx != nullptr, false, false};
    return backward_range(h, b, call, step_plan(h, b, call), dx, s);
}

// What assumes equal-width slots (E = io / S) is refused while the mixed-variable criterion is on, naming the option
static int refuse_with_variable_loss(codae_handle h, const char* option) {
    if (!h->variable_on()) return CODAE_OK;
    set_error("%s is not supported with the mixed-variable criterion (codae_set_variable_loss): it assumes equal-width slots", option);
    return CODAE_E_UNSUPPORTED;
}

// The slot contrast behind the criterion's kernel and its finish (a no-op while it is off): prepare this step's candidates, add the
// term's gradient to the dY the criterion left - its partial column-sum rows replace the criterion kernel's -, then add the term
// to CODAE_S_LAST_LOSS.  The per-block sums reuse the criterion's rows, which its finish has read by then (same stream).
static int run_slot_contrast(codae_handle h, const codae_buffers* b, const codae_hyper* hyper, LossLaunch ll, hipStream_t s) {
    if (!h->contrast_on()) return CODAE_OK;
    const int B = ll.batch->B;
    const int blocks = slot_contrast_blocks(B);
    CODAE_REQUIRE(blocks <= h->loss_part_cap && blocks <= (h->max_rows + 31) / 32,
                  "slot contrast: %d row blocks exceed the partial-sum rows (%d)", blocks, h->loss_part_cap);
    const double rows = hyper->loss_scale_rows > 0.f ? (double)hyper->loss_scale_rows : (double)B;
    const double scale = (double)h->tc.contrast.weight / (rows * (double)h->tc.contrast.n_slots);
    ll.emph = h->tc.emph_on ? &h->tc.emph : nullptr;
    ll.scale = (float)scale;
    int rc;
    {
        ProfScope prof(h, CODAE_K_LOSS, s);
        rc = launch_slot_contrast_prepare(ll.batch->data, ll.batch->io, &h->tc.contrast, ll.step, ll.step_dev, ll.dy_bf16, s, ll.present, ll.n_slots);
    }
    if (rc) return rc;
    {
        ProfScope prof(h, CODAE_K_LOSS, s);
        rc = launch_slot_contrast(ll, &h->tc.contrast, s);
    }
    if (rc) return rc;
    h->parts_pending[h->L - 1] = blocks;
    return launch_slot_contrast_finish(b->scalars, scale, ll.parts, blocks, s);
}

// The training step's stand-alone loss behind the last forward GEMM: dY, the last bias gradient's partial rows and the per-block
// sums from y, the finish that goes with the kernel, then the slot contrast.  A criterion other than the MSE first (with or without
// emphasis: its kernels form the weight themselves), then the emphasised MSE (a presence table without emphasis: the same kernel
// with unit weights), then the plain MSE.
static int run_standalone_loss(codae_handle h, const codae_buffers* b, const codae_batch* batch, const codae_hyper* hyper, const float* y,
                               hipStream_t s) {
    const int L = h->L, blocks = mse_loss_colsum_rows(batch->B);
    const double inv_n = loss_inv_n(hyper, batch);
    codae_emphasis unit{};
    unit.alpha = 1.f; unit.beta = 1.f;
    LossLaunch ll{batch, &h->tc.noise, hyper->step, step_dev(h, b), h->tc.emph_on ? &h->tc.emph : nullptr, h->tc.pres.table, h->tc.pres.n_slots,
                  y, dact_ptr(h, b, L - 1), h->prec == CODAE_PREC_BF16, h->out_ld[L - 1], (float)inv_n, part_ptr(h, b, L - 1), loss_parts_ptr(h, b),
                  &h->tc.swap};
    const bool weighted = h->recon_on() || h->tc.emph_on || ll.present != nullptr;      // (the kernels that leave three sums per block)
    int rc;
    if (h->variable_on()) {
        // the mixed-variable criterion: per-block sums, the finish that forms every variable's coefficient, then dY (its setter
        // refuses emphasis, another criterion, the slot contrast and a presence table: nothing else rides on this step's loss)
        const codae_engine::VarCfg& vc = h->tc.var;
        CODAE_REQUIRE(vc.ws_bytes >= variable_loss_ws_bytes(vc.n_var, batch->B), "variable loss: the work space does not hold %d rows", batch->B);
        {
            ProfScope prof(h, CODAE_K_LOSS, s);
            rc = launch_variable_partials(ll, vc.ws, vc.n_var, s);
        }
        if (rc) return rc;
        {
            ProfScope prof(h, CODAE_K_LOSS, s);
            rc = launch_variable_finish(ll, vc.ws, vc.n_var, b->scalars, s);
        }
        if (rc) return rc;
        h->norm_scalars_zero = true;
        {
            ProfScope prof(h, CODAE_K_LOSS, s);
            rc = launch_variable_grad(ll, vc.ws, vc.n_var, s);
        }
        if (rc) return rc;
        h->parts_pending[L - 1] = blocks;
        return CODAE_OK;
    }
    {
        ProfScope prof(h, CODAE_K_LOSS, s);
        if (h->recon_on()) {
            rc = launch_recon_loss(ll, &h->tc.recon, s);
        } else if (weighted) {
            if (!h->tc.emph_on) ll.emph = &unit;
            rc = launch_emph_loss(ll, s);
        } else {
            rc = launch_mse_loss(ll, 1, s);
        }
    }
    if (rc) return rc;
    h->parts_pending[L - 1] = blocks;
    h->norm_scalars_zero = true;
    rc = weighted ? launch_finish_emph_loss(b->scalars, inv_n, s, ll.parts, blocks) : finish_loss(h, b, batch, blocks, s);
    return rc ? rc : run_slot_contrast(h, b, hyper, ll, s);
}

// The gather of a bf16 step reads the registered bf16 image instead of the fp32 rows: only for the very dataset the image
// was registered with, only where the image kernel's 16-byte accesses are legal, and only when no arithmetic is done on the values -
// no noise (noise_kind: the kind this call applies), or swap noise, whose swapped slot is a bf16 row of another row; everything
// else runs what it always ran.
static bool gathers_from_image(codae_handle h, const codae_batch* batch, const void* out, int noise_kind) {
    const codae_engine::ImageCfg& im = h->tc.img;
    if (noise_kind != CODAE_NOISE_NONE && noise_kind != CODAE_NOISE_SWAP) return false;
    return h->prec == CODAE_PREC_BF16 && !h->cfg.no_dataset_image && im.image != nullptr && batch->data == im.data && batch->io == im.io &&
           gather_image_takes(batch, im.image, out, h->in_ld[0]);
}

// plan.loss_finish == LOSS_FINISH_CARRIED (codae_train_step): the fused loss's finish is not launched: *fold describes it for the
// bias-finish launch that ends the backward, and the gather's first block clears the norm accumulators instead.
// fold->scalars stays null when this call finished the loss itself.
static int forward_loss_impl(codae_handle h, const codae_buffers* b, const codae_batch* batch, const codae_hyper* hyper,
                             float* out_y, void* stream, const StepPlan& plan, LossFinish* fold) {
    int rc = check_common(h, b, batch->B);
    if (rc) return rc;
    CODAE_REQUIRE(batch->io == h->in[0] && batch->io == h->out[h->L - 1], "batch.io %d does not match the model (%d -> %d)",
                  batch->io, h->in[0], h->out[h->L - 1]);
    CODAE_REQUIRE(b->grads && b->dacts && b->scalars, "codae_step_forward_loss: grads / dacts / scalars missing");
    CODAE_REQUIRE(b->bias_parts, "codae_step_forward_loss: bias_parts missing");
    if (h->prof_on) ++h->prof_step;
    hipStream_t s = (hipStream_t)stream;
    const int B = batch->B, L = h->L;
    const int rows = plan.rows;
    const bool bf = h->prec == CODAE_PREC_BF16;
    forward_leaves(h, batch, hyper);
    const uint8_t* const pres = h->tc.pres.table;
    const int pres_slots = h->tc.pres.n_slots;
    const bool fuse_loss = plan.loss == LOSS_FUSED, fold_finish = plan.loss_finish == LOSS_FINISH_CARRIED;
    {
        ProfScope prof(h, CODAE_K_GATHER, s);
        double* zero_norm = fold_finish ? b->scalars : nullptr;
        const bool noised = hyper != nullptr && h->tc.noise.kind != CODAE_NOISE_NONE;      // training input only; the loss below reads the clean row
        const codae_noise* noise = noised ? &h->tc.noise : nullptr;
        const int32_t nstep = noised ? hyper->step : 0;
        if (gathers_from_image(h, batch, act_ptr(h, b, 0), noised ? h->tc.noise.kind : CODAE_NOISE_NONE))
            rc = launch_gather_image(batch, reinterpret_cast<const bf16_t*>(h->tc.img.image), reinterpret_cast<bf16_t*>(act_ptr(h, b, 0)), s,
                                     h->in_ld[0], zero_norm, pres, pres_slots, noise, nstep, step_dev(h, b), &h->tc.swap);
        else
            rc = launch_gather_noise(batch, noise, nstep, step_dev(h, b), act_ptr(h, b, 0), bf, s, h->in_ld[0], nullptr, zero_norm, pres,
                                     pres_slots, &h->tc.swap);
    }
    if (rc) return rc;
    rc = zero_pad_rows(h, act_ptr(h, b, 0), B, rows, h->in_ld[0], s);
    if (rc) return rc;
    float* y = out_y ? out_y : reinterpret_cast<float*>(act_ptr(h, b, L));
    GroupScope fwd_group(h, CODAE_K_GEMM_FWD, s);       // the plain forward launches of this step, back to back
    if (h->drop_live || h->tc.res.any || h->tc.norm.any || h->tc.sparse.on) fwd_group.close();   // (streaming kernels sit between them: every launch gets its own event pair)
    for (int l = 0; l < L; ++l) {
        const bool last = (l == L - 1);
        if (last && fuse_loss) {
            fwd_group.close();
            GemmBf16 g = layer_fwd_bf16(h, b, l, act_ptr(h, b, l), dact_ptr(h, b, l), h->out_ld[l], false, rows);
            g.colsum_part = part_ptr(h, b, l);
            g.loss.enabled = 1; g.loss.data = batch->data; g.loss.row_idx = batch->row_idx; g.loss.mask_id = batch->mask_id;
            g.loss.mask_to_use = batch->mask_to_use; g.loss.nb_run = batch->nb_run; g.loss.run = batch->run;
            g.loss.table = batch->mask_table; g.loss.io = batch->io; g.loss.B = B; g.loss.inv_n = (float)loss_inv_n(hyper, batch);
            g.loss.parts = loss_parts_ptr(h, b);
            if (b->shadow_wt != nullptr && l >= 1 && !h->cfg.no_wt && !h->cfg.no_prefetch) {     // the first data gradient's operand
                g.prefetch = reinterpret_cast<const bf16_t*>(b->shadow_wt) + h->w_off[l];
                g.prefetch_bytes = (int64_t)h->in[l] * h->out[l] * 2;
            }
            const int n_loss_parts = gemm_bf16_loss_parts(g);
            CODAE_REQUIRE(n_loss_parts <= h->loss_part_cap, "fused loss: %d workgroups exceed the partial-sum rows (%d)", n_loss_parts, h->loss_part_cap);
            {
                ProfScope prof(h, CODAE_K_LOSS, s);     // last layer + loss in one launch: its own class, not a plain forward GEMM
                rc = gemm_bf16(g, s);
            }
            if (rc) return rc;
            h->parts_pending[l] = gemm_bf16_colsum_rows(g);
            h->norm_scalars_zero = true;        // (by finish_loss below, or already by the gather's first block)
            if (fold_finish) {
                fold->scalars = b->scalars; fold->inv_n = 1.0 / ((double)B * batch->io);
                fold->parts = loss_parts_ptr(h, b); fold->n_parts = n_loss_parts;
                return CODAE_OK;
            }
            return finish_loss(h, b, batch, n_loss_parts, s);
        }
        rc = run_forward_layer(h, b, l, last ? y : nullptr, B, rows, hyper != nullptr, s, &fwd_group);
        if (rc) return rc;
    }
    fwd_group.close();
    if (hyper != nullptr) {
        rc = zero_pad_rows(h, dact_ptr(h, b, L - 1), B, rows, h->out_ld[L - 1], s);
        if (rc) return rc;
        return run_standalone_loss(h, b, batch, hyper, y, s);
    }
    // evaluation: the sums alone
    const LossLaunch sums{batch, nullptr, 0, nullptr, nullptr, pres, pres_slots, y, nullptr, 0, 0, 0.f, nullptr, loss_parts_ptr(h, b)};
    rc = launch_mse_loss(sums, 0, s);
    if (rc) return rc;
    return finish_loss(h, b, batch, mse_loss_colsum_rows(B), s);
}

int codae_step_forward_loss(codae_handle h, const codae_buffers* b, const codae_batch* batch, const codae_hyper* hyper,
                            float* out_y, void* stream) {
    CODAE_REQUIRE(batch != nullptr, "codae_step_forward_loss: null batch");
    CODAE_REQUIRE(h != nullptr && b != nullptr, "null handle or buffers");
    const StepCall call{hyper != nullptr ? STEP_FORWARD_LOSS : STEP_EVAL, batch->B, 0, h->L, true, false, out_y != nullptr, false};
    return forward_loss_impl(h, b, batch, hyper, out_y, stream, step_plan(h, b, call), nullptr);
}

int codae_set_input_noise(codae_handle h, const codae_noise* noise) {
    CODAE_REQUIRE(h != nullptr, "codae_set_input_noise: null handle");
    int rc = check_noise(noise);
    if (rc) return rc;
    if (noise != nullptr && noise->kind == CODAE_NOISE_SWAP) {
        rc = refuse_with_variable_loss(h, "swap noise");
        if (rc) return rc;
        rc = check_swap(&h->tc.swap, h->in[0], h->tc.pres.table, h->tc.pres.n_slots, "codae_set_input_noise");
        if (rc) return rc;
    }
    codae_noise n{};                     // (built field by field: the graph key compares bytes, padding included)
    if (noise != nullptr && noise->kind != CODAE_NOISE_NONE) {
        n.kind = noise->kind; n.p0 = noise->p0; n.seed = noise->seed;
        if (noise->kind == CODAE_NOISE_SALT_PEPPER) { n.p1 = noise->p1; n.p2 = noise->p2; }
    }
    h->tc.noise = n;
    return CODAE_OK;
}

int codae_set_swap_pool(codae_handle h, const int32_t* pool, int32_t n_pool, int32_t n_slots) {
    CODAE_REQUIRE(h != nullptr, "codae_set_swap_pool: null handle");
    codae_swap sw{};                     // (built field by field: the graph key compares bytes)
    if (pool == nullptr && n_pool == 0 && n_slots == 0) {
        CODAE_REQUIRE(h->tc.noise.kind != CODAE_NOISE_SWAP, "codae_set_swap_pool: swap noise is on: switch it off before clearing its slots");
    } else {
        sw.pool = pool; sw.n_pool = n_pool; sw.n_slots = n_slots;
        const int rc = check_swap(&sw, h->in[0], h->tc.pres.table, h->tc.pres.n_slots, "codae_set_swap_pool");
        if (rc) return rc;
    }
    h->tc.swap = sw;
    return CODAE_OK;
}

int codae_set_loss_emphasis(codae_handle h, const codae_emphasis* emphasis) {
    CODAE_REQUIRE(h != nullptr, "codae_set_loss_emphasis: null handle");
    int rc = check_emphasis(emphasis);
    if (rc) return rc;
    codae_emphasis e{};                  // (built field by field: the graph key compares bytes, padding included)
    const bool on = emphasis != nullptr && !(emphasis->alpha == 1.f && emphasis->beta == 1.f && emphasis->col_weight == nullptr);
    if (on) {
        rc = refuse_with_variable_loss(h, "loss emphasis");
        if (rc) return rc;
    }
    if (on) { e.alpha = emphasis->alpha; e.beta = emphasis->beta; e.col_weight = emphasis->col_weight; }
    h->tc.emph = e;
    h->tc.emph_on = on;
    return CODAE_OK;
}

int codae_set_recon_loss(codae_handle h, const codae_recon_loss* loss) {
    CODAE_REQUIRE(h != nullptr, "codae_set_recon_loss: null handle");
    int rc = check_recon_loss(loss, h->out[h->L - 1]);
    if (rc) return rc;
    CODAE_REQUIRE(loss == nullptr || loss->kind != CODAE_LOSS_SLOT_COSINE || h->tc.pres.table == nullptr || loss->n_slots == h->tc.pres.n_slots,
                  "codae_set_recon_loss: slot_cosine n_slots %d differs from the presence table's %d", loss->n_slots, h->tc.pres.n_slots);
    codae_recon_loss r{};                // (built field by field: the graph key compares bytes)
    const bool on = loss != nullptr && loss->kind != CODAE_LOSS_MSE;
    if (on) {
        rc = refuse_with_variable_loss(h, "a reconstruction loss (codae_set_recon_loss)");
        if (rc) return rc;
        r.kind = loss->kind;
        if (loss->kind == CODAE_LOSS_SMOOTH_L1 || loss->kind == CODAE_LOSS_HUBER) r.param = loss->param;
        if (loss->kind == CODAE_LOSS_SLOT_COSINE) { r.mse_weight = loss->mse_weight; r.n_slots = loss->n_slots; }
    }
    h->tc.recon = r;
    return CODAE_OK;
}

int codae_set_variable_loss(codae_handle h, const codae_variable_loss* loss) {
    CODAE_REQUIRE(h != nullptr, "codae_set_variable_loss: null handle");
    codae_engine::VarCfg v{};            // (built field by field: the graph key compares bytes)
    if (loss != nullptr) {
        int rc = check_variable_loss(loss, h->out[h->L - 1], h->max_batch);
        if (rc) return rc;
        const char* clash = h->tc.emph_on ? "loss emphasis" : h->recon_on() ? "a reconstruction loss (codae_set_recon_loss)" :
                            h->contrast_on() ? "slot contrast" : h->tc.pres.table != nullptr ? "a slot-presence table" :
                            h->tc.noise.kind == CODAE_NOISE_SWAP ? "swap noise" : nullptr;
        if (clash != nullptr) {
            set_error("%s is not supported with the mixed-variable criterion (codae_set_variable_loss): it assumes equal-width slots", clash);
            return CODAE_E_UNSUPPORTED;
        }
        if (h->dp != nullptr) {
            set_error("data parallel is not supported with the mixed-variable criterion: a global-batch RMSE is not a sum over shards");
            return CODAE_E_UNSUPPORTED;
        }
        rc = variable_loss_upload(loss);
        if (rc) return rc;
        v.ws = loss->ws; v.ws_bytes = loss->ws_bytes; v.n_var = loss->n_var; v.on = 1;
    }
    h->tc.var = v;
    return CODAE_OK;
}

int codae_set_slot_contrast(codae_handle h, const codae_slot_contrast* contrast) {
    CODAE_REQUIRE(h != nullptr, "codae_set_slot_contrast: null handle");
    int rc = check_slot_contrast(contrast, h->out[h->L - 1], h->prec == CODAE_PREC_BF16);
    if (rc) return rc;
    CODAE_REQUIRE(contrast == nullptr || contrast->weight == 0.f || h->tc.pres.table == nullptr ||
                      (contrast->n_slots == h->tc.pres.n_slots && (int64_t)contrast->n_rows <= h->tc.pres.n_rows),
                  "codae_set_slot_contrast: n_slots %d / n_rows %d do not fit the presence table (%d slots, %lld rows)", contrast->n_slots,
                  contrast->n_rows, h->tc.pres.n_slots, (long long)h->tc.pres.n_rows);
    codae_slot_contrast c{};             // (built field by field: the graph key compares bytes)
    const bool on = contrast != nullptr && contrast->weight != 0.f;
    if (on) {
        rc = refuse_with_variable_loss(h, "slot contrast");
        if (rc) return rc;
        rc = slot_contrast_warm();
        if (rc) return rc;
        c.n_slots = contrast->n_slots; c.n_neg = contrast->n_neg; c.tau = contrast->tau; c.weight = contrast->weight;
        c.seed = contrast->seed; c.n_rows = contrast->n_rows; c.n_pool = contrast->pool ? contrast->n_pool : 0;
        c.ws_bytes = contrast->ws_bytes; c.pool = contrast->pool; c.item_id = contrast->item_id; c.ws = contrast->ws;
    }
    h->tc.contrast = c;
    return CODAE_OK;
}

int codae_set_slot_presence(codae_handle h, const uint8_t* present, int64_t n_rows, int32_t n_slots) {
    CODAE_REQUIRE(h != nullptr, "codae_set_slot_presence: null handle");
    codae_engine::PresCfg p{};           // (built field by field: the graph key compares bytes, padding included)
    if (present != nullptr) {
        int rc = refuse_with_variable_loss(h, "a slot-presence table");
        if (rc) return rc;
        rc = check_presence(present, n_slots, h->out[h->L - 1], "codae_set_slot_presence");
        if (rc) return rc;
        CODAE_REQUIRE(n_rows >= 1, "codae_set_slot_presence: n_rows %lld must be >= 1", (long long)n_rows);
        CODAE_REQUIRE(!(h->recon_on() && h->tc.recon.kind == CODAE_LOSS_SLOT_COSINE) || h->tc.recon.n_slots == n_slots,
                      "codae_set_slot_presence: n_slots %d differs from slot_cosine's %d", n_slots, h->tc.recon.n_slots);
        CODAE_REQUIRE(!h->contrast_on() || (h->tc.contrast.n_slots == n_slots && (int64_t)h->tc.contrast.n_rows <= n_rows),
                      "codae_set_slot_presence: %d slots / %lld rows do not fit the slot contrast (%d slots, %d rows)", n_slots,
                      (long long)n_rows, h->tc.contrast.n_slots, h->tc.contrast.n_rows);
        CODAE_REQUIRE(h->tc.swap.n_slots == 0 || h->tc.swap.n_slots == n_slots, "codae_set_slot_presence: n_slots %d differs from the swap noise's %d",
                      n_slots, h->tc.swap.n_slots);
        p.table = present; p.n_rows = n_rows; p.n_slots = n_slots;
    }
    h->tc.pres = p;
    return CODAE_OK;
}

int codae_set_dataset_image(codae_handle h, const float* data, const void* image_bf16, int64_t n_rows, int32_t io) {
    CODAE_REQUIRE(h != nullptr, "codae_set_dataset_image: null handle");
    codae_engine::ImageCfg im{};         // (built field by field: the graph key compares bytes, padding included)
    if (image_bf16 != nullptr) {
        CODAE_REQUIRE(data != nullptr, "codae_set_dataset_image: an image without the dataset it was cast from");
        CODAE_REQUIRE(n_rows >= 1, "codae_set_dataset_image: n_rows %lld must be >= 1", (long long)n_rows);
        CODAE_REQUIRE(io == h->in[0], "codae_set_dataset_image: io %d does not match the model (%d)", io, h->in[0]);
        CODAE_REQUIRE((reinterpret_cast<uintptr_t>(image_bf16) & 15) == 0, "codae_set_dataset_image: the image must be 16-byte aligned");
        im.data = data; im.image = image_bf16; im.n_rows = n_rows; im.io = io;
    }
    h->tc.img = im;
    return CODAE_OK;
}

int codae_set_optimizer(codae_handle h, const codae_optimizer* opt) {
    CODAE_REQUIRE(h != nullptr, "codae_set_optimizer: null handle");
    int rc = check_optimizer(opt);
    if (rc) return rc;
    CODAE_REQUIRE(!is_trust_kind(opt) || h->L <= CODAE_TRUST_MAX_MATRICES, "optimizer: lamb / lars take at most %d matrices, the stack has %d",
                  CODAE_TRUST_MAX_MATRICES, h->L);
    // (the graph key compares bytes and the struct has padding in front of its second pointer: zeroed here, then field by field)
    const codae_optimizer c = optimizer_canonical(opt);
    codae_optimizer& d = h->tc.opt;
    memset(&d, 0, sizeof(d));
    d.kind = c.kind; d.amsgrad = c.amsgrad; d.momentum = c.momentum; d.nesterov = c.nesterov; d.sched = c.sched; d.warmup = c.warmup;
    d.total = c.total; d.period = c.period; d.min_factor = c.min_factor; d.gamma = c.gamma; d.vmax = c.vmax;
    d.trust_clip = c.trust_clip; d.trust_coef = c.trust_coef; d.decay_bias = c.decay_bias; d.trust_ws = c.trust_ws;
    return CODAE_OK;
}

int64_t codae_trust_ws_bytes(codae_handle h) {
    if (h == nullptr) return 0;
    int64_t flat = 0, tiled = 0;
    for (int l = 0; l < h->L; ++l) {
        flat += trust_parts_flat((int64_t)h->out[l] * h->in[l]);
        tiled += trust_parts_tiled(h->out[l], h->in[l]);
    }
    return CODAE_TRUST_MAX_MATRICES * (int64_t)sizeof(float) + 2 * (int64_t)sizeof(double) * (flat > tiled ? flat : tiled);
}

int codae_set_weight_average(codae_handle h, const codae_weight_average* wa) {
    CODAE_REQUIRE(h != nullptr, "codae_set_weight_average: null handle");
    int rc = check_weight_average(wa, true);
    if (rc) return rc;
    // (the graph key compares bytes and the struct has four bytes of padding in front of its pointer: zeroed here, then field by field)
    const codae_weight_average c = weight_average_canonical(wa);
    codae_weight_average& d = h->tc.avg;
    memset(&d, 0, sizeof(d));
    d.kind = c.kind; d.decay = c.decay; d.debias = c.debias; d.start = c.start; d.every = c.every; d.avg = c.avg;
    return CODAE_OK;
}

int codae_set_tied_weights(codae_handle h, int32_t on) {
    CODAE_REQUIRE(h != nullptr, "codae_set_tied_weights: null handle");
    if (on) {
        for (int l = 0; l < h->L / 2; ++l) {
            const int m = h->L - 1 - l;
            if (h->in[l] != h->out[m] || h->out[l] != h->in[m]) {
                set_error("tied weights: layers %d and %d are not mirror images (%d -> %d against %d -> %d)", l, m, h->in[l], h->out[l],
                          h->in[m], h->out[m]);
                return CODAE_E_UNSUPPORTED;
            }
        }
        h->tie_pairs.clear();
        for (int l = 0; l < h->L / 2; ++l) {
            codae_tie_pair p{};
            p.enc_off = h->w_off[l]; p.dec_off = h->w_off[h->L - 1 - l]; p.rows = h->out[l]; p.cols = h->in[l];
            h->tie_pairs.push_back(p);
        }
    }
    h->tc.tied = on ? 1 : 0;             // (tied_reserved stays zero: the graph key compares bytes)
    return CODAE_OK;
}

int codae_graph_captures(codae_handle h) { return h != nullptr ? h->graph_captures : 0; }

int codae_set_hidden_dropout(codae_handle h, const codae_dropout* d) {
    CODAE_REQUIRE(h != nullptr, "codae_set_hidden_dropout: null handle");
    codae_engine::DropCfg c{};           // (built field by field: the graph key compares bytes, padding included)
    if (d != nullptr) {
        CODAE_REQUIRE(d->n == h->L - 1, "codae_set_hidden_dropout: %d values for %d hidden outputs (n_layers - 1)", d->n, h->L - 1);
        CODAE_REQUIRE(d->n == 0 || d->p != nullptr, "codae_set_hidden_dropout: null p");
        for (int l = 0; l < d->n; ++l) {
            char who[64];
            snprintf(who, sizeof(who), "codae_set_hidden_dropout: layer %d", l);
            int rc = check_dropout_p(d->p[l], who);
            if (rc) return rc;
        }
        for (int l = 0; l < d->n; ++l) {
            if (!(d->p[l] > 0.f)) continue;
            if (h->act[l] != CODAE_ACT_NONE && h->act[l] != CODAE_ACT_LEAKY) {
                // (the backward takes the derivative from the saved output, which dropout rescales)
                set_error("codae_set_hidden_dropout: layer %d: dropout after activation kind %d is not supported (NONE, RELU and LEAKY only)",
                          l, (int)h->act[l]);
                return CODAE_E_UNSUPPORTED;
            }
            c.p[l] = d->p[l];
            c.on = 1;
        }
        if (c.on) c.seed = d->seed;
    }
    h->tc.drop = c;
    return CODAE_OK;
}

// The canonical flags of a codae_residual on this stack (all zero = off) and the layout of its work space: G of the widest skipped
// layer first, then the masks.  CODAE_E_INVALID / CODAE_E_UNSUPPORTED as codae_set_residual documents.
static int residual_layout(codae_handle h, const codae_residual* r, const char* who, uint8_t* on, std::vector<int64_t>* bits_off, int64_t* bytes) {
    memset(on, 0, 64);
    if (bits_off) bits_off->assign(h->L, -1);
    *bytes = 0;
    if (r == nullptr) return CODAE_OK;
    return stream_layout(h, who, r->n, r->on, "skip", "skipped", true, on, bits_off, bytes, [&](const uint8_t* flagged) {
        int maxw = 0;
        for (int l = 0; l < h->L; ++l)
            if (flagged[l] && h->out[l] > maxw) maxw = h->out[l];
        return round_up((int64_t)h->max_batch * maxw * 4, 256);
    });
}

int64_t codae_residual_ws_bytes(codae_handle h, const codae_residual* r) {
    if (h == nullptr) { set_error("codae_residual_ws_bytes: null handle"); return -1; }
    uint8_t on[64];
    int64_t bytes = 0;
    return residual_layout(h, r, "codae_residual_ws_bytes", on, nullptr, &bytes) == CODAE_OK ? bytes : -1;
}

int codae_set_residual(codae_handle h, const codae_residual* r, void* ws, int64_t ws_bytes) {
    CODAE_REQUIRE(h != nullptr, "codae_set_residual: null handle");
    codae_engine::ResCfg c{};            // (built field by field: the graph key compares bytes)
    std::vector<int64_t> bits_off;
    int64_t need = 0;
    int rc = residual_layout(h, r, "codae_set_residual", c.on, &bits_off, &need);
    if (rc) return rc;
    if (need > 0) {
        rc = check_stream_ws("codae_set_residual", ws, ws_bytes, need);
        if (rc) return rc;
        c.ws = ws; c.ws_bytes = ws_bytes; c.any = 1;
    }
    rc = refuse_on_sparse_layer(h, "codae_set_residual", c.on, "skip");
    if (rc) return rc;
    h->tc.res = c;
    h->res_bits_off = bits_off;
    h->res_bits_live = false;
    return CODAE_OK;
}

// The canonical flags of a codae_norm on this stack (all zero = off) and the layout of its work space: r of every normalised layer
// first, then the masks.  CODAE_E_INVALID / CODAE_E_UNSUPPORTED as codae_set_norm documents.
static int norm_layout(codae_handle h, const codae_norm* n, const char* who, uint8_t* on, std::vector<int64_t>* r_off, std::vector<int64_t>* bits_off,
                       int64_t* bytes) {
    memset(on, 0, 64);
    if (r_off) r_off->assign(h->L, -1);
    if (bits_off) bits_off->assign(h->L, -1);
    *bytes = 0;
    if (n == nullptr) return CODAE_OK;
    CODAE_REQUIRE(n->kind == CODAE_NORM_LAYER || n->kind == CODAE_NORM_RMS, "%s: kind %d is neither CODAE_NORM_LAYER nor CODAE_NORM_RMS", who, n->kind);
    CODAE_REQUIRE(n->eps > 0.f && n->eps <= 3.402823466e38f, "%s: eps %g must be finite and > 0", who, (double)n->eps);
    return stream_layout(h, who, n->n, n->on, "norm", "normalised", false, on, bits_off, bytes, [&](const uint8_t* flagged) {
        int64_t off = 0;
        for (int l = 0; l < h->L; ++l) {
            if (!flagged[l]) continue;
            if (r_off) (*r_off)[l] = off;
            off += round_up((int64_t)h->max_batch * 4, 256);
        }
        return off;
    });
}

int64_t codae_norm_ws_bytes(codae_handle h, const codae_norm* n) {
    if (h == nullptr) { set_error("codae_norm_ws_bytes: null handle"); return -1; }
    uint8_t on[64];
    int64_t bytes = 0;
    return norm_layout(h, n, "codae_norm_ws_bytes", on, nullptr, nullptr, &bytes) == CODAE_OK ? bytes : -1;
}

int codae_set_norm(codae_handle h, const codae_norm* n, void* ws, int64_t ws_bytes) {
    CODAE_REQUIRE(h != nullptr, "codae_set_norm: null handle");
    codae_engine::NormCfg c{};           // (built field by field: the graph key compares bytes)
    std::vector<int64_t> r_off, bits_off;
    int64_t need = 0;
    int rc = norm_layout(h, n, "codae_set_norm", c.on, &r_off, &bits_off, &need);
    if (rc) return rc;
    if (need > 0) {
        rc = check_stream_ws("codae_set_norm", ws, ws_bytes, need);
        if (rc) return rc;
        c.ws = ws; c.ws_bytes = ws_bytes; c.any = 1; c.kind = n->kind; c.eps = n->eps;
    }
    rc = refuse_on_sparse_layer(h, "codae_set_norm", c.on, "norm");
    if (rc) return rc;
    h->tc.norm = c;
    h->norm_r_off = r_off;
    h->norm_bits_off = bits_off;
    h->norm_bits_live = false;
    return CODAE_OK;
}

// The canonical form of a codae_sparse_code on this stack (all zero = off: NULL, or keep == the width of the code) and the bytes of
// its work space, the 1-bit keep mask.  CODAE_E_INVALID / CODAE_E_UNSUPPORTED as codae_set_sparse_code documents.
static int sparse_layout(codae_handle h, const codae_sparse_code* c, const char* who, codae_engine::SparseCfg* out, int64_t* bytes) {
    *out = codae_engine::SparseCfg{};
    *bytes = 0;
    if (c == nullptr) return CODAE_OK;
    CODAE_REQUIRE(c->layer >= 1 && c->layer <= h->L, "%s: layer %d outside [1, %d]", who, c->layer, h->L - 1);
    const int m = c->layer - 1;
    char why[160] = "";
    if (m == h->L - 1) snprintf(why, sizeof(why), "the last layer's output is the reconstruction and takes no sparse code");
    else if (h->act[m] != CODAE_ACT_NONE && h->act[m] != CODAE_ACT_LEAKY)
        snprintf(why, sizeof(why), "the sparse layer's activation must be none, ReLU or LeakyReLU");
    else if (h->tc.res.any && h->tc.res.on[m])
        snprintf(why, sizeof(why), "the sparse layer takes no skip (it would add the dense h_%d back): name the layers and leave out layer %d", m, m);
    else if (h->tc.norm.any && h->tc.norm.on[m])
        snprintf(why, sizeof(why), "the sparse layer takes no norm (its backward needs the full xhat): name the layers and leave out layer %d", m);
    if (why[0] != 0) {
        set_error("%s: layer %d (%d -> %d, activation kind %d): %s", who, m, h->in[m], h->out[m], h->relu[m] ? CODAE_ACT_RELU : (int)h->act[m], why);
        return CODAE_E_UNSUPPORTED;
    }
    CODAE_REQUIRE(c->keep >= 1 && c->keep <= h->out[m], "%s: keep %d outside [1, %d], the width of layer %d's output", who, c->keep, h->out[m], m);
    if (c->keep == h->out[m]) return CODAE_OK;                 // every unit kept: off
    out->on = 1; out->m = m; out->keep = c->keep;
    *bytes = round_up((int64_t)h->max_batch * ((h->out[m] + 7) / 8), 256);
    return CODAE_OK;
}

int64_t codae_sparse_code_ws_bytes(codae_handle h, const codae_sparse_code* c) {
    if (h == nullptr) { set_error("codae_sparse_code_ws_bytes: null handle"); return -1; }
    codae_engine::SparseCfg cfg;
    int64_t bytes = 0;
    return sparse_layout(h, c, "codae_sparse_code_ws_bytes", &cfg, &bytes) == CODAE_OK ? bytes : -1;
}

int codae_set_sparse_code(codae_handle h, const codae_sparse_code* c, void* ws, int64_t ws_bytes) {
    CODAE_REQUIRE(h != nullptr, "codae_set_sparse_code: null handle");
    codae_engine::SparseCfg cfg;         // (built field by field from zero: the graph key compares bytes)
    int64_t need = 0;
    int rc = sparse_layout(h, c, "codae_set_sparse_code", &cfg, &need);
    if (rc) return rc;
    if (need > 0) {
        rc = check_stream_ws("codae_set_sparse_code", ws, ws_bytes, need);
        if (rc) return rc;
        cfg.ws = ws; cfg.ws_bytes = ws_bytes;
    }
    h->tc.sparse = cfg;
    h->sparse_bits_live = false;
    return CODAE_OK;
}

int codae_eval_step(codae_handle h, const codae_buffers* b, const codae_batch* batch, float* out_y, void* stream) {
    return codae_step_forward_loss(h, b, batch, nullptr, out_y, stream);
}

// Assemble the leave-one-out rows of Q outfits into act[0], run the evaluation's forward launches over them (run_linear per layer, the
// last one into the fp32 output buffer) and score them: no noise, no dropout, no criterion, no loss kernel - the metric sums are not
// touched -, the presence table consulted by ITEM row, never by batch position.  bf16 engine: the rows come from the registered bf16
// image when `data` is the dataset it was made from (the same bits as rounding the fp32 rows).
int codae_score_outfits(codae_handle h, const codae_buffers* b, const float* data, int64_t n_rows, const int32_t* items, int32_t Q,
                        int32_t n_slots, float* cos, float* sq, float* score, int32_t* n_present, void* stream) {
    CODAE_REQUIRE(h != nullptr && b != nullptr, "null handle or buffers");
    const int L = h->L, io = h->in[0];
    CODAE_REQUIRE(io == h->out[L - 1], "codae_score_outfits: the model maps %d columns to %d", io, h->out[L - 1]);
    CODAE_REQUIRE(n_slots >= 1 && n_slots <= 128, "codae_score_outfits: 1 .. 128 slots, got %d", n_slots);
    CODAE_REQUIRE(io % n_slots == 0, "codae_score_outfits: n_slots %d does not divide io %d", n_slots, io);
    CODAE_REQUIRE(Q >= 1, "codae_score_outfits: Q %d must be at least 1", Q);
    CODAE_REQUIRE((int64_t)Q * n_slots <= h->max_batch, "codae_score_outfits: %d outfits of %d slots exceed max_batch %d", Q, n_slots,
                  h->max_batch);
    CODAE_REQUIRE(data && items && cos && sq && score && n_present && n_rows > 0, "codae_score_outfits: null argument, or no rows");
    const uint8_t* const pres = h->tc.pres.table;
    CODAE_REQUIRE(pres == nullptr || (h->tc.pres.n_slots == n_slots && h->tc.pres.n_rows == n_rows),
                  "codae_score_outfits: the presence table is [%lld][%d], the outfits index [%lld][%d]", (long long)h->tc.pres.n_rows,
                  h->tc.pres.n_slots, (long long)n_rows, n_slots);
    const int B = Q * n_slots;
    int rc = check_common(h, b, B);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const bool bf = h->prec == CODAE_PREC_BF16;
    const int rows = h->rows_for(B);
    forward_leaves(h, nullptr, nullptr);      // (an evaluation forward)
    const codae_engine::ImageCfg& im = h->tc.img;
    const bool from_image = bf && !h->cfg.no_dataset_image && im.image != nullptr && data == im.data && io == im.io && n_rows == im.n_rows;
    {
        ProfScope prof(h, CODAE_K_GATHER, s);
        rc = launch_assemble_outfits(from_image ? im.image : (const void*)data, from_image, n_rows, io, n_slots, items, Q, nullptr, 1, pres,
                                     act_ptr(h, b, 0), bf, h->in_ld[0], s);
    }
    if (rc) return rc;
    rc = zero_pad_rows(h, act_ptr(h, b, 0), B, rows, h->in_ld[0], s);
    if (rc) return rc;
    float* y = reinterpret_cast<float*>(act_ptr(h, b, L));
    for (int l = 0; l < L; ++l) {
        rc = run_forward_layer(h, b, l, l == L - 1 ? y : nullptr, B, rows, false, s);
        if (rc) return rc;
    }
    return launch_outfit_scores(data, n_rows, io, n_slots, items, Q, pres, y, io, cos, sq, score, n_present, s);
}

// Outfit codes.  The dense fp32 rows of `x` into act[l] in working precision, as codae_forward ingests its input; the pad rows cleared.
static int ingest_dense(codae_handle h, const codae_buffers* b, const float* x, int B, int rows, int l, hipStream_t s) {
    codae_batch in{};
    in.data = x; in.B = B; in.io = h->in[l];
    int rc = launch_gather_noise(&in, nullptr, 0, nullptr, act_ptr(h, b, l), h->prec == CODAE_PREC_BF16, s, h->in_ld[l]);
    if (rc) return rc;
    return zero_pad_rows(h, act_ptr(h, b, l), B, rows, h->in_ld[l], s);
}

// h_layers of an evaluation forward: every layer lands in act[l + 1], so its skip and its norm run (codae_forward's partial range
// writes the last Linear straight into the caller's tensor and would lose them); then the stored rows leave through the export kernel.
int codae_encode(codae_handle h, const codae_buffers* b, const float* x, int32_t B, int32_t layers, float* code, float* norm, void* stream) {
    int rc = check_common(h, b, B);
    if (rc) return rc;
    CODAE_REQUIRE(x && code, "codae_encode: null x or code");
    CODAE_REQUIRE(layers >= 1 && layers <= h->L - 1, "codae_encode: %d layers outside [1, %d]", layers, h->L - 1);
    hipStream_t s = (hipStream_t)stream;
    const int rows = h->rows_for(B);
    forward_leaves(h, nullptr, nullptr);      // (an evaluation forward)
    rc = ingest_dense(h, b, x, B, rows, 0, s);
    if (rc) return rc;
    for (int l = 0; l < layers; ++l) {
        rc = run_forward_layer(h, b, l, nullptr, B, rows, false, s);
        if (rc) return rc;
    }
    ProfScope prof(h, CODAE_K_DROPOUT, s);     // the class of the streaming kernels between the GEMMs
    return launch_export_rows(act_ptr(h, b, layers), h->prec == CODAE_PREC_BF16, h->in_ld[layers], B, h->in[layers], code, h->in[layers], norm, s);
}

// Linears layer_lo .. L - 1 on a code: it becomes act[layer_lo] (a skip around Linear layer_lo reads it there), the last Linear
// writes the caller's fp32 tensor as every evaluation's does.
int codae_decode(codae_handle h, const codae_buffers* b, const float* code, int32_t B, int32_t layer_lo, float* y, void* stream) {
    int rc = check_common(h, b, B);
    if (rc) return rc;
    CODAE_REQUIRE(code && y, "codae_decode: null code or y");
    CODAE_REQUIRE(layer_lo >= 1 && layer_lo <= h->L - 1, "codae_decode: layer %d outside [1, %d]", layer_lo, h->L - 1);
    hipStream_t s = (hipStream_t)stream;
    const int rows = h->rows_for(B), L = h->L;
    forward_leaves(h, nullptr, nullptr);
    rc = ingest_dense(h, b, code, B, rows, layer_lo, s);
    if (rc) return rc;
    for (int l = layer_lo; l < L; ++l) {
        rc = run_forward_layer(h, b, l, l == L - 1 ? y : nullptr, B, rows, false, s);
        if (rc) return rc;
    }
    return CODAE_OK;
}

// a layer range of the step's backward; join: the call returns with `stream` waiting for the side stream
static int step_backward(const char* who, codae_handle h, const codae_buffers* b, int B, int layer_lo, int layer_hi, bool join, void* stream) {
    int rc = check_common(h, b, B);
    if (rc) return rc;
    CODAE_REQUIRE(b->grads && b->dacts, "%s: grads / dacts missing", who);
    CODAE_REQUIRE(layer_lo >= 0 && layer_lo < layer_hi && layer_hi <= h->L, "%s: layer range [%d, %d)", who, layer_lo, layer_hi);
    const StepCall call{STEP_BACKWARD, B, layer_lo, layer_hi, join, false, false, false};
    return backward_range(h, b, call, step_plan(h, b, call), nullptr, (hipStream_t)stream);
}

int codae_step_backward(codae_handle h, const codae_buffers* b, int32_t B, int32_t layer_lo, int32_t layer_hi, void* stream) {
    return step_backward("codae_step_backward", h, b, B, layer_lo, layer_hi, true, stream);
}

int codae_step_backward_async(codae_handle h, const codae_buffers* b, int32_t B, int32_t layer_lo, int32_t layer_hi, void* stream) {
    return step_backward("codae_step_backward_async", h, b, B, layer_lo, layer_hi, false, stream);
}

int codae_side_stream(codae_handle h, void** out) {
    CODAE_REQUIRE(h && out, "codae_side_stream: null argument");
    *out = nullptr;
    if (!two_streams(h)) return CODAE_OK;           // everything runs on the caller's stream
    int rc = ensure_side_stream(h);
    if (rc) return rc;
    *out = h->side;
    return CODAE_OK;
}

// The update behind a backward: what earlier calls left open (side stream, pending bias rows), the tied fold, the norm where plan.norm
// leaves it to a flat pass, then the kernels plan.update names over the free parameters.
static int update_impl(codae_handle h, const codae_buffers* b, const codae_hyper* hyper, hipStream_t s, const StepPlan& plan) {
    CODAE_REQUIRE(b->params && b->grads && b->adam_m && b->adam_v && b->scalars, "codae_step_update: buffer missing");
    int rc = join_side(h, s);                 // (a backward issued with codae_step_backward_async)
    if (rc) return rc;
    if (bias_pending_from(h, 0) && b->bias_parts != nullptr) {               // (a bucketed backward that did not reach layer 0)
        rc = finish_bias(h, b, s, false);
        if (rc) return rc;
    }
    // tied weights: the decoder matrices' gradients are folded into the encoder's (behind every reduce of a data-parallel step, which
    // ends here) and left +0: the flat vector is the gradient of the tied parameter set, and the flat norm below counts it once
    const bool tied = h->tc.tied != 0 && !h->tie_pairs.empty();
    if (tied) {
        ProfScope prof(h, CODAE_K_SUMSQ, s);
        rc = launch_tie_fold(b->grads, h->tie_pairs.data(), (int)h->tie_pairs.size(), s);
        if (rc) return rc;
    }
    const bool scalars_zero = h->norm_scalars_zero;
    h->norm_scalars_zero = false;
    if (plan.norm == NORM_FLAT) {
        ProfScope prof(h, CODAE_K_SUMSQ, s);
        // (cleared here for a stand-alone update: no step_forward_loss of this step did it)
        rc = launch_grad_sumsq(b->grads, h->n_param, b->scalars, !scalars_zero, s);
        if (rc) return rc;
    }
    const bool bf = h->prec == CODAE_PREC_BF16;
    bf16_t* shadow = bf ? reinterpret_cast<bf16_t*>(b->shadow_w) : nullptr;
    bf16_t* shadow_t = bf ? reinterpret_cast<bf16_t*>(b->shadow_wt) : nullptr;
    CODAE_REQUIRE(!bf || shadow, "codae_step_update: shadow_w missing");
    // (Measured and dropped: per-layer Adam kernels on the side stream beside the NEXT forward - HBM / L2 contention
    // slowed those GEMMs from 46.8 to 56.9 us each and the step from 1.76 to 1.84 ms.)
    ProfScope prof(h, CODAE_K_ADAM, s);
    // the weight average rides in every launch below, at the offsets of p
    UpdateLaunch u{};
    u.x = ParamVectors{b->params, b->grads, b->adam_m, b->adam_v, h->tc.opt.vmax, h->tc.avg.avg, shadow};
    u.n = h->n_param; u.hp = hyper; u.grad_sq = b->scalars + CODAE_S_GRAD_SQ; u.step_dev = step_dev(h, b);
    u.opt = &h->tc.opt; u.wa = &h->tc.avg;
    // tied: the free parameters only - the encoder matrices (and the middle one of an odd stack) and every bias; the moments of the
    // decoder matrices are neither read nor written - then the decoder's three images from the updated encoder
    const int n_mats = tied ? h->n_free() : h->L;
    // LAMB / LARS: the norms of every free matrix and their ratios first (two launches on the tiled path, whatever the depth), then
    // the update, which reads its matrix's ratio in its prologue
    const bool trust = is_trust_kind(&h->tc.opt);
    if (plan.update == UPDATE_TILED) {
        // one tiled pass: p, m, v, the bf16 shadow and the transposed shadow of every layer that has a data gradient
        const UpdateTiles tiles{shadow_t, n_mats, h->w_off.data(), h->out.data(), h->in.data(), 1, h->bias_begin, h->n_param - h->bias_begin};
        if (trust) {
            rc = launch_trust_norms_tiled(u, tiles, s);
            if (rc) return rc;
        }
        rc = launch_update_tiled(u, tiles, s);
        if (rc) return rc;
    } else if (trust) {
        // the flat kernel once per matrix (its own ratio; the padding behind a matrix stays as it is: zero) and once for the bias block
        std::vector<int64_t> len(n_mats);
        for (int l = 0; l < n_mats; ++l) len[l] = (int64_t)h->out[l] * h->in[l];
        rc = launch_trust_norms(u, n_mats, h->w_off.data(), len.data(), s);
        if (rc) return rc;
        for (int l = 0; l <= n_mats; ++l) {
            UpdateLaunch span = u;
            const int64_t lo = l < n_mats ? h->w_off[l] : h->bias_begin;
            span.x = u.x.at(lo); span.n = l < n_mats ? len[l] : h->n_param - h->bias_begin; span.trust_mat = l < n_mats ? l : -1;
            rc = launch_update(span, s);
            if (rc) return rc;
        }
        rc = refresh_transposed(h, b, s, 1, n_mats);
        if (rc) return rc;
    } else {
        const int64_t mats_end = tied ? h->w_off[n_mats] : h->n_param;         // (untied: one span, matrices and biases)
        const int64_t spans[2][2] = {{0, mats_end}, {h->bias_begin, h->n_param}};
        for (int i = 0; i < (tied ? 2 : 1); ++i) {
            UpdateLaunch span = u;
            span.x = u.x.at(spans[i][0]); span.n = spans[i][1] - spans[i][0];
            rc = launch_update(span, s);
            if (rc) return rc;
        }
        rc = refresh_transposed(h, b, s, 1, n_mats);
        if (rc) return rc;
    }
    return tied ? launch_tie_mirror(b->params, shadow, shadow_t, h->tie_pairs.data(), (int)h->tie_pairs.size(), s) : CODAE_OK;
}

int codae_step_update(codae_handle h, const codae_buffers* b, const codae_hyper* hyper, void* stream) {
    CODAE_REQUIRE(h && b && hyper, "codae_step_update: null argument");
    return update_impl(h, b, hyper, (hipStream_t)stream, step_plan(h, b, update_call(hyper)));
}

int codae_span_sumsq(const float* g, int64_t n, double* acc, void* stream) {
    return launch_sumsq_to(g, n, acc, (hipStream_t)stream);
}

int codae_step_update_span(codae_handle h, const codae_buffers* b, const codae_hyper* hyper, int64_t lo, int64_t hi,
                           const double* total_sq, void* stream) {
    CODAE_REQUIRE(h && b && hyper, "codae_step_update_span: null argument");
    CODAE_REQUIRE(b->params && b->grads && b->adam_m && b->adam_v && b->scalars, "codae_step_update_span: buffer missing");
    CODAE_REQUIRE(lo >= 0 && lo < hi && hi <= h->n_param && lo % 4 == 0 && hi % 4 == 0, "codae_step_update_span: range [%lld, %lld)",
                  (long long)lo, (long long)hi);
    CODAE_REQUIRE(hyper->max_grad_norm <= 0.f || total_sq != nullptr, "codae_step_update_span: clipping needs the global sum g^2");
    if (h->tc.tied && !h->tie_pairs.empty()) {
        set_error("tied weights: the sharded update is not supported: the tied layers %d and %d lie in different shards", 0, h->L - 1);
        return CODAE_E_UNSUPPORTED;
    }
    if (h->tc.avg.kind != CODAE_AVG_OFF) {
        set_error("weight average: the sharded update is not supported: the average of a shard would have to be all-gathered too");
        return CODAE_E_UNSUPPORTED;
    }
    if (is_trust_kind(&h->tc.opt)) {
        set_error("%s: the sharded update is not supported: a matrix's norm spans shards", h->tc.opt.kind == CODAE_OPT_LAMB ? "lamb" : "lars");
        return CODAE_E_UNSUPPORTED;
    }
    hipStream_t s = (hipStream_t)stream;
    int rc = join_side(h, s);
    if (rc) return rc;
    h->norm_scalars_zero = false;
    const double* coef = nullptr;
    if (hyper->max_grad_norm > 0.f) {
        rc = launch_clip_coef(total_sq, hyper->max_grad_norm, b->scalars + CODAE_S_CLIP_COEF, s);
        if (rc) return rc;
        coef = b->scalars + CODAE_S_CLIP_COEF;
    }
    bf16_t* shadow = h->prec == CODAE_PREC_BF16 ? reinterpret_cast<bf16_t*>(b->shadow_w) : nullptr;
    CODAE_REQUIRE(h->prec != CODAE_PREC_BF16 || shadow, "codae_step_update_span: shadow_w missing");
    ProfScope prof(h, CODAE_K_ADAM, s);
    UpdateLaunch u{};
    u.x = ParamVectors{b->params, b->grads, b->adam_m, b->adam_v, h->tc.opt.vmax, nullptr, shadow}.at(lo);
    u.n = hi - lo; u.hp = hyper; u.coef_in = coef; u.opt = &h->tc.opt;
    return launch_update(u, s);
}

int codae_sync_transposed(codae_handle h, const codae_buffers* b, void* stream) {
    CODAE_REQUIRE(h && b, "codae_sync_transposed: null argument");
    return refresh_transposed(h, b, (hipStream_t)stream);
}

int codae_join(codae_handle h, void* stream) {
    CODAE_REQUIRE(h != nullptr, "codae_join: null handle");
    return join_side(h, (hipStream_t)stream);
}

int codae_step_path(codae_handle h, const codae_buffers* b, int32_t B) {
    if (h == nullptr || b == nullptr || B <= 0 || B > h->max_batch) return 0;
    return step_plan(h, b, StepCall{STEP_TRAIN, B, 0, h->L, true, false, false, false}).path;
}

int codae_step_stores_output(codae_handle h, const codae_buffers* b, int32_t B) {
    if (h == nullptr || b == nullptr || B <= 0 || B > h->max_batch) return 0;
    const StepPlan p = step_plan(h, b, StepCall{STEP_TRAIN, B, 0, h->L, true, false, false, false});
    return p.path == PATH_LAYERS && p.loss == LOSS_STANDALONE ? 1 : 0;
}

int codae_train_step(codae_handle h, const codae_buffers* b, const codae_batch* batch, const codae_hyper* hyper, void* stream) {
    CODAE_REQUIRE(hyper != nullptr, "codae_train_step: null hyper");
    CODAE_REQUIRE(batch != nullptr, "codae_train_step: null batch");
    CODAE_REQUIRE(h != nullptr && b != nullptr, "null handle or buffers");
    const StepCall call{STEP_TRAIN, batch->B, 0, h->L, true, false, false, hyper->max_grad_norm > 0.f};
    const StepPlan plan = step_plan(h, b, call);
    hipStream_t s = (hipStream_t)stream;
    LossFinish lf{};                 // (filled when the loss finish is left to the backward's bias-finish launch)
    int rc;
    if (plan.path == PATH_CHAIN) {
        rc = check_common(h, b, batch->B);
        if (rc) return rc;
        CODAE_REQUIRE(batch->io == h->in[0], "batch.io %d does not match the model (%d)", batch->io, h->in[0]);
        CODAE_REQUIRE(b->grads && b->dacts && b->scalars && b->bias_parts, "codae_train_step: grads / dacts / scalars / bias_parts missing");
        CODAE_REQUIRE(batch->data && batch->B > 0 && (!(batch->mask_id || batch->mask_to_use) || batch->mask_table), "codae_train_step: bad batch");
        CODAE_REQUIRE(!batch->mask_to_use || batch->mask_id || (batch->nb_run > 0 && batch->run >= 0 && batch->run < batch->nb_run),
                      "codae_train_step: run %d outside [0, %d)", batch->run, batch->nb_run);
        if (h->prof_on) ++h->prof_step;
        rc = join_side(h, s);
        if (rc) return rc;
        forward_leaves(h, batch, hyper);                           // (the chain runs without dropout, skips or a norm: all clear)
        rc = run_chain(h, b, batch, hyper, s, &lf);                // (forward, loss and every data gradient)
        if (rc) return rc;
        rc = run_grouped_tail(h, b, plan, s, &lf);
    } else {
        rc = forward_loss_impl(h, b, batch, hyper, nullptr, stream, plan, &lf);
        if (rc) return rc;
        // (codae_step_backward's argument checks - check_common, grads / dacts - were made by the forward just above)
        rc = backward_range(h, b, call, plan, nullptr, s, lf.scalars != nullptr ? &lf : nullptr);
    }
    if (rc) return rc;
    return update_impl(h, b, hyper, s, plan);
}

static bool same_bytes(const void* a, const void* b, size_t n) { return memcmp(a, b, n) == 0; }

int codae_train_step_graph(codae_handle h, const codae_buffers* b, const codae_batch* batch, const codae_hyper* hyper, void* stream) {
    CODAE_REQUIRE(h && b && batch && hyper, "codae_train_step_graph: null argument");
    CODAE_REQUIRE(!h->prof_on, "codae_train_step_graph: launch profiling (codae_profile_begin) cannot run inside a graph");
    CODAE_REQUIRE(b->scalars != nullptr, "codae_train_step_graph: scalars missing");
    CODAE_REQUIRE(stream != nullptr, "codae_train_step_graph: the default (null) stream cannot be captured - pass a created stream");
    if (h->variable_on()) {
        // the mixed-variable criterion is replayed on its own only: with the default Adam and none of the step's options
        const codae_optimizer none{};
        const char* with = h->tc.noise.kind != CODAE_NOISE_NONE ? "input noise" : h->tc.drop.on ? "hidden dropout" :
                           !same_bytes(&h->tc.opt, &none, sizeof(none)) ? "an optimizer setting (codae_set_optimizer)" :
                           h->tc.res.any ? "residual connections" : h->tc.norm.any ? "normalisation" : h->tc.sparse.on ? "the sparse code" :
                           h->tc.tied ? "tied weights" : h->tc.avg.kind != CODAE_AVG_OFF ? "the weight average" : nullptr;
        if (with != nullptr) {
            set_error("codae_train_step_graph: graph replay of the mixed-variable criterion together with %s is not supported: "
                      "run plain steps (codae_train_step)", with);
            return CODAE_E_UNSUPPORTED;
        }
    }
    hipStream_t s = (hipStream_t)stream;
    // what the captured kernel arguments depend on (the step count is the one thing that may change)
    codae_hyper hk = *hyper;
    hk.step = 0;
    const bool fresh = h->graph_exec == nullptr || !same_bytes(&h->graph_key.batch, batch, sizeof(*batch)) ||
                       !same_bytes(&h->graph_key.hyper, &hk, sizeof(hk)) || !same_bytes(&h->graph_key.bufs, b, sizeof(*b)) ||
                       !same_bytes(&h->graph_key.tc, &h->tc, sizeof(h->tc));
    if (fresh) {
        if (h->graph_exec) { (void)hipGraphExecDestroy(h->graph_exec); h->graph_exec = nullptr; }
        int rc = check_common(h, b, batch->B);
        if (rc) return rc;
        if (two_streams(h)) {
            rc = ensure_side_stream(h);                      // (no stream / event creation inside the capture)
            if (rc) return rc;
        }
        rc = codae_join(h, stream);                          // nothing recorded outside may be waited for inside
        if (rc) return rc;
        CODAE_HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed));
        h->capturing = true;
        rc = codae_train_step(h, b, batch, hyper, stream);
        h->capturing = false;
        hipGraph_t graph = nullptr;
        const hipError_t ee = hipStreamEndCapture(s, &graph);
        if (rc != CODAE_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
        if (ee != hipSuccess || graph == nullptr) {
            set_error("codae_train_step_graph: stream capture failed: %s", hipGetErrorString(ee));
            return CODAE_E_HIP;
        }
        const hipError_t ei = hipGraphInstantiate(&h->graph_exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (ei != hipSuccess) {
            h->graph_exec = nullptr;
            set_error("codae_train_step_graph: hipGraphInstantiate failed: %s", hipGetErrorString(ei));
            return CODAE_E_HIP;
        }
        h->graph_key.batch = *batch; h->graph_key.hyper = hk; h->graph_key.bufs = *b; h->graph_key.tc = h->tc;
        ++h->graph_captures;
    }
    int rc = launch_set_scalar(b->scalars + CODAE_S_ADAM_STEP, (double)hyper->step, s);
    if (rc) return rc;
    CODAE_HIP_CHECK(hipGraphLaunch(h->graph_exec, s));
    return CODAE_OK;
}

// ---- data parallel with a library-owned RCCL communicator --------------------------------

int codae_dp_unique_id(void* out, int32_t capacity) {
    CODAE_REQUIRE(out != nullptr && capacity >= (int32_t)sizeof(ncclUniqueId), "codae_dp_unique_id: need %d bytes", (int)sizeof(ncclUniqueId));
    int rc = rccl_load();
    if (rc) return rc;
    ncclUniqueId id;
    CODAE_RCCL_CHECK(g_rccl.GetUniqueId(&id));
    memcpy(out, &id, sizeof(id));
    return CODAE_OK;
}

int codae_dp_init(codae_handle h, const void* unique_id, int32_t rank, int32_t world) {
    CODAE_REQUIRE(h != nullptr && unique_id != nullptr && world >= 1 && rank >= 0 && rank < world, "codae_dp_init: bad arguments");
    CODAE_REQUIRE(h->dp == nullptr, "codae_dp_init: this engine already has a communicator");
    if (h->variable_on()) {
        set_error("data parallel is not supported with the mixed-variable criterion: a global-batch RMSE is not a sum over shards");
        return CODAE_E_UNSUPPORTED;
    }
    int rc = rccl_load();
    if (rc) return rc;
    DpState* d = new DpState();
    d->rank = rank; d->world = world;
    ncclUniqueId id;
    memcpy(&id, unique_id, sizeof(id));
    ncclResult_t r = g_rccl.CommInitRank(&d->comm, world, id, rank);          // (collective: every rank calls it)
    if (r != ncclSuccess) { set_error("ncclCommInitRank failed: %s", g_rccl.GetErrorString(r)); delete d; return CODAE_E_HIP; }
    int prio_least = 0, prio_greatest = 0;
    hipError_t e1 = hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    if (e1 == hipSuccess) e1 = hipStreamCreateWithPriority(&d->stream, hipStreamNonBlocking, prio_greatest);
    for (int i = 0; i <= CODAE_DP_MAX_BUCKETS && e1 == hipSuccess; ++i) e1 = hipEventCreateWithFlags(&d->ev_bucket[i], hipEventDisableTiming);
    if (e1 == hipSuccess) e1 = hipEventCreateWithFlags(&d->ev_done, hipEventDisableTiming);
    if (e1 != hipSuccess) {
        set_error("codae_dp_init: stream / event creation failed: %s", hipGetErrorString(e1));
        (void)g_rccl.CommDestroy(d->comm);
        delete d;
        return CODAE_E_HIP;
    }
    h->dp = d;
    return CODAE_OK;
}

int codae_dp_destroy(codae_handle h) {
    if (h == nullptr || h->dp == nullptr) return CODAE_OK;
    DpState* d = h->dp;
    if (d->stream) (void)hipStreamSynchronize(d->stream);
    if (d->comm) (void)g_rccl.CommDestroy(d->comm);
    for (int i = 0; i <= CODAE_DP_MAX_BUCKETS; ++i) if (d->ev_bucket[i]) (void)hipEventDestroy(d->ev_bucket[i]);
    if (d->ev_done) (void)hipEventDestroy(d->ev_done);
    if (d->stream) (void)hipStreamDestroy(d->stream);
    delete d;
    h->dp = nullptr;
    return CODAE_OK;
}

// One data-parallel optimizer step, collectives included: forward + loss; the backward bucket by bucket (layer ranges
// [lo_i, hi_i), top down, ending at layer 0), each bucket's weight gradients all-reduced (SUM, in place, fp32) on the
// communicator's own stream as soon as they exist on the engine's side stream - no host round trip between buckets -; the
// bias block last; then the caller's stream waits ONCE for the collectives and runs clip + Adam on the summed gradients.
// hyper->loss_scale_rows must hold the GLOBAL batch rows (so that the SUM is the global-batch mean gradient).
int codae_train_step_dp(codae_handle h, const codae_buffers* b, const codae_batch* batch, const codae_hyper* hyper, int32_t n_buckets,
                        const int32_t* bucket_lo, const int32_t* bucket_hi, void* stream) {
    CODAE_REQUIRE(h != nullptr && h->dp != nullptr, "codae_train_step_dp: codae_dp_init has not been called on this engine");
    CODAE_REQUIRE(b && batch && hyper && bucket_lo && bucket_hi, "codae_train_step_dp: null argument");
    CODAE_REQUIRE(n_buckets >= 1 && n_buckets <= CODAE_DP_MAX_BUCKETS, "codae_train_step_dp: %d buckets", n_buckets);
    CODAE_REQUIRE(bucket_hi[0] == h->L && bucket_lo[n_buckets - 1] == 0, "codae_train_step_dp: buckets must run from the top layer down to layer 0");
    for (int i = 0; i < n_buckets; ++i) {
        CODAE_REQUIRE(bucket_lo[i] >= 0 && bucket_lo[i] < bucket_hi[i] && (i == 0 || bucket_hi[i] == bucket_lo[i - 1]),
                      "codae_train_step_dp: bucket %d = [%d, %d) does not continue the one above it", i, bucket_lo[i], bucket_hi[i]);
    }
    if (h->variable_on()) {
        set_error("data parallel is not supported with the mixed-variable criterion: a global-batch RMSE is not a sum over shards");
        return CODAE_E_UNSUPPORTED;
    }
    DpState* d = h->dp;
    hipStream_t s = (hipStream_t)stream;
    int rc = codae_step_forward_loss(h, b, batch, hyper, nullptr, stream);
    if (rc) return rc;
    for (int i = 0; i < n_buckets; ++i) {
        const StepCall range{STEP_BACKWARD, batch->B, bucket_lo[i], bucket_hi[i], false, false, false, false};
        rc = backward_range(h, b, range, step_plan(h, b, range), nullptr, s);
        if (rc) return rc;
        // the bucket's weight gradients are complete, in order, on the side stream (or on s itself in single-stream mode)
        hipStream_t producer = h->side != nullptr && two_streams(h) ? h->side : s;
        CODAE_HIP_CHECK(hipEventRecord(d->ev_bucket[i], producer));
        CODAE_HIP_CHECK(hipStreamWaitEvent(d->stream, d->ev_bucket[i], 0));
        const int64_t lo_off = h->w_off[bucket_lo[i]];
        const int64_t hi_off = bucket_hi[i] < h->L ? h->w_off[bucket_hi[i]] : h->bias_begin;
        float* span = b->grads + lo_off;
        CODAE_RCCL_CHECK(g_rccl.AllReduce(span, span, (size_t)(hi_off - lo_off), ncclFloat, ncclSum, d->comm, d->stream));
    }
    rc = join_side(h, s);
    if (rc) return rc;
    // (the last range finished every bias gradient on s)
    CODAE_HIP_CHECK(hipEventRecord(d->ev_bucket[n_buckets], s));
    CODAE_HIP_CHECK(hipStreamWaitEvent(d->stream, d->ev_bucket[n_buckets], 0));
    float* bias = b->grads + h->bias_begin;
    CODAE_RCCL_CHECK(g_rccl.AllReduce(bias, bias, (size_t)(h->n_param - h->bias_begin), ncclFloat, ncclSum, d->comm, d->stream));
    CODAE_HIP_CHECK(hipEventRecord(d->ev_done, d->stream));
    CODAE_HIP_CHECK(hipStreamWaitEvent(s, d->ev_done, 0));
    return update_impl(h, b, hyper, s, step_plan(h, b, update_call(hyper)));
}

// what step_plan answers for a call described in integers (include/codae_hip.h); nothing is launched
int codae_debug_step_plan(codae_handle h, const codae_buffers* b, const int32_t* call, int32_t* out, int32_t capacity) {
    CODAE_REQUIRE(h != nullptr && b != nullptr && call != nullptr, "codae_debug_step_plan: null argument");
    CODAE_REQUIRE(out != nullptr && capacity >= CODAE_STEP_PLAN_FIELDS, "codae_debug_step_plan: needs room for %d fields", CODAE_STEP_PLAN_FIELDS);
    StepCall c{call[0], call[1], call[2], call[3], call[4] != 0, call[5] != 0, call[6] != 0, call[7] != 0};
    CODAE_REQUIRE(c.kind >= STEP_TRAIN && c.kind <= STEP_UPDATE, "codae_debug_step_plan: unknown kind %d", c.kind);
    CODAE_REQUIRE(c.kind == STEP_UPDATE || (c.B > 0 && c.B <= h->max_batch), "codae_debug_step_plan: batch %d outside (0, %d]", c.B, h->max_batch);
    if (c.kind == STEP_BACKWARD || c.kind == STEP_DROPIN_BACKWARD)
        CODAE_REQUIRE(c.layer_lo >= 0 && c.layer_lo < c.layer_hi && c.layer_hi <= h->L, "codae_debug_step_plan: layer range [%d, %d)", c.layer_lo, c.layer_hi);
    if (c.kind == STEP_TRAIN) { c.layer_lo = 0; c.layer_hi = h->L; c.join = true; c.want_dx = false; c.has_out_y = false; }      // (as codae_train_step)
    const StepPlan p = step_plan(h, b, c);
    const int32_t fields[CODAE_STEP_PLAN_FIELDS] = {p.rows, p.path, p.loss, p.loss_finish, p.wgrad, p.streams, p.tail_on_caller, p.bias_finish,
                                                    p.norm, p.update};
    for (int i = 0; i < CODAE_STEP_PLAN_FIELDS; ++i) out[i] = fields[i];
    return CODAE_OK;
}

}  // extern "C"
