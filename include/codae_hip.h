/*
 * codae_hip.h — C ABI of libcodae_hip.so: the MI355X (gfx950) implementation of
 * CODAE's denoising-autoencoder training hot path.
 *
 * The reference (victordeleau/MUI-DeepAutoEncoder) is pure Python on PyTorch and
 * has no FFI of its own; the boundary this library sits behind is the Python
 * class surface of `codae.model` / `codae.tool` as used by
 * script/train_dae_on_embedding.py and script/train_dae_on_abalone.py
 * (SURVEY.md section 8b).  Each entry point below names the reference lines it
 * replaces.  The host-side mirror (mui-deepautoencoder_amd/codae, ctypes) is the
 * only caller; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - plain C, no torch types: device pointers + sizes; `stream` is a hipStream_t
 *     passed as void* (torch.cuda.current_stream().cuda_stream).
 *   - every function returns 0 on success or a negative CODAE_E_* code and never
 *     throws; codae_last_error() returns a thread-local message.
 *   - no function synchronises the device or allocates device memory: all
 *     buffers (parameters, gradients, Adam state, bf16 shadows, activation
 *     workspace, scalars) are caller-allocated and borrowed for the call.
 *   - a handle is used by one host thread at a time (one process per GPU).
 *   - all matrices are row-major; Linear weights are W[out][in] fp32 as in
 *     torch.nn.Linear (embedding_denoising_autoencoder.py:63).
 */
#ifndef CODAE_HIP_H
#define CODAE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped on EVERY change of a struct layout, an enum value or a function signature below.
 *   1: round 1 as first published (9-field codae_buffers)
 *   2: codae_buffers.shadow_wt, CODAE_S_ADAM_STEP / CODAE_S_COUNT 80, codae_struct_sizes, codae_reload_env,
 *      codae_train_step_graph, codae_step_backward_async, codae_side_stream, codae_join, codae_profile_stride
 *   3: codae_buffers.bias_parts, codae_sizes.bias_part_bytes, CODAE_K_CHAIN / CODAE_K_BIAS_FINISH, codae_span_sumsq,
 *      codae_step_update_span, codae_sync_transposed, codae_dgrad_bf16's partial-sum workspace
 *   4: + codae_ranking_loss_batched, codae_gather_inventory_rows, codae_step_path (new entries only; no layout change)
 *   5: + codae_monitor_accumulate; codae_ranking_loss_batched takes val_group (rows of the validation inventory that are
 *      exact duplicates of each other) behind val_pos; + codae_dp_unique_id / _init / _destroy, codae_train_step_dp
 *   6: codae_spec.act_kind / act_param (appended), CODAE_ACT_*, codae_linear_act_f32 / _bf16, codae_dgrad_act_f32 / _bf16
 *   7: + codae_topk_init / _merge / _finish, codae_complete_topk (new entries only; no layout change)
 *   8: + CODAE_NOISE_*, codae_noise, codae_set_input_noise, codae_corrupt_batch, codae_noise_box_muller (new entries only; no
 *      layout change of an existing struct, codae_struct_sizes keeps its seven entries)
 *   9: + codae_debug_gemm_bf16_plan, CODAE_GEMM_PLAN_FIELDS (new entry only; no layout change)
 *  10: + codae_emphasis, codae_set_loss_emphasis, codae_emph_loss, codae_emph_loss_blocks (new entries only; no layout change
 *      of an existing struct; codae_sizes.bias_part_bytes grows by a third column of per-block loss sums)
 *  11: + codae_dropout, codae_set_hidden_dropout, codae_dropout_fwd, codae_dropout_bwd, codae_dropout_blocks, CODAE_K_DROPOUT /
 *      CODAE_K_COUNT 11 (new entries only; no layout change of an existing struct)
 *      (still 11) + CODAE_LOSS_*, CODAE_COS_EPS, codae_recon_loss, codae_set_recon_loss, codae_recon_loss_fwd_bwd,
 *      codae_recon_loss_blocks: new entries only, no layout or enum change, the new kernels are booked under CODAE_K_LOSS
 *      (still 11) + codae_slot_contrast, codae_set_slot_contrast, codae_slot_contrast_ws_bytes, codae_slot_contrast_prepare,
 *      codae_slot_contrast_fwd_bwd, codae_slot_contrast_blocks: new entries only, no layout or enum change, booked under CODAE_K_LOSS
 *      (still 11) + CODAE_OPT_*, CODAE_SCHED_*, codae_optimizer, codae_set_optimizer, codae_optimizer_update, codae_graph_captures:
 *      new entries only, no layout or enum change, every variant of the update is booked under CODAE_K_ADAM
 *      (still 11) + codae_set_slot_presence, codae_corrupt_batch_present, codae_mse_loss_present, codae_emph_loss_present,
 *      codae_recon_loss_fwd_bwd_present, codae_slot_contrast_prepare_present, codae_slot_contrast_fwd_bwd_present: new entries only, no
 *      layout or enum change, no new kernel class
 *      (still 11) + codae_tie_pair, codae_set_tied_weights, codae_tie_fold, codae_tie_mirror: new entries only, no layout or enum
 *      change; the fold is booked under CODAE_K_SUMSQ (it forms the vector the norm is taken of), the mirror under CODAE_K_ADAM
 *      (still 11) + codae_set_dataset_image, codae_corrupt_batch_image: new entries only, no layout or enum change; the image gather is
 *      booked under CODAE_K_GATHER
 *      (still 11) + CODAE_AVG_*, codae_weight_average, codae_set_weight_average, codae_weight_average_update: new entries only, no
 *      layout or enum change; the average rides in the update's launch (CODAE_K_ADAM)
 *      (still 11) + CODAE_RM_*, codae_retrieval_metrics_batched: a new entry with plain arguments only, no struct, no layout or enum
 *      change
 *      (still 11) - the copy-out of the stamped GEMM build's timeline: an entry with no caller outside tools/ was removed; no
 *      layout or enum change
 *      (still 11) + codae_debug_gemm_bf16: a new entry with plain arguments only, no layout or enum change
 *      (still 11) + codae_debug_step_plan, CODAE_STEP_PLAN_FIELDS: a new host-only entry with plain arguments, no layout or enum change
 *      (still 11) + CODAE_AUC_*, codae_assemble_outfits, codae_outfit_scores, codae_auc_blocks, codae_auc_counts, codae_score_outfits:
 *      new entries with plain arguments only, no struct, no layout or enum change; the assemble is booked under CODAE_K_GATHER
 *      (still 11) + CODAE_NOISE_SWAP, codae_swap, codae_set_swap_pool, codae_corrupt_batch_swap, codae_emph_loss_swap,
 *      codae_recon_loss_fwd_bwd_swap: a new noise kind and new entries only, codae_noise keeps its layout, no existing enum value
 *      changes; the swap gathers are booked under CODAE_K_GATHER
 *      (still 11) + codae_residual, codae_residual_ws_bytes, codae_set_residual, codae_residual_fwd, codae_residual_bwd,
 *      codae_residual_blocks: new entries only, no layout or enum change; the two kernels are booked under CODAE_K_DROPOUT, the
 *      class of the streaming kernels between a step's GEMMs
 *      (still 11) + codae_norm, CODAE_NORM_*, codae_norm_ws_bytes, codae_set_norm, codae_norm_fwd, codae_norm_bwd, codae_norm_blocks:
 *      new entries only, no layout or existing enum change; the two kernels are booked under CODAE_K_DROPOUT as well
 *      (still 11) + codae_export_rows, codae_encode, codae_decode: new entries with plain arguments only, no struct, no layout or enum
 *      change; the export kernel is booked under CODAE_K_DROPOUT as well
 *      (still 11) + codae_nearest_centroid, codae_nearest_centroid_ws_bytes, codae_centroid_update, codae_centroid_update_ws_bytes: new
 *      entries with plain arguments only, no struct, no layout or enum change, no profiling kind
 *      (still 11) + codae_sparse_code, codae_sparse_code_ws_bytes, codae_set_sparse_code, codae_sparse_code_fwd, codae_sparse_code_bwd,
 *      codae_sparse_code_blocks: new entries only, no layout or enum change; the two kernels are booked under CODAE_K_DROPOUT as well
 *      (still 11) + CODAE_OPT_LAMB, CODAE_OPT_LARS, codae_trust_ws_bytes, codae_trust_ws_bytes_flat, codae_trust_update; codae_optimizer grows at its END by
 *      trust_clip, trust_coef, decay_bias, trust_ws (48 -> 72 bytes; the struct is not in codae_struct_sizes, a caller that fills the
 *      old fields and zeroes the rest gets what it got): no existing enum value or field moves; the norms pass and the finish are
 *      booked under CODAE_K_ADAM
 *      (still 11) + CODAE_VAR_*, codae_variable_loss, codae_set_variable_loss, codae_variable_loss_ws_bytes, codae_variable_loss_blocks,
 *      codae_variable_loss_fwd_bwd, codae_step_stores_output: new entries only, no layout or enum change; the three kernels are
 *      booked under CODAE_K_LOSS
 * The binding must refuse a library whose codae_abi_version() differs and must check its own struct sizes against
 * codae_struct_sizes() at load (mui-deepautoencoder_amd/codae/hip/__init__.py does both). */
#define CODAE_ABI_VERSION 11

enum {
    CODAE_OK = 0,
    CODAE_E_INVALID = -1,   /* bad argument / shape the kernels cannot take */
    CODAE_E_HIP = -2,       /* a HIP runtime call or launch failed */
    CODAE_E_UNSUPPORTED = -3
};

/* arithmetic of the GEMM chain */
enum {
    CODAE_PREC_F32 = 0,  /* parity mode: fp32 operands and fp32 accumulation; products formed from three bf16 planes per operand
                          * (gemm_f32x3.hip: six v_mfma_f32_16x16x32_bf16 per fp32 product, closer to float64 than an fp32 fma chain)
                          * wherever rows are 16-byte aligned and K is in whole 32-deep tiles, v_mfma_f32_32x32x2_f32 elsewhere and
                          * everywhere under CODAE_F32_GEMM=native */
    CODAE_PREC_BF16 = 1  /* throughput mode: bf16 operands, fp32 accumulate, v_mfma_f32_16x16x32_bf16; every layer width a
                          * multiple of 8 (16-byte rows; the activation buffers pad their rows to multiples of 64 themselves);
                          * codae_create returns CODAE_E_UNSUPPORTED otherwise (the caller falls back to CODAE_PREC_F32) */
};

/* activation after a Linear (the `activation` factory of the reference constructors, called as activation(True)).  Each is
 * monotone, so the backward takes its derivative from the saved OUTPUT y - what torch's in-place backward of these modules
 * does.  Parameters p[3] per layer:
 *   NONE         identity                                               -
 *   RELU         max(v, 0)                                               -
 *   LEAKY        v > 0 ? v : s v                     dy/dv = y > 0 ? 1 : s             p = {s >= 0}
 *   RELU6        min(max(v, 0), 6)                   dy/dv = 0 < y < 6                 -
 *   ELU          v > 0 ? l v : l a (exp(v / b) - 1)  dy/dv = y > 0 ? l : (y + l a) / b  p = {l > 0, a > 0, 1 / b > 0}
 *                (torch.nn.ELU: l = 1, b = 1; CELU: l = 1, b = a; SELU: torch's l and a, b = 1)
 *   SOFTPLUS     b v > t ? v : log1p(exp(b v)) / b   dy/dv = b y > t ? 1 : -expm1(-b y) p = {b > 0, t}
 *   HARDSIGMOID  clamp(v / 6 + 1/2, 0, 1)            dy/dv = 0 < y < 1 ? 1/6 : 0       - */
/* Non-finite values.  The kernels follow torch, so that a diverged run looks diverged (tests/test_gpu_nonfinite.py):
 *   1. every forward epilogue computes act(v) as torch.nn's module does for a non-finite v: NaN stays NaN for every CODAE_ACT_*
 *      and for the identity (ReLU is an IEEE 754-2019 maximum, not a max that drops the NaN operand); +-Inf maps as the module
 *      maps it (ReLU: +Inf, 0; ReLU6: 6, 0; ELU: +Inf, -l a; Softplus: +Inf, 0; Hardsigmoid: 1, 0).  The backward of ReLU, ReLU6 and
 *      Hardsigmoid SELECTS (0 under a dead unit whatever the incoming gradient), every other kind multiplies, as torch's do.
 *   2. GEMM arithmetic propagates as IEEE does: an output is NaN, +Inf or -Inf exactly where the float64 product of the same
 *      operands is, and a non-finite operand touches only the outputs that depend on it (ragged tiles, clamped loads, column-sum
 *      partials and split-K slabs included).
 *   3. a NaN total gradient norm gives a NaN clip coefficient - every parameter, both Adam moments and the bf16 shadows are NaN
 *      after the update, as after clip_grad_norm_ + Adam.step; a total of +Inf gives coefficient 0 (torch.clamp(max=1), not fminf).
 *   4. a training or evaluation step whose reference loss is non-finite reports a non-finite CODAE_S_LAST_LOSS and non-finite
 *      epoch sums, never a finite one.
 *   5. the one exception: the bf16-plane fp32 GEMM (CODAE_PREC_F32 above, gemm_f32x3.hip) turns an Inf ELEMENT of an operand
 *      into NaN at the outputs that depend on it - the residual planes of an Inf are Inf - Inf.  Never a finite value, and not
 *      for an Inf bias, which is added in fp32.  CODAE_F32_GEMM=native has no exception. */
enum {
    CODAE_ACT_NONE = 0,
    CODAE_ACT_RELU = 1,
    CODAE_ACT_LEAKY = 2,
    CODAE_ACT_RELU6 = 3,
    CODAE_ACT_ELU = 4,
    CODAE_ACT_SOFTPLUS = 5,
    CODAE_ACT_HARDSIGMOID = 6
};

/* Input noise of the denoising autoencoder (Vincent et al. 2010), applied to the TRAINING input by the gather of the fused step,
 * before the whole-slot mask (a blanked element is exactly 0 whatever the noise); the loss target stays the clean row.
 * Random words: Philox4x32-10 (Salmon et al. 2011; multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9, 0xBB67AE85),
 *   key = (seed & 0xffffffff, seed >> 32), counter = (g, row, step, 0), g = column / 4, row = the DATASET row (row_idx[b], or
 *   b when row_idx is NULL - never the position in the batch), step = the 1-based Adam step index; the four output words
 *   r[0..3] belong to columns 4g .. 4g + 3 (a last group that sticks out past io uses its leading words only).
 * x = the gathered fp32 value, r = its word, T = floor(p 2^32) (formed in double, compared as a 64-bit integer):
 *   MASKING      x <- 0 iff r < T (no rescaling)                                    p0 = p in [0, 1]
 *   SALT_PEPPER  r < T: x <- r < T / 2 ? lo : hi                                    p0 = p in [0, 1], p1 = lo, p2 = hi
 *   GAUSSIAN     x <- x + sigma n; the words of a group in pairs (r0, r1), (r2, r3): u1 = ((ra >> 8) + 1) 2^-24,
 *                u2 = (rb >> 8) 2^-24, rho = sqrt(-2 ln u1), n_a = rho cos(2 pi u2), n_b = rho sin(2 pi u2)
 *                                                                                   p0 = sigma >= 0
 * The same dataset row gets the same noise wherever it sits in a batch and on whichever data-parallel rank (a row that
 * appears twice in one batch gets the same noise twice; the epoch sampler draws without replacement).
 *
 * Swap noise (CODAE_NOISE_SWAP): with probability p a whole SLOT of the training input is replaced by the same slot of another
 * dataset row - the corruption of denoising autoencoders on categorical and entity data, and the training-side counterpart of the
 * swapped negatives of "Assembled outfits and compatibility".  p0 = p in [0, 1]; a codae_swap carries the slot count S (io = S E)
 * and an optional pool: a device int32 [P] of dataset rows that items may be taken from, 1 <= P < 2^31, every entry a valid row,
 * borrowed until replaced; pool NULL = every row of the dataset: P = n_pool = n_rows, pool[j] = j.  (A training script passes its
 * training rows, so that no validation item ever reaches a training input.)  For dataset row r (row_idx[b], or noise_rows[b] for a
 * batch gathered by the caller - never the position in the batch), slot s and the 1-based step t:
 *   words     (w0, w1, w2, w3) = Philox4x32-10(key = (seed & 0xffffffff, seed >> 32), counter = (s, r, t, 512)); counter word
 *             3 = 512 keeps the stream apart from the element noises (0), dropout (1 + layer) and the slot contrast (256);
 *             w2 and w3 are unused
 *   hit       w0 < T, T = floor(p 2^32) formed in double and compared as 64-bit - the rule of the kinds above
 *   source    j = ((uint64) w1 * P) >> 32, q = pool[j]
 *   accepted  hit && q != r, and with a presence table additionally present[r][s] && present[q][s].  No redraw and no loop: a
 *             rejected draw leaves the slot as it is; an absent slot is never noised
 *   input     every column of slot s of the batch row is data[q][sE .. (s+1)E) instead of data[r][..]; behind that the slot
 *             blank (a blanked element stays exactly 0), behind that the presence rule.  No arithmetic is done on the values,
 *             so a bf16 step may gather a swapped row from the dataset's bf16 image (codae_set_dataset_image): same bits
 *   target    the loss target and the monitors stay the clean row r; evaluation, completion and scoring never swap
 *   replaced  for "Loss emphasis": replaced(b, c) = accepted(r, c / E, t), recomputed from the words, the pool and the presence
 *             table - nothing is read back from the input; an accepted swap counts even when q holds the same bytes
 * The definition depends on (seed, pool, step, presence) alone: one process and N data-parallel ranks build the same inputs.
 * Not covered: swap combined with an element noise (one kind at a time), the mixed-variable path, redrawing after a rejection, the
 * persistent chain kernel (as for every noise kind). */
enum {
    CODAE_NOISE_NONE = 0,
    CODAE_NOISE_GAUSSIAN = 1,
    CODAE_NOISE_MASKING = 2,
    CODAE_NOISE_SALT_PEPPER = 3,
    CODAE_NOISE_SWAP = 4
};

typedef struct {
    int32_t kind;       /* CODAE_NOISE_* */
    float p0, p1, p2;   /* sigma or p; lo, hi (SALT_PEPPER) */
    uint64_t seed;
} codae_noise;

/* what CODAE_NOISE_SWAP needs beside codae_noise, whose layout stays: the graph key compares its bytes */
typedef struct {
    const int32_t* pool;   /* device [n_pool] dataset rows, or NULL = rows 0 .. n_pool - 1; borrowed */
    int32_t n_pool;        /* P >= 1; with pool NULL: the dataset's row count */
    int32_t n_slots;       /* S >= 1, dividing io */
} codae_swap;

/* Emphasised denoising loss (Vincent et al. 2010, section 4.3): the TRAINING loss weights corrupted and untouched elements
 * differently.  For batch row b (dataset row r = row_idx[b], or b when row_idx is NULL) and column c:
 *   blank(b,c)     the row has a mask id (mask_id or mask_to_use) and mask_table[id_b][c] == 0
 *   replaced(b,c)  the engine's input noise is MASKING or SALT_PEPPER and the element's Philox word satisfies r < T - word,
 *                  counter and T exactly as under "Input noise" above, with this step's index; GAUSSIAN replaces nothing;
 *                  SWAP: the element's slot took an accepted swap ("Swap noise")
 *   corrupted      blank or replaced
 *   w(b,c)         col_weight[c] * (corrupted ? alpha : beta), col_weight == 1 when absent; formed in fp32
 *   L              sum w (x - y)^2 * inv_n, inv_n = 1 / (rows * io) with rows = hyper->loss_scale_rows (the GLOBAL batch), or
 *                  batch->B when that is 0: no renormalisation by the weights
 *   dL/dy          2 w (y - x) inv_n
 * CODAE_S_LAST_LOSS is L.  The metric sums CODAE_S_SQ_FULL / CODAE_S_SQ_PARTIAL stay UNWEIGHTED, so monitors are comparable
 * across runs with different emphasis.  The target is the clean row.  Evaluation (codae_eval_step, hyper == NULL) is never
 * weighted.  Weights multiply: a NaN difference under weight 0 gives NaN in dy and in L, as (w * (x - y) ** 2).sum() does in
 * torch.  w depends on (dataset row, column, step, seed) only, so data-parallel ranks weight their shards as one process
 * weights the global batch. */
typedef struct {
    float alpha, beta;        /* weight of a corrupted / an untouched element; finite, >= 0 */
    const float* col_weight;  /* device, [io] or NULL; borrowed until the setting is replaced */
} codae_emphasis;

/* Slot presence: rows that lack an item in some slot take part in training, evaluation and completion.
 * A presence table is present[n_rows][S] of uint8, device resident; present[r][s] == 0 says that DATASET row r has no item in slot
 * s.  S = the slot count, io = S E, 1 <= S <= 128.  The table is keyed by the dataset row - row_idx[b], or b when row_idx is NULL -,
 * never by the position in the batch.  The rule is SELECTION, not multiplication: what `data` holds in an absent slot is never used
 * and may be NaN (compare "Loss emphasis", where weights multiply and a NaN under weight 0 stays a NaN).
 *   1. input      the gather writes exactly 0 into every column of an absent slot, in training and in evaluation, behind the input
 *                 noise and the slot blank: an absent element is never noised, and it never counts as corrupted or replaced.
 *   2. element-wise loss (MSE, emphasised MSE, L1, SMOOTH_L1, HUBER, the MSE anchor of SLOT_COSINE): an absent element's term is 0
 *                 and its dL/dy is exactly +0, whatever x and y hold; present elements keep their formulas, rounding order and
 *                 weights.  inv_n = 1 / (rows io) does not change: nothing renormalises by the number of present elements.
 *   3. SLOT_COSINE an absent pair (b, s) contributes 0 to L and 0 to dy - not the term W of a zero PRESENT target; W(b,s) of a
 *                 present pair is unchanged.
 *   4. slot contrast  an absent pair is a pair without a positive: 0 to loss and gradient (a NaN or Inf in its y slot still makes
 *                 the pair's dy and L NaN, as for any pair without a positive).  A candidate row_k whose slot s is absent is left out
 *                 of every pair, next to the accidental hits, and its vector reaches the products as zeros.  Drawing is unchanged
 *                 (same Philox stream, same j): the candidates of a step do not depend on the table.  Item ids are >= 0.
 *   5. monitors   CODAE_S_SQ_FULL sums (x-y)^2 over present elements, CODAE_S_SQ_PARTIAL over present and blanked ones, in training
 *                 and in codae_eval_step; CODAE_S_LAST_LOSS is L as defined here.
 *   6. everything else - dropout, clip, optimizer, schedule, shadows - is untouched.  Absence depends on the dataset row only, so a
 *                 data-parallel shard's dy rows are the bits of the same rows of the global batch, and a replayed graph has the bits
 *                 of a plain step.
 * While a table is set the training loss runs in the stand-alone kernels (the emphasised kernel with unit weights for the plain
 * MSE, the criterion's kernels otherwise), never in the last GEMM's epilogue, and the stack stays off the persistent chain kernel.
 * Not covered: renormalising by present counts, the ranking monitor on incomplete rows, the mixed-variable path, and
 * codae_forward / codae_backward on dense x (the binding has torch helpers for those loops). */

/* Training criterion: what the TRAINING loss measures between the clean row x and the output y; the default is the mean squared
 * error the reference script hard-wires.  d = x - y, rows = the global batch (hyper->loss_scale_rows, or batch->B when that is 0),
 * io = S E, inv_n = 1 / (rows io), w(b,c) = the emphasis weight defined above (1 everywhere when emphasis is off).
 * Element-wise kinds: L = sum w rho(d) inv_n, dL/dy = -w rho'(d) inv_n
 *   MSE        rho = d^2 (no factor 1/2)                                   rho' = 2 d                      -
 *   L1         rho = |d|                                                   rho' = sign(d), sign(0) = 0     -
 *   SMOOTH_L1  rho = |d| < beta ? d^2 / (2 beta) : |d| - beta / 2          rho' = d / beta or sign(d)      param = beta > 0
 *   HUBER      rho = |d| <= delta ? d^2 / 2 : delta (|d| - delta / 2)      rho' = d or delta sign(d)       param = delta > 0
 * (torch's l1_loss, smooth_l1_loss(beta=) and huber_loss(delta=) with reduction="none", weighted and summed.)
 * SLOT_COSINE, n_slots = S dividing io; for row b and slot s over its E columns:
 *   dot = sum x y, nx = max(|x|, eps), ny = max(|y|, eps), eps = CODAE_COS_EPS, cos = dot / (nx ny)
 *   W(b,s)  = (1 / E) sum_{c in s} w(b,c)
 *   L       = sum_{b,s} W (1 - cos) / (rows S)  +  mse_weight sum w d^2 inv_n
 *   dL/dy_c = -W / (rows S) (x_c / (nx ny) - [|y| > eps] cos y_c / |y|^2)  +  mse_weight 2 w (y_c - x_c) inv_n
 *   (torch's cosine_similarity(dim=-1, eps=1e-8) and its autograd.)  A zero target slot: cos = 0, term W, gradient 0.
 *   mse_weight >= 0 keeps the lengths anchored, which the cosine ignores.
 * CODAE_S_LAST_LOSS is L; CODAE_S_SQ_FULL / CODAE_S_SQ_PARTIAL stay the unweighted squared-error sums whatever the criterion;
 * evaluation never sees it.  Weights multiply and NaN propagates: a NaN in a slot of y makes that slot's dy and L NaN, under
 * weight 0 too.  The order in which a pair's E products are added depends on E alone, so a data-parallel shard's dy rows are
 * the bits of the same rows of the global batch. */
enum {
    CODAE_LOSS_MSE = 0,
    CODAE_LOSS_L1 = 1,
    CODAE_LOSS_SMOOTH_L1 = 2,
    CODAE_LOSS_HUBER = 3,
    CODAE_LOSS_SLOT_COSINE = 4
};
#define CODAE_COS_EPS 1e-8f

typedef struct {
    int32_t kind;       /* CODAE_LOSS_* */
    float param;        /* beta (SMOOTH_L1) or delta (HUBER): finite, > 0; ignored by the other kinds */
    float mse_weight;   /* SLOT_COSINE only: finite, >= 0; must be 0 for every other kind */
    int32_t n_slots;    /* SLOT_COSINE only: 1 <= n_slots <= 128, dividing io */
} codae_recon_loss;

/* Mixed-variable criterion: the TRAINING loss of a row made of variables (tabular data: one-hot and numeric columns), the
 * reference's CombinedCriterion(reduction="mean").  The row is described by n_var entries (position, size, type, weight): disjoint,
 * in ascending position, covering [0, io).  x = the clean row, y = the output, B = batch->B:
 *   L = (1 / n_var) sum_v w_v L_v
 *   REGRESSION      L_v = sqrt(sum_{b,k} (x - y)^2 / (B s_v)),          dL/dy = (w_v / n_var) (y - x) / (B s_v L_v)
 *   CLASSIFICATION  L_v = -(1 / B) sum_b log_softmax(y_slice)[t_b],     dL/dy = (w_v / n_var) (softmax(y_slice) - onehot(t_b)) / B
 *                   t_b = the FIRST maximum of the clean x slice
 * A regression variable reconstructed exactly (L_v = 0) gets 0 * inf = NaN in every one of its columns, as torch's autograd of
 * sqrt(mse_loss) gives; NaN and Inf in y propagate as in torch (a NaN in a one-hot slice makes the slice's dy and L NaN).
 * CODAE_S_LAST_LOSS is L; CODAE_S_SQ_FULL / CODAE_S_SQ_PARTIAL stay the unweighted sums of (x - y)^2 over ALL columns, one-hot
 * columns included, so they compare with those of a mean-squared-error run; evaluation never sees the criterion.
 * Three launches behind the last forward GEMM - per-(32-row block, variable) partial sums in double, one workgroup that adds every
 * variable's blocks in index order and forms L_v and the coefficient of its dy, then dy and the last bias gradient's partial rows -
 * with no float or double atomics: the same inputs give the same bits.  Every coefficient is formed on the device.
 * Limits: 1 <= n_var <= CODAE_VAR_MAX; 1 <= size (a thread walks a variable's columns of one row: any size runs, wide one-hots run
 * slowly); weights finite and >= 0.  position / size / type / weight are HOST arrays the setter reads; ws is DEVICE memory of at
 * least codae_variable_loss_ws_bytes(n_var, max batch) bytes, 16-byte aligned, borrowed until the setting is replaced: the table's
 * device image, the coefficients and the partial sums. */
enum {
    CODAE_VAR_REGRESSION = 0,
    CODAE_VAR_CLASSIFICATION = 1
};
#define CODAE_VAR_MAX 65536

typedef struct {
    int32_t n_var;
    int32_t reserved;          /* 0 */
    const int32_t* position;   /* [n_var] host: first column of the variable */
    const int32_t* size;       /* [n_var] host: its columns, >= 1 */
    const int32_t* type;       /* [n_var] host: CODAE_VAR_* */
    const float* weight;       /* [n_var] host: w_v, finite, >= 0 */
    void* ws;                  /* device work space */
    int64_t ws_bytes;
} codae_variable_loss;

/* Slot contrast: a sampled softmax (InfoNCE) over the true item of a slot and K negatives sampled from the same inventory, an
 * ADDITIONAL term of the TRAINING loss on top of whichever criterion is set (MSE included).  The stack is judged on a ranking by
 * cosine; the criterion pulls a reconstruction towards its own item, this term pushes it away from the other items of the slot.
 * Per batch row b and slot s (E columns, io = S E): x = the clean target slot, y = the output slot, eps = CODAE_COS_EPS, rows = the
 * global batch exactly as the criterion defines it, W(b,s) = the mean emphasis weight over the slot's columns (slot_cosine's W; 1
 * without emphasis).  Hats are unit vectors, v^ = v / max(|v|, eps).
 * Candidates belong to step t and slot s and are shared by every row and every rank.  For k in 0 .. K - 1:
 *   r       word k % 4 of Philox4x32-10 (constants of "Input noise"), key = (seed & 0xffffffff, seed >> 32), counter =
 *           (k / 4, s, t, 256): the fourth word keeps the stream apart from input noise (0) and dropout (1 + layer <= 255)
 *   j       ((uint64) r * P) >> 32, P = n_pool, or n_rows when pool is NULL;  row_k = pool ? pool[j] : j
 *   c_k     slot s of data[row_k], the clean dataset row - never noised, never masked.  Drawing is with replacement: a candidate
 *           drawn twice counts twice.  t = the 1-based Adam step (read from scalars[CODAE_S_ADAM_STEP] under graph replay)
 * Accidental hits: candidate k is left out for pair (b, s) iff item_id[s][row_k] == item_id[s][row_b] (item_id NULL: iff
 *   row_k == row_b), row_b = the dataset row of batch row b (row_idx[b], or b when row_idx is NULL).
 * Loss of a pair:
 *   z_0 = (x^ . y^) / tau,  z_k = (c_k^ . y^) / tau over the kept k
 *   l   = logsumexp(z_0, z_kept) - z_0,  p_j = softmax(z_0, z_kept)
 *   g   = sum_kept p_k c_k^ - (1 - p_0) x^
 *   dl/dy = [|y| > eps] (g - (g . y^) y^) / (tau |y|)
 *   a target slot with |x| <= eps has no positive: the pair contributes 0 to the loss and to the gradient; a pair whose candidates
 *   are all left out has l = 0 and a zero gradient by the formulas themselves.
 * Total: L = L_criterion + weight sum_{b,s} W l / (rows S); dL/dy is the sum of the two gradients; CODAE_S_LAST_LOSS is the total;
 *   CODAE_S_SQ_FULL / CODAE_S_SQ_PARTIAL stay the unweighted squared-error sums; evaluation never sees the term.
 * NaN: a NaN or Inf anywhere in a y slot makes that pair's dy and L NaN, under weight W = 0 and for a zero target too; no other pair
 *   is affected.  (A finite slot whose squares overflow fp32, |y| > 1.8e19, counts as Inf.)
 * Determinism: the order in which a pair's sums over E and over K are added depends on E and K alone - not on B, nor on the row's
 *   position in the batch or in a tile: a data-parallel shard's dy rows are the bits of the same rows of the global batch.
 * Operand precision follows the engine: bf16 unit vectors into v_mfma_f32_16x16x32_bf16 (the p_k rounded to bf16 for the weighted
 *   sum), or fp32 into v_mfma_f32_16x16x4_f32; fp32 accumulation and fp32 softmax either way; z_0 always in fp32. */
typedef struct {
    int32_t n_slots;         /* S: 1 <= n_slots <= 128, dividing io; E = io / S <= 1024 */
    int32_t n_neg;           /* K: 1 <= n_neg <= 4096 */
    float tau;               /* finite, >= 0.01 */
    float weight;            /* finite, >= 0; 0 = off */
    uint64_t seed;
    int32_t n_rows;          /* rows of batch->data */
    int32_t n_pool;          /* entries of pool; 0 (or n_rows) when pool is NULL */
    int64_t ws_bytes;        /* bytes behind ws: >= codae_slot_contrast_ws_bytes(S, K, E, bf16 engine) */
    const int32_t* pool;     /* device, [n_pool] rows of data to draw from, or NULL = every row */
    const int32_t* item_id;  /* device, [S][n_rows] item identity of every dataset row per slot, or NULL = the row itself */
    void* ws;                /* device, 16-byte aligned work space; all three borrowed until the setting is replaced */
} codae_slot_contrast;

/* Hidden dropout (Srivastava et al. 2014, inverted form as torch.nn.Dropout): the TRAINING step multiplies the output of layer l,
 * 0 <= l <= n_layers - 2 - what layer l + 1 reads and the engine keeps as act[l + 1] - by a random factor.  The last layer's
 * output is never dropped (the input has its own masking noise, above).  For batch row b and column c < out[l]:
 *   row     the DATASET row: row_idx[b], or b when row_idx is NULL
 *   r       Philox4x32-10 with the multipliers and Weyl constants of "Input noise", key = (seed & 0xffffffff, seed >> 32),
 *           counter = (c / 4, row, step, 1 + l); word c % 4 of the output belongs to column c (a last group that sticks out past
 *           the width uses its leading words only); step = the 1-based Adam step.  The fourth counter word keeps the stream apart
 *           from the input noise (word 0) and from the other layers, even under the same seed
 *   T       floor(p_l 2^32), formed in double and compared as a 64-bit integer; the element is DROPPED iff r < T
 *   f       0 when dropped, else s_l = (float)(1.0 / (1.0 - (double)p_l))
 *   forward   a <- a f: one fp32 multiplication (bf16 engine: the stored bf16 value widened, multiplied, rounded to nearest even)
 *   backward  the stored activation gradient of layer l: d <- d f, the same factor and rounding, applied after the data-gradient
 *             GEMM's epilogue has applied the activation derivative; the bias gradient of layer l is the column sum of the FINAL d
 *             over rows < B
 * The factor multiplies: a NaN under a dropped element stays NaN and an Inf becomes NaN, as torch.nn.functional.dropout does (in
 * line with points 1 - 4 of "Non-finite values").  One case differs from torch in non-finite arithmetic only: a ReLU layer whose
 * data gradient takes its mask from the saved (dropped) output instead of the 1-bit masks selects 0 under a dropped unit before
 * the factor is applied, so a non-finite incoming gradient there gives 0 where torch gives NaN.
 * Training steps only: codae_eval_step, codae_forward / codae_backward and a forward with hyper == NULL never drop.  The metric
 * sums and CODAE_S_LAST_LOSS are those of the dropped network's output; no separate clean forward is run.
 * The backward takes an activation's derivative from its saved output, which is y s after dropout, so p_l > 0 is accepted only
 * where the derivative does not depend on the output's magnitude: CODAE_ACT_NONE, RELU (1-bit masks or the saved output) and
 * LEAKY.  f depends on (seed, dataset row, column, step, layer) only, so data-parallel ranks drop their shards as one process
 * drops the global batch. */
typedef struct {
    const float* p;     /* HOST array [n], n == n_layers - 1; copied by the setter */
    int32_t n;
    uint64_t seed;
} codae_dropout;

/* Residual connections: an identity skip around a hidden layer of equal widths (He et al. 2016); no parameters, no projection.
 * Layers are l = 0 .. L-1, h_0 is the corrupted input, skip_l in {0, 1}:
 *   z_l = W_l h_l + b_l          a_l = act_l(z_l)   (times the dropout factor f_l when layer l is dropped)
 *   h_{l+1} = a_l + skip_l h_l                       loss on h_L
 * Backward, with G_l = dL/dh_l and D_l = dL/dz_l (what dA_l holds, read by the weight and the data gradient of layer l):
 *   U_l = W_l^T D_l                                  (the data-gradient GEMM of layer l, UNMASKED)
 *   G_l = U_l + skip_l G_{l+1}
 *   D_{l-1} = G_l * act'_{l-1} (* f_{l-1})           db_{l-1} = column sums of D_{l-1} over rows < B
 * skip_l = 1 is accepted only where in[l] == out[l], l <= L-2 and act_l is CODAE_ACT_NONE, RELU or LEAKY.  The last layer never
 * has a skip: its output is the reconstruction.  Other activations are excluded because the derivative is taken from the saved
 * output, and once h_l is added that output no longer determines it.
 * It is part of the MODEL: every forward adds the skips - the training steps, codae_eval_step, codae_forward over the whole stack,
 * codae_score_outfits, and whatever buffer set (the weight average's) the call is given.
 * Forward, behind the GEMM of a skipped layer l and behind its dropout kernel: act[l + 1] <- rne(float(act[l + 1]) + float(act[l]))
 * in place, one fp32 add, rounded to the working type.  A TRAINING forward first writes the 1-bit mask of a_l the backward needs
 * (act[l + 1] afterwards holds h_{l+1}, from which the sign of a_l cannot be recovered): one bit per element, 8 columns per byte,
 * column 8 j + k in bit k of byte j, set iff the stored a_l has its sign clear and is not zero - the predicate and the layout of the
 * forward GEMM's 1-bit ReLU masks, so a NaN with a clear sign counts as positive.  Layers with CODAE_ACT_NONE need no mask.
 * Backward, behind the data-gradient GEMM of layer l iff skip_l or skip_{l-1}: that GEMM runs unmasked and leaves U_l in dA_{l-1}
 * in working precision; the kernel reads G_{l+1} (iff skip_l), adds in fp32, stores G_l (iff skip_{l-1}), forms D_{l-1} = G_l where
 * the bit is set, else 0 (RELU) or G_l slope (LEAKY), stores it over U_l in working precision and leaves the column sums of the
 * STORED values as layer l-1's partial bias-gradient rows (fixed order, no atomics).  When skip_{l-1} = 0 the derivative of layer
 * l-1 comes from the saved activation act[l], as the GEMM epilogue takes it.  Dropout's backward kernel then scales D_{l-1} and
 * rewrites the rows.  G is kept in fp32 in one [rows][width] buffer of the work space, updated in place: it is a sum of up to
 * L-2 terms, and in the bf16 engine every U_l already arrives rounded once.  Every other data gradient runs masked as always. */
typedef struct {
    int32_t n;            /* == n_layers */
    const uint8_t* on;    /* HOST array [n]: on[l] != 0 = a skip around layer l; copied by the setter */
} codae_residual;

/* Normalisation: parameter-free layer / RMS normalisation (Ba et al. 2016; Zhang & Sennrich 2019) of a hidden layer's output, per
 * batch row, as the last thing the layer does (post-norm).  With f_l the dropout factor and skip_l the residual flag, norm_l in {0, 1}:
 *   a_l = f_l act_l(W_l h_l + b_l)      s_l = a_l + skip_l h_l      h_{l+1} = norm_l ? N(s_l) : s_l
 * N acts on one batch row x of width w = out[l], eps > 0:
 *   CODAE_NORM_LAYER  mu = sum x / w, v = sum (x - mu)^2 / w (biased, two passes), r = 1 / sqrt(v + eps), xhat = (x - mu) r
 *   CODAE_NORM_RMS    r = 1 / sqrt(sum x^2 / w + eps), xhat = x r
 * There is no gain and no bias: every normalised layer is followed by a Linear, which absorbs them (W diag(gamma), b + W beta), so
 * the parameter vector, the optimizer spans, tied weights, the average and the checkpoint tensors keep their shape.  The statistics
 * are per row: no value crosses rows or ranks, evaluation needs no running average, and a shard of a batch gives the bits of the
 * same rows of the whole batch.
 * Precision: the statistics are fp32, formed from the STORED working-precision s_l; a lane adds its columns in ascending order, the
 * 64 lanes' sums meet in a butterfly whose result is the same in every lane; no atomics.  xhat is rounded to nearest even into the
 * working type and stored IN PLACE in act[l + 1]; r stays fp32, one value per (normalised layer, batch row), in the work space.
 * Backward, Gh_{l+1} = dL/dh_{l+1} as the UNMASKED data-gradient GEMM of layer l + 1 leaves it (working precision) plus the skip
 * term skip_{l+1} G, all arithmetic fp32, xhat = the stored (rounded) activation:
 *   c1 = sum Gh / w (LAYER only)          c2 = sum (Gh xhat) / w
 *   Gs_l = r (Gh - c1 - xhat c2) (LAYER)  Gs_l = r (Gh - xhat c2) (RMS)       Gs_l = Gh (norm_l = 0)
 *   D_l = Gs_l act'_l (rounded once into the working type; then dropout's factor, in dropout's own kernel)
 *   Gh_l = D_l W_l + skip_l Gs_l          (the matrix G of "Residual connections" holds Gs)
 * act'_l comes from a 1-bit mask of the pre-norm value (layout and predicate of the residual masks): after normalising, the saved
 * output no longer determines it.  A skipped layer's mask is the residual kernel's; otherwise a TRAINING forward's norm kernel
 * writes it into the norm's work space before it normalises.
 * norm_l = 1 is accepted only for l <= L-2 (the last layer's output is the reconstruction) and only behind CODAE_ACT_NONE, RELU or
 * LEAKY; eps must be finite and > 0.  Unlike a skip it needs no equal widths: layer 0 and tapered stacks are allowed.
 * It is part of the MODEL: every forward normalises - the training steps, codae_eval_step, codae_forward over the whole stack,
 * codae_score_outfits, with whatever buffer set (the weight average's) the call is given.  Pad columns (ld > width) and pad rows are
 * never written: xhat of a zero pad column would be -mu r, and the next GEMM runs k over the padded width. */
enum { CODAE_NORM_LAYER = 1, CODAE_NORM_RMS = 2 };
typedef struct {
    int32_t n;            /* == n_layers */
    const uint8_t* on;    /* HOST array [n]: on[l] != 0 = layer l's output is normalised; copied by the setter */
    int32_t kind;         /* CODAE_NORM_LAYER or CODAE_NORM_RMS, one kind for the stack */
    float eps;
} codae_norm;

/* Sparse code: the k-sparse autoencoder's hard top-k code layer (Makhzani & Frey 2013; the "TopK" form of sparse-autoencoder work).
 * `layer` follows codae_encode's convention: it is the index of the Linear that READS the code, 1 <= layer <= L - 1; the Linear
 * that produces it is m = layer - 1, and Z = out[m].  Sparsifying is the last thing layer m does, after the activation and the
 * dropout factor.  For each batch row:
 *   key(v) = the bit pattern of the STORED value v with the sign bit cleared, read as an unsigned integer (the stored value is a
 *            bf16 number in the bf16 engine and fp32 in the fp32 engine; widening bf16 to fp32 keeps the order).  -0 and +0 have
 *            the same key, Inf sorts above every finite value, and every NaN sorts above Inf, ordered by payload.
 *   Columns are ranked by (key descending, column ascending).  The first `keep` columns are KEPT and their bits stay as stored;
 *   every other column is stored as +0.  Because NaN ranks first, a NaN is always kept, so a NaN row still makes its outputs and
 *   the loss NaN.
 * Backward is selection, not multiplication: dA_m[b][j] is unchanged where column j was kept and exactly +0 elsewhere, even under
 * a NaN gradient; the bias-gradient partial column sums of layer m are rewritten from those final values.
 * keep == Z is accepted and is OFF; keep < 1 and keep > Z are refused.
 * It is part of the MODEL, like the skips and the norm: every forward sparsifies - the training steps in every step form,
 * codae_eval_step, codae_forward over the whole stack, codae_score_outfits, codae_encode (whose codes then have at most `keep`
 * non-zeros per row) -, with whatever buffer set the call is given; codae_decode starts at Linear `layer` and takes the code as
 * given.  The selection is per row: a shard of a batch gives the bits of the same rows of the whole batch, and nothing is kept
 * between steps.
 * Limits: no skip and no norm on layer m itself (a skip would add the dense h_m back; a norm's backward needs the full xhat, which
 * the in-place store has overwritten) - skips and norms on every other layer are allowed, a skip around Linear `layer` included;
 * the activation of layer m is CODAE_ACT_NONE, RELU or LEAKY (the derivative the GEMM epilogue takes from the saved output is then
 * right wherever the value was kept, and what it takes under a dropped element is selected away); never the last layer.
 * Pad columns (ld > width) and pad rows are never written. */
typedef struct {
    int32_t layer;        /* the Linear that reads the code: 1 .. n_layers - 1 */
    int32_t keep;         /* units kept per row: 1 .. Z; Z = off */
} codae_sparse_code;

/* Optimizer and schedule: what the update at the end of every training step does with the clipped gradient; the default is the line
 * the reference script hard-wires, clip_grad_norm_ + torch.optim.Adam with L2 decay, AMSGrad off and a constant lr.
 * t = the 1-based step, coef = the clip coefficient ("Non-finite values", point 3), lr, wd, b1, b2, eps = the fields of codae_hyper.
 * Schedule, evaluated in double (W = warmup, T = total):
 *   w(t)  = W > 0 && t <= W ? t / W : 1
 *   q(t)  = clamp((t - W) / (T - W), 0, 1)
 *   f(t)  = w(t) * { CONSTANT: 1
 *                    COSINE:   min_factor + (1 - min_factor) (1 + cos(pi q)) / 2
 *                    LINEAR:   1 - (1 - min_factor) q
 *                    STEP:     gamma ^ floor((t - 1) / period) }
 *   lr_t  = (float)((double)lr * f(t))
 *   Past T the factor stays at its end value: torch's LambdaLR with lambda(t - 1).  The factor is computed on the device, in the
 *   update kernel's prologue, from t = hyper->step in a plain step and t = scalars[CODAE_S_ADAM_STEP] under graph replay - the same
 *   code, so a replayed step has the bits of a plain one and a schedule never re-captures the graph.
 * Updates, bc1 = 1 - b1^t, bc2 = 1 - b2^t:
 *   ADAM   g' = g coef + wd p;  m' = b1 m + (1-b1) g';  v' = b2 v + (1-b2) g'^2;  d = v'
 *   ADAMW  g' = g coef;         p1 = p (1 - lr_t wd);   m', v' as above from g';  d = v'     (torch.optim.AdamW)
 *          (p1 is evaluated as p - (lr_t wd) p: one rounding at the size of p)
 *     amsgrad: vmax' = max(vmax, v'), a NaN on either side staying NaN as in torch.maximum (not fmaxf);  d = vmax'
 *          p' = (p | p1) - lr_t / bc1 * m' / (sqrt(d) / sqrt(bc2) + eps)
 *   SGD    g' = g coef + wd p;  m' = mu m + g';  u = nesterov ? g' + mu m' : m';  p' = p - lr_t u;  v is neither read nor written
 *          (torch.optim.SGD with dampening 0; with a zero-initialised m its first step is torch's)
 * A NaN clip coefficient makes every parameter and every state tensor that is written NaN, as under the default.
 * Every kind writes p, the moments it keeps, the bf16 shadow and the transposed shadow in the one pass the default makes.
 *
 * Layer-wise trust ratios (LAMB: You et al. 2020; LARS: You et al. 2017).  A MATRIX is one weight matrix W_l of the flat parameter
 * vector (its offset, out[l] x in[l]; with tied weights the free ones); the BIAS BLOCK is [bias_begin, n_param).  Norms are per
 * matrix: P = sqrt(sum p^2), U = sqrt(sum u^2), G = sqrt(sum g'^2) over the matrix's elements; each square is formed in fp32 from
 * the fp32 value, widened, and added in double, in an order the matrix shape alone fixes (per 64 x 128 tile of the tiled update, per
 * 4096 consecutive elements of the flat one: 256 lanes in element order, an xor-butterfly per wave, the four waves in order; then the
 * partial pairs in index order) - not the grid, not the run, not plain versus replayed.  wd' = wd in a matrix, decay_bias ? wd : 0 in
 * the bias block; inv_bc1 = (float)(1 / bc1), inv_sqrt_bc2 = (float)(1 / sqrt(bc2)); every fp32 operation below is rounded on its
 * own (no fused multiply-add), in the order written:
 *   LAMB   g' = g coef;  m' = b1 m + (1-b1) g';  v' = b2 v + ((1-b2) g') g'
 *          u  = (m' / (sqrt(v') inv_sqrt_bc2 + eps)) inv_bc1 + wd' p
 *          matrix: phi = (P > 0 && U > 0) ? P / U : 1 in double;  if (trust_clip > 0) phi = min(phi, trust_clip);  phi32 = (float)phi
 *          bias block: phi32 = 1 (no adaptation)
 *          p' = p - (lr_t phi32) u
 *   LARS   g' = g coef
 *          matrix: lambda = (P > 0 && G > 0) ? trust_coef P / (G + wd P + eps) : 1 in double;  trust_clip as above;  lambda32 = (float)
 *          bias block: lambda32 = 1
 *          d = lambda32 (g' + wd' p);  m' = mu m + d;  u = nesterov ? d + mu m' : m';  p' = p - lr_t u;  v is neither read nor written
 * A comparison with a NaN norm is false: the ratio is 1 and the NaN elements of u decide.  The norms pass reads p, g, m, v and writes
 * no state; it forms u with the update's own prologue and per-element function.  The finish writes the fp32 ratio of matrix l to
 * ((float*)trust_ws)[l]: the ratios of the last update can be read there.  Both run in front of the update on its stream, inside a
 * captured graph too.  Tied weights: one ratio per free matrix, from the folded gradient.  Refused: amsgrad with either kind,
 * trust_clip < 0 or non-finite, trust_coef <= 0 or non-finite (LARS), a missing, misaligned or short trust_ws, more than 64
 * matrices: CODAE_E_INVALID; codae_step_update_span while either kind is set: CODAE_E_UNSUPPORTED (a matrix's norm spans shards).
 * Not covered: decay_bias for the other kinds, per-tensor adaptation of single bias vectors, the mixed-variable path. */
enum { CODAE_OPT_ADAM = 0, CODAE_OPT_ADAMW = 1, CODAE_OPT_SGD = 2, CODAE_OPT_LAMB = 3, CODAE_OPT_LARS = 4 };
#define CODAE_TRUST_MAX_MATRICES 64      /* the ratios at the head of trust_ws */
#define CODAE_TRUST_CHUNK 4096           /* elements per partial pair of the flat norms pass */
enum { CODAE_SCHED_CONSTANT = 0, CODAE_SCHED_COSINE = 1, CODAE_SCHED_LINEAR = 2, CODAE_SCHED_STEP = 3 };
typedef struct {
    int32_t kind;          /* CODAE_OPT_* */
    int32_t amsgrad;       /* ADAM / ADAMW only */
    float   momentum;      /* SGD: mu in [0, 1) */
    int32_t nesterov;      /* SGD, needs mu > 0 */
    int32_t sched;         /* CODAE_SCHED_* */
    int32_t warmup;        /* W >= 0 steps */
    int32_t total;         /* T > W for COSINE / LINEAR */
    int32_t period;        /* STEP: >= 1 */
    float   min_factor;    /* COSINE / LINEAR: in [0, 1] */
    float   gamma;         /* STEP: in (0, 1] */
    float*  vmax;          /* device [n_param] fp32, zero before first use (padding too); required iff amsgrad; borrowed */
    float   trust_clip;    /* LAMB / LARS: upper bound of the ratio, 0 = none */
    float   trust_coef;    /* LARS: > 0 */
    int32_t decay_bias;    /* LAMB / LARS: 0 or 1: weight decay in the bias block too */
    void*   trust_ws;      /* LAMB / LARS: device work space of codae_trust_ws_bytes(h) bytes, 16-byte aligned, zero before first use;
                            * 64 fp32 ratios, then the (sum p^2, sum u^2) double pairs of the norms pass; borrowed */
} codae_optimizer;

/* Tied weights (Vincent et al. 2010): the decoder's Linear l' = L-1-l uses the transpose of the encoder's Linear l.  With tying on
 * (codae_set_tied_weights) the FREE parameters are the weights of the layers l < L/2, the middle layer's weight when L is odd, and
 * every bias (biases stay untied).  The tie is MATERIALISED: for every pair (l, l') with l < l' the decoder matrix is kept in memory
 * as W_l' = W_l^T - in the fp32 parameter vector, in the bf16 shadow of l' (bf16 of the transpose), and in the transposed shadow of
 * l' (the bits of l's plain shadow) - so the forward, the data-gradient chain and the weight-gradient launches run unchanged (the
 * persistent chain kernel, the grouped weight-gradient launch and graph replay included) and every reader of the parameters sees
 * a whole decoder.  The backward still leaves a gradient for W_l and one for W_l'.  The tie lives between backward and update:
 *   1. fold    g[W_l][i][j] <- g[W_l][i][j] + g[W_l'][j][i] (one fp32 add, in that operand order), then g[W_l'] <- +0.  The flat
 *              gradient vector IS then the gradient of the tied parameter set.  Under data parallel it runs after the reduce.
 *   2. norm    the flat sum g^2 over that vector (every tied weight once, as clip_grad_norm_ counts a shared nn.Parameter; the bias
 *              block once); the per-matrix sums of the weight-gradient epilogues and slab reduces are not gathered.
 *   3. update  the optimizer of "Optimizer and schedule", every kind, on the free parameters only: weight decay acts once per
 *              tied weight; adam_m, adam_v and vmax of the decoder matrices are never read or written.
 *   4. mirror  W_l' <- W_l^T in fp32, the bf16 shadow of l' (the rounding of the cast: bf16 of the fp32 value) and the transposed
 *              shadow of l'.  codae_sync_shadows runs it too: the encoder is the truth, a decoder matrix found in params is overwritten.
 * Refused with CODAE_E_UNSUPPORTED, the message naming the pair: a stack where in_l != out_l' or out_l != in_l' for some pair; and
 * codae_step_update_span while tying is on (a tied pair straddles two shards of the sharded update). */
typedef struct {
    int64_t enc_off;       /* element offset of the encoder matrix W [rows][cols] in the flat vectors */
    int64_t dec_off;       /* element offset of the decoder matrix W' [cols][rows] = W^T */
    int32_t rows, cols;
} codae_tie_pair;

/* Weight average: an average of the iterates, kept beside the parameters by the update itself, for evaluation (Polyak & Juditsky
 * 1992; Izmailov et al. 2018, SWA; torch.optim.swa_utils.AveragedModel).  t = the 1-based step of this update (hyper->step in a plain
 * step, scalars[CODAE_S_ADAM_STEP] under graph replay), p' = the parameter the update has just produced, a = avg at that element.
 *   t < start or (t - start) % every != 0:  the step does not SAMPLE: avg is neither read nor written.
 *   otherwise n = (t - start) / every, the number of earlier samples, and, in double:
 *     SWA  w = 1 / (n + 1)                                        (the equal-weight mean of the samples)
 *     EMA  w = 1 when n == 0, else 1 - d_n,  d_n = debias ? min(decay, (1 + n) / (10 + n)) : decay
 *   w32 = (float)w;  a' = p' bit for bit when w32 == 1 (avg is not read), else a' = a + w32 (p' - a) in fp32 (the compiler may
 *   contract the product and the sum into one fma).  A NaN in p' becomes a NaN in a'.
 * The weight is computed in the update kernel's prologue from the same step count as the schedule, so a replayed step has the
 * bits of a plain one and a graph is never re-captured for a new w; a step that does not sample issues no access to avg.
 * avg has the layout of params; its padding stays zero (p' = 0 there).  Tied weights: only the free parameters are averaged - the
 * decoder ranges of avg are never written by the update; averaging is linear, so the decoder of the average is the mirror of the
 * averaged encoder, which codae_sync_shadows on a codae_buffers whose params point at avg materialises.
 * p, the moments and the shadows of a step are bit for bit those of the same step without averaging.
 * Not covered: the sharded update (codae_step_update_span refuses while averaging is on: a shard's average would have to be
 * all-gathered too), the mixed-variable path, averaging of optimizer moments, checkpoint files. */
enum { CODAE_AVG_OFF = 0, CODAE_AVG_EMA = 1, CODAE_AVG_SWA = 2 };
typedef struct {
    int32_t kind;          /* CODAE_AVG_* */
    float   decay;         /* EMA: in [0, 1) */
    int32_t debias;        /* EMA: 0 or 1 */
    int32_t start;         /* >= 1: the first averaged step */
    int32_t every;         /* >= 1 */
    float*  avg;           /* device [n_param] fp32 in the layout of params, padding zero, 16-byte aligned; borrowed */
} codae_weight_average;

typedef struct codae_engine* codae_handle;

/* Network description: the Linear stack built by
 * EmbeddingDenoisingAutoencoder.__init__ (embedding_denoising_autoencoder.py:49-129)
 * or MixedVariableDenoisingAutoencoder.__init__ (mixed_variable_...py:45-125). */
typedef struct {
    int32_t n_layers;
    const int32_t* in_features;  /* [n_layers] */
    const int32_t* out_features; /* [n_layers] */
    const uint8_t* relu;         /* [n_layers] 1 = ReLU follows this Linear */
    int32_t max_batch;           /* rows the workspaces are sized for */
    int32_t precision;           /* CODAE_PREC_* */
    /* ABI 6.  NULL: `relu` alone says what follows each Linear (ReLU or nothing).  Else act_kind[l] (CODAE_ACT_*) does and
     * `relu` is not read; act_param [n_layers][3] holds the parameters above (may be NULL when no layer needs any).  The
     * last layer takes NONE or RELU only.  Layers with another kind than RELU get no 1-bit masks and keep the stack off the
     * persistent chain kernel (codae_step_path).  codae_create returns CODAE_E_INVALID for an unknown kind or a parameter
     * out of range. */
    const uint8_t* act_kind;
    const float* act_param;
} codae_spec;

/* Byte sizes / element offsets the caller needs to allocate the borrowed buffers. */
typedef struct {
    int64_t n_param;        /* elements of the flat fp32 parameter vector (with padding) */
    int64_t n_weight;       /* elements of the flat bf16 weight shadow (BF16 mode, else 0) */
    int64_t act_bytes;      /* activation workspace */
    int64_t dact_bytes;     /* activation-gradient workspace: min(n_layers + 1, 16) buffers (at least 3), one per layer
                               so that the two backward streams never wait for each other; deeper stacks rotate */
    int64_t slab_bytes;     /* split-K partial slabs for the weight-gradient GEMM (BF16 mode) */
    int64_t bias_part_bytes; /* partial column sums of the bias gradients (codae_buffers.bias_parts) */
    int32_t n_scalars;      /* doubles in the scalar block (CODAE_S_*) */
} codae_sizes;

/* Borrowed device buffers.
 * Buffer contents.  The library allocates nothing and zeroes nothing at first use, so the caller hands the buffers over in this
 * state (tests/test_gpu_history.py poisons every byte that is NOT listed and compares the results bit for bit).
 * Before the first call these borrowed bytes must be ZERO:
 *   (1) params, grads, adam_m and adam_v outside the weight and bias tensors (the padding that rounds every tensor up to 64
 *       floats): the norm and Adam kernels sweep the whole flat vectors, and the padding stays zero under them (g = 0, p = 0);
 *   (2) all of scalars: the metric sums accumulate across calls until the caller zeroes them, the rest is scratch the step
 *       clears itself on its way;
 *   (3) only when a layer width is not a multiple of 64: all of acts and dacts (the pad columns between a row's width and its
 *       64-element stride are never written and are multiplied with whatever follows a weight row) and the 64 * maxw elements of
 *       shadow_w and shadow_wt behind n_param (the slack n_weight includes: a GEMM whose k extent is a padded width reads the
 *       weight operand up to 63 elements past the last matrix).
 * Everything else may hold anything: the weight and bias tensors inside params / adam_m / adam_v are the caller's to fill, the
 * first n_param elements of shadow_w and shadow_wt are written by codae_sync_shadows, and every call writes what it reads of
 * slabs, bias_parts, the weight and bias tensors inside grads, and - when every width is a multiple of 64 - acts, dacts and the
 * slack behind n_param in both shadows.  That holds between calls too: a call never depends on what an earlier call with another
 * batch size, another entry point or non-finite data left in a workspace (pad rows included); after a diverged step, reloading
 * params / adam_m / adam_v (padding included) and codae_sync_shadows is the whole recovery. */
typedef struct {
    float* params;      /* flat: per layer W[out*in] then b[out], each padded to 64 floats */
    float* grads;       /* same layout */
    float* adam_m;      /* same layout (exp_avg)    — may be NULL if codae_step_update is unused */
    float* adam_v;      /* same layout (exp_avg_sq) */
    void* shadow_w;     /* bf16 copy of the weights, per layer [out][in]; BF16 mode only */
    void* acts;         /* act_bytes */
    void* dacts;        /* dact_bytes */
    void* slabs;        /* slab_bytes */
    double* scalars;    /* n_scalars doubles, see CODAE_S_* */
    void* shadow_wt;    /* optional (BF16 mode): bf16 TRANSPOSED weights, per layer [in][out] at the same offsets as
                           shadow_w; when present the data-gradient GEMM reads it k-contiguously (forward-form
                           kernel) instead of reading W through transposed LDS reads; n_weight elements */
    float* bias_parts;  /* bias_part_bytes: every producer of an activation gradient leaves per-row-block partial column
                           sums here with plain stores; one small kernel per backward call adds them up in a fixed order
                           into grads' bias block (autograd's bias gradient, train_dae_on_embedding.py:210) - the step has
                           no float atomics, so the same inputs give the same bits on every run (ABI 3) */
} codae_buffers;

/* indices into codae_buffers.scalars (device memory, accumulated across calls until zeroed) */
enum {
    CODAE_S_SQ_FULL = 0,     /* sum (x-y)^2              (train_dae_on_embedding.py:218-220) */
    CODAE_S_SQ_PARTIAL = 1,  /* sum (1-fmask)(x-y)^2     (train_dae_on_embedding.py:223)     */
    CODAE_S_GRAD_SQ = 2,     /* sum g^2 of the last codae_step_update (pre-clip)             */
    CODAE_S_LAST_LOSS = 3,   /* mean MSE of the last step (train_dae_on_embedding.py:206)    */
    CODAE_S_STEP_SQ = 4,     /* scratch: sum (x-y)^2 of the current step                     */
    CODAE_S_CLIP_COEF = 5,   /* (5, 6) reserved                                                             */
    CODAE_S_GRAD_SQ_SLOTS = 8, /* 64 partial sums of g^2: same-address atomics serialise (~12 ns each), so
                                  reduction kernels scatter over these slots; sum g^2 = GRAD_SQ + sum(slots) */
    CODAE_S_N_SLOTS = 64,
    CODAE_S_ADAM_STEP = 72,  /* graph replay: Adam's step count t, written before each codae_train_step_graph launch */
    CODAE_S_COUNT = 80
};

/* One minibatch of the hot loop (train_dae_on_embedding.py:194-203). */
typedef struct {
    const float* data;       /* dataset matrix [n_rows][io] fp32 resident in HBM
                                (ConcatenatedEmbeddingDataset.data, concatenated_embedding_dataset.py:53-74) */
    const int32_t* row_idx;  /* [B] rows of `data` forming the batch (DataLoader+collate_embedding,
                                data_tool.py:96-103); NULL = rows 0..B-1 */
    const int32_t* mask_id;  /* [B] row of mask_table per sample = Corrupter.mask_to_use[idx][run]
                                (data_tool.py:252-260); NULL = no corruption */
    const uint8_t* mask_table; /* [n_masks][io] 0/1 = Corrupter.binary_masks (data_tool.py:202-209) */
    int32_t B;
    int32_t io;
    /* alternative to mask_id: look the id up on the device, id = mask_to_use[row * nb_run + run]
     * with row = row_idx[b] (Corrupter.mask_to_use, data_tool.py:222-226); used when mask_id is NULL */
    const int32_t* mask_to_use;
    int32_t nb_run;
    int32_t run;
} codae_batch;

typedef struct {
    float lr, weight_decay, beta1, beta2, eps; /* torch.optim.Adam (train_dae_on_embedding.py:160-163) */
    float max_grad_norm;   /* clip_grad_norm_(params, 1) (:213); <= 0 disables clipping.  A NaN norm gives a NaN coefficient,
                            * an infinite one 0 ("Non-finite values" above, point 3) */
    int32_t step;          /* 1-based Adam step index t */
    float loss_scale_rows; /* rows of the GLOBAL batch (data-parallel: sum over ranks); 0 = batch.B */
} codae_hyper;

const char* codae_last_error(void);
int codae_abi_version(void);
/* sizeof() of the structs above as THIS library was compiled, then CODAE_S_COUNT and CODAE_K_COUNT:
 * out[0..6] = {codae_spec, codae_sizes, codae_buffers, codae_batch, codae_hyper, CODAE_S_COUNT, CODAE_K_COUNT}.
 * A binding compares them with its own declarations before the first call (a short codae_buffers would make the
 * engine read shadow_wt past the caller's struct). */
#define CODAE_N_STRUCTS 7
int codae_struct_sizes(int32_t* out, int32_t capacity);
/* The CODAE_* tuning environment variables (CODAE_GEMM_TILE, CODAE_SINGLE_STREAM, CODAE_NO_FUSED_LOSS ...)
 * are read when the library is first used and at every codae_create, never on the launch path; a caller that
 * changes one and wants the stand-alone GEMM entry points to see it calls this. */
int codae_reload_env(void);

/* ---- handle ------------------------------------------------------------- */
int codae_create(const codae_spec* spec, codae_handle* out);
int codae_destroy(codae_handle h);
int codae_get_sizes(codae_handle h, codae_sizes* out);
/* element offset of layer l's weight / bias inside the flat parameter vector,
 * and of its bf16 shadow inside shadow_w */
int codae_param_offsets(codae_handle h, int32_t layer, int64_t* w_off, int64_t* b_off, int64_t* shadow_off);

/* ---- drop-in path: model(c_input) / loss.backward() ---------------------- */
/* forward(x) = decode(encode(x)) (embedding_denoising_autoencoder.py:137-185).
 * x [B][in0] fp32, y [B][outL] fp32.  layer_lo/layer_hi select a sub-chain
 * [layer_lo, layer_hi) for encode()/decode().  save_for_backward != 0 keeps the
 * activations in bufs->acts. */
int codae_forward(codae_handle h, const codae_buffers* bufs, const float* x, float* y, int32_t B,
                  int32_t layer_lo, int32_t layer_hi, int32_t save_for_backward, void* stream);
/* autograd of the chain (loss.backward(), train_dae_on_embedding.py:210):
 * dy [B][out of layer_hi-1] fp32 -> bufs->grads of layers [layer_lo, layer_hi) (overwritten),
 * optional dx [B][in of layer_lo] fp32.  Uses the activations the matching codae_forward left. */
int codae_backward(codae_handle h, const codae_buffers* bufs, const float* dy, float* dx, int32_t B,
                   int32_t layer_lo, int32_t layer_hi, void* stream);
/* refresh the bf16 weight shadows from bufs->params (after an external optimizer step) */
int codae_sync_shadows(codae_handle h, const codae_buffers* bufs, void* stream);

/* ---- fused training step: train_dae_on_embedding.py:198-223 --------------- */
/* gather+corrupt -> forward -> MSE(mean) loss + dL/dy + metric sums.
 * out_y (optional, [B][io] fp32) receives the reconstruction. */
int codae_step_forward_loss(codae_handle h, const codae_buffers* bufs, const codae_batch* batch,
                            const codae_hyper* hyper, float* out_y, void* stream);
/* backward for layers layer_hi-1 ... layer_lo (descending); call with decreasing
 * ranges to hand gradient buckets to the all-reduce as they complete. */
int codae_step_backward(codae_handle h, const codae_buffers* bufs, int32_t B, int32_t layer_lo,
                        int32_t layer_hi, void* stream);
/* global grad norm -> clip -> Adam -> bf16 shadow refresh (:212-215) */
int codae_step_update(codae_handle h, const codae_buffers* bufs, const codae_hyper* hyper, void* stream);
/* codae_train_step replayed from a hipGraph: the first call (and any call whose batch shape / pointers / hyper-
 * parameters differ from the captured ones) captures the whole step - both streams of the backward included - and
 * instantiates it; every call then costs one scalar write (Adam's step count, kept in device memory because kernel
 * arguments are frozen at capture) and one hipGraphLaunch instead of ~55 kernel launches.  For launch-bound shapes
 * (small batches: the reference's stock BATCH_SIZE 128).  batch->row_idx / mask_id must point to buffers whose
 * CONTENTS the caller refreshes between calls (same addresses).  Same results as codae_train_step. */
int codae_train_step_graph(codae_handle h, const codae_buffers* bufs, const codae_batch* batch,
                           const codae_hyper* hyper, void* stream);
/* Data-parallel form of codae_step_backward: returns WITHOUT making `stream` wait for the engine's side stream.
 * When it returns, the weight gradients of [layer_lo, layer_hi) are complete in enqueue order on the stream
 * codae_side_stream() reports (on `stream` itself when that is NULL), the bias and data gradients on `stream`.
 * The caller orders its consumer (a bucket all-reduce) behind the side stream, goes on with the next bucket, and calls
 * codae_join() before anything on `stream` reads the weight gradients (codae_step_update does so itself).
 * Replaces the autograd hooks torch's DistributedDataParallel would put on loss.backward()
 * (script/train_dae_on_embedding.py:210). */
int codae_step_backward_async(codae_handle h, const codae_buffers* bufs, int32_t B, int32_t layer_lo,
                              int32_t layer_hi, void* stream);
/* The stream the weight-gradient GEMMs and slab reduces run on (created on first use); NULL when the engine runs
 * everything on the caller's stream (CODAE_SINGLE_STREAM). Owned by the handle. */
int codae_side_stream(codae_handle h, void** stream_out);
/* Make `stream` wait for everything the engine still has in flight on its side stream (weight-gradient GEMMs and
 * slab reduces of a backward issued with codae_step_backward_async).  Call before anything on `stream`, another
 * stream or the host reads the weight gradients; codae_step_update does so itself. */
int codae_join(codae_handle h, void* stream);

/* ---- sharded data-parallel update (reduce-scatter -> Adam on 1/N of the parameters -> all-gather of the bf16 shadows)
 * What torch's ZeroRedundancyOptimizer would do around optimizer.step() (script/train_dae_on_embedding.py:212-215): each
 * rank owns a contiguous shard of every gradient bucket.  The caller (codae.train.DataParallel(sharded=True)) runs the
 * collectives; these three entry points are the arithmetic in between. */
/* *acc (device double) += sum g[i]^2, i in [0, n): a rank's share of clip_grad_norm_'s total norm */
int codae_span_sumsq(const float* g, int64_t n, double* acc, void* stream);
/* clip + Adam on elements [lo, hi) of the flat parameter / gradient / moment vectors, *total_sq (device double) being
 * the GLOBAL sum g^2 (all-reduced over the ranks); writes the bf16 shadow of the range (BF16 mode).  lo, hi multiples
 * of 4.  Does not touch the transposed shadow: codae_sync_transposed after the shadows have been all-gathered. */
int codae_step_update_span(codae_handle h, const codae_buffers* bufs, const codae_hyper* hyper, int64_t lo, int64_t hi,
                           const double* total_sq, void* stream);
/* shadow_wt <- transpose(shadow_w) for every layer that has a data gradient (BF16 mode; no-op otherwise) */
int codae_sync_transposed(codae_handle h, const codae_buffers* bufs, void* stream);
/* all three, single GPU.  Narrow stacks (bf16, every width a multiple of 64 and <= 512, at most 15 layers, widths summing
 * to <= 6144, batch <= 2048 rows) take the persistent fused chain instead of per-layer launches: ONE kernel for gather +
 * corruption + all forward layers + loss + the whole data-gradient chain (a workgroup walks 16 batch rows through every
 * layer; weights stream from L2 through per-wave LDS rings), ONE grouped launch for every layer's weight gradient (with
 * the norm's sum g^2), bias finish + loss finish, Adam: 4 launches instead of ~55 (the reference's stock BATCH_SIZE 128
 * on a narrow stack and BASELINE config 2 are launch-bound).  Same arithmetic, same buffers; CODAE_NO_CHAIN=1 keeps
 * the per-layer path; codae_step_path tells which one a batch size takes.
 * Wide stacks (per-layer path, batch >= 1024 rows, at most 15 layers, >= 200 tiles of 256 x 192 over all weight gradients): the
 * backward is the data-gradient chain followed by ONE grouped launch for every layer's weight gradient with the whole batch as
 * its k extent - no split-K slabs, no reduce pass (CODAE_NO_DEFER_WGRAD=1: the per-layer weight gradients of
 * codae_step_backward, which data-parallel callers use bucket by bucket). */
int codae_train_step(codae_handle h, const codae_buffers* bufs, const codae_batch* batch,
                     const codae_hyper* hyper, void* stream);
/* ---- data parallel with a library-owned RCCL communicator (one process per GPU) ----------------------------
 * RCCL is dlopen()ed on first use (the copy already in the process, else the system's): the library does not link it.
 * codae_dp_unique_id: rank 0 fills `out` (capacity >= 128 bytes) with an ncclUniqueId and ships it to the other ranks by any
 * means; codae_dp_init (collective: every rank calls it with the same id) creates this engine's communicator and its
 * highest-priority collective stream; codae_destroy / codae_dp_destroy release them. */
int codae_dp_unique_id(void* out, int32_t capacity);
int codae_dp_init(codae_handle h, const void* unique_id, int32_t rank, int32_t world);
int codae_dp_destroy(codae_handle h);
/* One data-parallel optimizer step with the collectives inside the call: forward + loss, the backward in n_buckets layer
 * ranges [bucket_lo[i], bucket_hi[i]) from the top layer down to layer 0, each range's weight gradients all-reduced (SUM, in
 * place, fp32) on the communicator's stream as soon as they exist - no host round trip between buckets -, the bias block
 * last, ONE wait of `stream` for the collectives, then clip + Adam on the summed gradients.  hyper->loss_scale_rows = the
 * GLOBAL batch rows.  (What DistributedDataParallel's bucket hooks + optimizer.step do around script/train_dae_on_embedding.py:210-215.) */
int codae_train_step_dp(codae_handle h, const codae_buffers* bufs, const codae_batch* batch, const codae_hyper* hyper,
                        int32_t n_buckets, const int32_t* bucket_lo, const int32_t* bucket_hi, void* stream);
/* 1 if codae_train_step with B rows runs the persistent chain on this engine and these buffers, 0 if the per-layer launches
 * (tests and bench lines name the path they measured).  Only the fused training step takes the chain: codae_eval_step, the
 * step-by-step entries and codae_train_step_dp always run the per-layer launches.  It is field `path` of codae_debug_step_plan. */
int codae_step_path(codae_handle h, const codae_buffers* bufs, int32_t B);
/* 1 if codae_train_step with B rows leaves its fp32 output y [B][io] in the work space (the per-layer launches with a stand-alone
 * loss: the fp32 engine, and the bf16 engine under any setting that takes the loss out of the last GEMM's epilogue), 0 if y is
 * never stored (the fused-loss epilogue, the persistent chain).  Read off the same step plan the step itself follows. */
int codae_step_stores_output(codae_handle h, const codae_buffers* bufs, int32_t B);
/* Host-only query (no HIP call is made, no device needed; the members of bufs are only tested for null, never read through):
 * which launches a call makes on this engine with its settings as they stand and the CODAE_* variables as codae_create read them.
 * Every entry point that issues a step, or a part of one, asks the same function once and hands the answer down; this entry pins
 * it in tests.
 *   call[8]: kind (0 codae_train_step, 1 codae_step_forward_loss with a hyper, 2 codae_eval_step, 3 a range of the step's backward
 *            - codae_step_backward, _async, the buckets of codae_train_step_dp -, 4 codae_backward, 5 codae_step_update), B,
 *            layer_lo, layer_hi (kinds 3 and 4), join (kind 3: 0 for _async and the buckets), dx wanted (kind 4), out_y given
 *            (kinds 1 and 2), clipping on (max_grad_norm > 0; kinds 0 and 5)
 *   out[CODAE_STEP_PLAN_FIELDS], 0 wherever the call has no such part:
 *            rows           B as the kernels see it (bf16: padded to 64)
 *            path           0 per-layer launches, 1 persistent chain
 *            loss           0 none, 1 stand-alone kernels, 2 fused into the last forward GEMM, 3 inside the chain kernel
 *            loss_finish    0 none, 1 a launch of its own, 2 carried by the bias finish that ends the backward
 *            wgrad          0 per layer, beside the data gradients; after them in one grouped launch of 1 the pipelined 256 x 192
 *                           tile, 2 the one-barrier kernel, 3 the exact-fp32 engine's bf16-plane kernel
 *            streams        1 or 2: the per-layer weight gradients go to the side stream (a grouped launch stays on the caller's)
 *            tail_on_caller layer 0's weight gradient runs on the caller's stream, third slab buffer
 *            bias_finish    0 none in this call (left pending), 1 a launch of its own, 2 trailing workgroups of the grouped launch
 *            norm           0 no clipping, 1 sum g^2 gathered by the backward's launches, 2 a flat pass in the update
 *            update         0 none, 1 the flat kernel + transposes, 2 one tiled pass
 * Not in the plan: whether the gather reads the registered bf16 image (that depends on the batch's pointers and alignment), and
 * what one call leaves for the next (pending bias rows, cleared norm scalars, a dropped forward, side-stream work not yet joined).
 * CODAE_E_INVALID for a null argument, capacity < CODAE_STEP_PLAN_FIELDS, an unknown kind, B outside (0, max_batch] (kind 5
 * takes none) or a layer range outside the stack. */
#define CODAE_STEP_PLAN_FIELDS 10
int codae_debug_step_plan(codae_handle h, const codae_buffers* bufs, const int32_t* call, int32_t* out, int32_t capacity);
/* Input noise of every training step that follows - codae_train_step, codae_train_step_graph (a change re-captures the
 * graph; under replay the step index is read from scalars[CODAE_S_ADAM_STEP]), codae_step_forward_loss with a hyper (the
 * torch.distributed data-parallel path) and codae_train_step_dp, each with hyper->step as the counter's step.  NULL or
 * CODAE_NOISE_NONE switches it off.  CODAE_E_INVALID for an unknown kind, p outside [0, 1], a negative sigma or a non-finite
 * parameter (nothing is launched, the previous setting stays).  Evaluation (codae_eval_step, hyper == NULL) is never
 * noised.  While noise is on the stack stays off the persistent chain kernel, which fuses the gather (codae_step_path
 * reports 0), exactly as a non-ReLU activation keeps it off. */
int codae_set_input_noise(codae_handle h, const codae_noise* noise);
/* The slot count and the pool of CODAE_NOISE_SWAP ("Swap noise" above) for the training steps that follow: pool [n_pool] int32 on the
 * device, borrowed until replaced, or NULL = every row (n_pool is then the dataset's row count).  Required before
 * codae_set_input_noise accepts CODAE_NOISE_SWAP; the setting is part of the graph key (a change re-captures).  pool NULL with
 * n_pool == 0 and n_slots == 0 clears it (refused while SWAP is the noise kind).  CODAE_E_INVALID for n_slots < 1 or not dividing
 * io, n_pool < 1, and an n_slots that differs from a presence table's; codae_set_input_noise returns CODAE_E_INVALID for SWAP
 * without slots and for p outside [0, 1].  On an error nothing is launched and the previous setting stays.  A bf16 step with swap
 * noise keeps gathering from the registered bf16 image (codae_set_dataset_image). */
int codae_set_swap_pool(codae_handle h, const int32_t* pool, int32_t n_pool, int32_t n_slots);
/* Loss emphasis of every training step that follows (the step forms codae_set_input_noise lists; a change re-captures the
 * graph).  NULL switches it off; alpha = beta = 1 with a NULL col_weight also means off: the engine then runs exactly the
 * launches it ran before.  CODAE_E_INVALID for a negative or non-finite alpha or beta (nothing is launched, the previous
 * setting stays).  While it is on, the loss leaves the last forward GEMM's epilogue for a stand-alone kernel on the per-layer
 * path (the route CODAE_NO_FUSED_LOSS and the fp32 engine take) and the stack stays off the persistent chain kernel
 * (codae_step_path reports 0). */
int codae_set_loss_emphasis(codae_handle h, const codae_emphasis* emphasis);
/* Training criterion of every training step that follows (the step forms codae_set_input_noise lists; a change re-captures the
 * graph).  NULL or kind CODAE_LOSS_MSE switches it off: the engine then runs exactly the launches it ran before (the fused
 * epilogue or the chain kernel, the emphasised kernel with emphasis).  CODAE_E_INVALID for an unknown kind, a beta / delta that
 * is not finite and > 0, a negative or non-finite mse_weight, an mse_weight != 0 with a kind other than SLOT_COSINE, n_slots < 1
 * or not dividing io; CODAE_E_UNSUPPORTED for n_slots > 128.  On any error nothing is launched and the previous setting stays.
 * While it is on, the loss runs as a stand-alone kernel behind the last forward GEMM, with or without emphasis, and the stack
 * stays off the persistent chain kernel (codae_step_path reports 0), exactly as with emphasis. */
int codae_set_recon_loss(codae_handle h, const codae_recon_loss* loss);
/* The mixed-variable criterion ("Mixed-variable criterion" above) as the training criterion of every step of a single process that
 * follows: codae_train_step, codae_train_step_graph (a change re-captures), codae_step_forward_loss + _backward + _update.  NULL
 * switches it off: the engine then runs exactly what it ran before.  The setter copies the table into ws (a blocking copy).  While
 * it is on, the loss runs as three stand-alone launches behind the last forward GEMM and the stack stays off the persistent chain
 * kernel (codae_step_path reports 0).  On plain steps it composes with the element noises, hidden dropout, skips, norms, the sparse
 * code, every optimizer, tied weights and the weight average; codae_train_step_graph replays the criterion on its own only (the
 * default Adam, none of those options) and returns CODAE_E_UNSUPPORTED, naming the option, otherwise.  CODAE_E_INVALID for n_var outside [1, CODAE_VAR_MAX], a null array, a size < 1,
 * an unknown type, a negative or non-finite weight, variables that overlap or leave a column of [0, io) uncovered, a ws that is
 * NULL, misaligned or smaller than codae_variable_loss_ws_bytes(n_var, max_batch).  CODAE_E_UNSUPPORTED, the message naming the
 * option, together with what assumes equal-width slots - loss emphasis, a criterion of codae_set_recon_loss, the slot contrast, a
 * slot-presence table, swap noise (their setters refuse likewise while this criterion is on) - and in codae_train_step_dp: a
 * global-batch RMSE is not a sum over shards.  On any error the previous setting stays. */
int codae_set_variable_loss(codae_handle h, const codae_variable_loss* loss);
/* Hidden dropout of every training step that follows (the step forms codae_set_input_noise lists; a change re-captures the
 * graph; under replay the step index is read from scalars[CODAE_S_ADAM_STEP]).  NULL, or every p_l == 0, switches it off: the
 * engine then runs exactly the launches it ran before.  CODAE_E_INVALID for a p_l outside [0, 1), a non-finite p_l or
 * n != n_layers - 1; CODAE_E_UNSUPPORTED for p_l > 0 on a layer whose activation is RELU6, ELU, SOFTPLUS or HARDSIGMOID (the
 * message names the layer).  On any error nothing is launched and the previous setting stays.  While it is on: one stand-alone
 * kernel behind the forward GEMM of every dropped layer and one behind the data-gradient GEMM that produces its activation
 * gradient (class CODAE_K_DROPOUT), and the stack stays off the persistent chain kernel (codae_step_path reports 0).
 * The backward entry points take no batch: a training forward records batch->row_idx and hyper->step in the handle, so
 * batch->row_idx must stay valid until the backward of that step has been issued. */
int codae_set_hidden_dropout(codae_handle h, const codae_dropout* d);
/* Residual connections ("Residual connections" above) of every call that follows - training steps in every step form AND every
 * evaluation forward; a change re-captures the graph.  NULL, or an all-zero `on`, switches them off: the engine then runs exactly
 * the launches it ran before, bit for bit, codae_step_path included, and ws may be NULL.  CODAE_E_INVALID for n != n_layers, a
 * null `on`, a ws that is NULL, not 16-byte aligned or smaller than codae_residual_ws_bytes says; CODAE_E_UNSUPPORTED for a skip
 * around the last layer, around a layer of unequal widths or around one whose activation is RELU6, ELU, SOFTPLUS or HARDSIGMOID (the
 * message names the layer and the reason).  On any error nothing is launched and the previous setting stays.  ws is borrowed until
 * the setting is replaced; it holds G and the mask bits, its contents need not be zero, and codae_sizes / codae_buffers do not
 * change.  codae_residual_ws_bytes: the bytes needed (0 when off), or -1 with the same errors.
 * While skips are on: one stand-alone kernel behind the forward GEMM of every skipped layer and one behind the data-gradient GEMM of
 * every layer l with skip_l or skip_{l-1} (class CODAE_K_DROPOUT), the stack stays off the persistent chain kernel (codae_step_path
 * reports 0), and nothing else of the step plan changes (fused loss, grouped weight gradients, two streams, the backward by ranges -
 * G lives in ws between the range calls).  codae_backward, and codae_forward over a partial layer range, return
 * CODAE_E_UNSUPPORTED.  A step backward needs a training forward before it: only that writes the masks. */
int64_t codae_residual_ws_bytes(codae_handle h, const codae_residual* r);
int codae_set_residual(codae_handle h, const codae_residual* r, void* ws, int64_t ws_bytes);
/* Normalisation ("Normalisation" above) of every call that follows - training steps in every step form AND every evaluation
 * forward; a change re-captures the graph.  NULL, or an all-zero `on`, switches it off: the engine then runs exactly the launches it
 * ran before, bit for bit, codae_step_path included, and ws may be NULL.  The error contract of codae_set_residual: CODAE_E_INVALID
 * for n != n_layers, a null `on`, an unknown kind, an eps that is not finite or not > 0, a ws that is NULL, not 16-byte aligned or
 * smaller than codae_norm_ws_bytes says; CODAE_E_UNSUPPORTED for a norm on the last layer or behind RELU6, ELU, SOFTPLUS or
 * HARDSIGMOID (the message names the layer and the reason).  On any error nothing is launched and the previous setting stays.  ws is
 * borrowed until the setting is replaced; it holds r and the 1-bit masks, its contents need not be zero, and codae_sizes /
 * codae_buffers do not change.  codae_norm_ws_bytes: the bytes needed (0 when off), or -1 with the same errors.
 * While a norm is on: one stand-alone kernel behind the forward GEMM of every normalised layer l (behind its dropout and skip
 * kernels), and behind the data-gradient GEMM of layer l + 1, which runs unmasked, one kernel that does the whole job of the
 * residual backward kernel at that site and TAKES ITS PLACE (both class CODAE_K_DROPOUT); the stack stays off the persistent chain
 * kernel (codae_step_path reports 0), and nothing else of the step plan changes.  codae_backward, and codae_forward over a partial
 * layer range, return CODAE_E_UNSUPPORTED.  A step backward needs a training forward before it: only that writes the masks. */
int64_t codae_norm_ws_bytes(codae_handle h, const codae_norm* n);
int codae_set_norm(codae_handle h, const codae_norm* n, void* ws, int64_t ws_bytes);
/* Sparse code ("Sparse code" above) of every call that follows - training steps in every step form AND every evaluation forward; a
 * change re-captures the graph.  NULL, or keep == Z, switches it off: the engine then runs exactly the launches it ran before, bit
 * for bit, codae_step_path included, and ws may be NULL.  CODAE_E_INVALID for a layer outside [1, n_layers], a keep outside [1, Z],
 * a ws that is NULL, not 16-byte aligned or smaller than codae_sparse_code_ws_bytes says; CODAE_E_UNSUPPORTED for layer == n_layers
 * (the last layer's output is the reconstruction), for a layer m behind RELU6, ELU, SOFTPLUS or HARDSIGMOID, and for a layer m that
 * the residual or the norm setting in force covers - and codae_set_residual / codae_set_norm refuse a setting that covers layer m
 * while a sparse code is on; the message names the layer and the reason ("name the layers and leave out layer m").  On any error
 * nothing is launched and the previous setting stays.  ws is borrowed until the setting is replaced; it holds the 1-bit keep mask
 * of the last training forward ([max_batch] rows, ceil(Z / 8) bytes apart; column 8 j + i in bit i of byte j, pad bits 0), its
 * contents need not be zero, and codae_sizes / codae_buffers do not change.  codae_sparse_code_ws_bytes: the bytes needed (0 when
 * off), or -1 with the same errors.
 * While it is on: one stand-alone kernel behind the forward GEMM of layer m (behind its dropout kernel), and one behind the
 * data-gradient GEMM that produces dA_m (behind the residual kernel of a skip around Linear `layer`, in front of dropout's), both
 * class CODAE_K_DROPOUT; the stack stays off the persistent chain kernel (codae_step_path reports 0), and nothing else of the step
 * plan changes.  codae_backward, and codae_forward over a partial layer range, return CODAE_E_UNSUPPORTED.  A step backward needs a
 * training forward before it: only that writes the mask. */
int64_t codae_sparse_code_ws_bytes(codae_handle h, const codae_sparse_code* c);
int codae_set_sparse_code(codae_handle h, const codae_sparse_code* c, void* ws, int64_t ws_bytes);
/* Slot contrast of every training step that follows (the step forms codae_set_input_noise lists; a change re-captures the graph;
 * under replay the step index is read from scalars[CODAE_S_ADAM_STEP]).  NULL or weight == 0 switches it off: the engine then runs
 * exactly what it ran before, bit for bit, codae_step_path included.  CODAE_E_INVALID for n_neg outside [1, 4096], a tau that is
 * not finite or < 0.01, a negative or non-finite weight, n_slots < 1, > 128 or not dividing io, n_rows < 1, a pool without entries,
 * a ws that is NULL, misaligned or smaller than codae_slot_contrast_ws_bytes says; CODAE_E_UNSUPPORTED for E > 1024 (the message
 * names E).  On any error nothing is launched and the previous setting stays.  While it is on: the criterion runs as its
 * stand-alone kernel (no fused-loss epilogue), followed by a prepare launch and the contrast launch (both booked under
 * CODAE_K_LOSS, after the criterion's record) and a one-thread finish (not timed, like the criterion's), and the stack stays off the persistent chain kernel (codae_step_path reports 0). */
int codae_set_slot_contrast(codae_handle h, const codae_slot_contrast* contrast);
/* Optimizer and schedule of every update that follows - codae_step_update, codae_step_update_span (with vmax + lo), codae_train_step,
 * codae_train_step_graph and codae_train_step_dp.  NULL, or {ADAM, amsgrad 0, CONSTANT, warmup 0}, switches it off: the engine then
 * launches exactly the kernel instantiation it launched before, with the same bits.  CODAE_E_INVALID for an unknown kind or
 * schedule, a parameter outside the range the struct names, amsgrad with SGD, nesterov without momentum, and a NULL or misaligned
 * (16 bytes) vmax with amsgrad; on an error nothing changes.  Fields the kind and the schedule do not read are ignored.  The
 * setting is part of the graph key (a change re-captures; a schedule alone never does) and never changes which forward or backward
 * path a stack takes: codae_step_path is unaffected.  vmax is borrowed until the setting is replaced; SGD leaves adam_v alone. */
int codae_set_optimizer(codae_handle h, const codae_optimizer* opt);
/* bytes of codae_optimizer.trust_ws for this handle (every update path, tied or not); 0 for a null handle */
int64_t codae_trust_ws_bytes(codae_handle h);
/* Slot presence of every step that follows - training (every step form codae_set_input_noise lists; the pointer is part of the
 * graph key) AND codae_eval_step.  present [n_rows][n_slots] uint8 on the device, borrowed until replaced; NULL switches it off: the
 * engine then runs exactly what it ran before, bit for bit, codae_step_path included.  CODAE_E_INVALID for n_slots outside [1, 128]
 * or not dividing io, n_rows < 1, and an n_slots that differs from the one a SLOT_COSINE criterion or a slot contrast is set with
 * (those two setters refuse a disagreement with the table the same way: whichever comes second), or from the swap noise's slot
 * count (codae_set_swap_pool, likewise); nothing is launched, the previous
 * setting stays.  Every row index of a batch must be < n_rows.  While a table is set codae_step_path reports 0. */
int codae_set_slot_presence(codae_handle h, const uint8_t* present, int64_t n_rows, int32_t n_slots);
/* A resident bf16 image of the dataset: image_bf16 [n_rows][io] bf16 on the device, image[r][c] = bf16(data[r][c]) as
 * codae_cast_f32_to_bf16 rounds it, borrowed until replaced; NULL clears the registration.  The bf16 engine's steps - training in
 * every step form, and codae_eval_step - then gather their input from the image instead of converting the fp32 rows again, whenever
 * batch->data == data, batch->io == io, io % 8 == 0 and the call applies no input noise other than CODAE_NOISE_SWAP (the element
 * noises are added in fp32 before the rounding; a swapped slot is a bf16 row of another row); every other call, and the fp32 engine, runs exactly what it ran before.  The gathered input has the same bits either
 * way, so no result changes; the loss keeps reading the fp32 target rows.  Every row index of such a batch must be < n_rows.  A
 * caller that rewrites the dataset in place registers the image again (after casting it again): the engine cannot see the
 * change.  The registration is part of the graph key.  CODAE_NO_DATASET_IMAGE (read at codae_create) keeps the fp32 gather.
 * CODAE_E_INVALID for an image without data, n_rows < 1, an io that is not the model's, or an image that is not 16-byte aligned;
 * the previous registration stays. */
int codae_set_dataset_image(codae_handle h, const float* data, const void* image_bf16, int64_t n_rows, int32_t io);
/* Tied weights ("Tied weights" above) of every update that follows - codae_step_update, codae_train_step, codae_train_step_graph
 * and codae_train_step_dp; codae_sync_shadows mirrors the decoder while it is on.  on = 0 switches it off: the engine then runs
 * exactly what it ran before, bit for bit.  CODAE_E_UNSUPPORTED for a stack that is not mirror-symmetric, naming the first
 * offending layer pair; nothing changes then.  The setter moves no data: call codae_sync_shadows afterwards, which makes the state
 * tied (decoder matrices and their shadows overwritten from the encoder's).  The setting is part of the graph key and never
 * changes which forward or backward path a stack takes: codae_step_path is unaffected. */
int codae_set_tied_weights(codae_handle h, int32_t on);
/* Weight average ("Weight average" above) of every update that follows - codae_step_update, codae_train_step, codae_train_step_graph
 * and codae_train_step_dp: the average is one more stream of the update's own launch.  NULL or kind CODAE_AVG_OFF switches it off:
 * the engine then launches exactly the kernel instantiations it launched before.  CODAE_E_INVALID for an unknown kind, a decay
 * outside [0, 1) or not finite, a debias that is neither 0 nor 1, start < 1, every < 1, a NULL or misaligned (16 bytes) avg; on an
 * error nothing changes.  Fields the kind does not read are ignored.  The setting is part of the graph key (a change re-captures;
 * a new weight never does) and never changes which path a stack takes.  While it is on codae_step_update_span returns
 * CODAE_E_UNSUPPORTED.  avg is borrowed until the setting is replaced; the setter moves no data. */
int codae_set_weight_average(codae_handle h, const codae_weight_average* wa);
/* how many times codae_train_step_graph has captured (and instantiated) a graph on this handle since codae_create */
int codae_graph_captures(codae_handle h);
/* validation body (:245-258): forward + metric sums only */
int codae_eval_step(codae_handle h, const codae_buffers* bufs, const codae_batch* batch, float* out_y,
                    void* stream);

/* ---- per-kernel timing (bench.py roofline leg) ------------------------------ */
/* kernel classes recorded by the engine's step/forward/backward entry points */
enum {
    CODAE_K_GEMM_FWD = 0,   /* y = act(x W^T + b) */
    CODAE_K_GEMM_DGRAD = 1, /* dx = (dy W) * relu' */
    CODAE_K_GEMM_WGRAD = 2, /* dW = dy^T x (the GEMM launch only); the grouped launch of a wide stack's step is reported as one
                             * record per weight gradient inside it, each with elapsed / count */
    CODAE_K_LOSS = 3,       /* MSE loss fwd+bwd; in the fused bf16 step: the last forward GEMM with the loss in its epilogue */
    CODAE_K_GATHER = 4,
    CODAE_K_SUMSQ = 5,
    CODAE_K_ADAM = 6,
    CODAE_K_SLAB_REDUCE = 7,
    CODAE_K_CHAIN = 8,       /* narrow stacks: gather + forward chain + loss + data-gradient chain in one launch */
    CODAE_K_BIAS_FINISH = 9, /* partial column sums -> bias gradients (+ their share of sum g^2) */
    CODAE_K_DROPOUT = 10,    /* streaming kernels between a step's GEMMs - hidden dropout: the factor on a layer's output / on its
                              * activation gradient (+ its column sums); residual connections: the skip add, and G + the derivative;
                              * normalisation: the row statistics + xhat, and Gs + the derivative */
    CODAE_K_COUNT = 11
};
/* Start recording a hipEvent pair around every launch whose class bit is set in class_mask
 * (bit k = CODAE_K_k), on the stream the launch uses; at most max_records pairs are kept. */
int codae_profile_begin(codae_handle h, uint32_t class_mask, int32_t max_records);
/* Stop recording, wait for the recorded events and return per record the class and the elapsed
 * milliseconds.  n_out receives the number of records written (<= capacity).  A class of work that rides in the launch recorded
 * just before it instead of being launched - the bias finish as trailing workgroups of the pipelined grouped weight-gradient launch -
 * is listed where the host would have issued it, as one record of exactly 0 ms: the carrying launch keeps its whole time. */
/* Time launches only in every n-th training step (default 1 = every step): an event pair costs 2-4 us of stream time,
 * which matters when the region being timed is also the throughput measurement. */
int codae_profile_stride(codae_handle h, int32_t every_n_steps);
int codae_profile_end(codae_handle h, int32_t* kinds, float* ms, int32_t capacity, int32_t* n_out);

/* ---- stand-alone ops (also used by the drop-in classes) ------------------- */
/* model.corrupt(input, mask) = input.clone()*mask (embedding_...py:226-239) */
int codae_corrupt(const float* x, const float* mask, float* out, int64_t n, void* stream);
/* The fused step's gather + input noise + slot corruption on its own (the launcher the engine uses): out[b][:] =
 * mask(noise(data[row_idx[b]][:])), fp32 or (out_bf16 != 0) bf16, rows out_ld elements apart (<= 0: io; columns past io are
 * not written).  noise NULL or CODAE_NOISE_NONE: the plain gather; `step` is the counter's step word.  noise_rows (NULL: none):
 * [B] dataset rows for the counter when batch->data is a batch that has ALREADY been gathered (row_idx NULL; the drop-in
 * scripts hold them as batch_indices) - batch row b is then read at row b and noised as dataset row noise_rows[b]. */
int codae_corrupt_batch(const codae_batch* batch, const codae_noise* noise, int32_t step, const int32_t* noise_rows, void* out,
                        int32_t out_bf16, int64_t out_ld, void* stream);
/* The emphasised loss on its own (the launcher the engine uses): y [B][io] fp32 against the clean rows of `batch`; dy fp32 or
 * (dy_bf16 != 0) bf16, rows dy_ld elements apart (<= 0: io; columns past io are not written); `noise` / `step` say which
 * elements the gather of that step replaced (NULL, NONE or GAUSSIAN: none).  One block per 32 batch rows -
 * codae_emph_loss_blocks(B) of them -, each leaving one row of colsum_part [blocks][io] (partial column sums of dy; may be NULL)
 * and one row of parts [blocks][3] doubles: sum w (x-y)^2, sum (x-y)^2, sum (1-fmask)(x-y)^2 (0 without a mask).  No atomics: the
 * same inputs give the same bits. */
int codae_emph_loss(const codae_batch* batch, const codae_noise* noise, int32_t step, const codae_emphasis* emphasis, const float* y,
                    void* dy, int32_t dy_bf16, int64_t dy_ld, float inv_n, float* colsum_part, double* parts, void* stream);
int codae_emph_loss_blocks(int32_t B);
/* A criterion other than the MSE on its own (the launcher the engine uses; "Training criterion" above has the definition):
 * arguments as codae_emph_loss, with `emphasis` NULL = all weights 1 and `loss` a validated non-MSE criterion (kind MSE:
 * CODAE_E_INVALID - that one runs on codae_emph_loss).  One block per 32 batch rows - codae_recon_loss_blocks(B) of them -, each
 * leaving one row of colsum_part [blocks][io] (may be NULL) and one row of parts [blocks][3] doubles: the criterion's sum (times
 * inv_n = L; SLOT_COSINE: mse_weight sum w d^2 + E sum W (1 - cos)), sum (x-y)^2, sum (1-fmask)(x-y)^2.  No atomics: the same
 * inputs give the same bits.  On an error nothing is launched and nothing is written. */
int codae_recon_loss_fwd_bwd(const codae_batch* batch, const codae_noise* noise, int32_t step, const codae_emphasis* emphasis,
                             const codae_recon_loss* loss, const float* y, void* dy, int32_t dy_bf16, int64_t dy_ld, float inv_n,
                             float* colsum_part, double* parts, void* stream);
int codae_recon_loss_blocks(int32_t B);
/* The mixed-variable criterion on its own (the launchers the engine uses; "Mixed-variable criterion" above has the definition): y
 * [B][io] fp32 against the clean rows of `batch`; dy fp32 or (dy_bf16 != 0) bf16 - the fp32 value rounded to nearest even -, rows
 * dy_ld elements apart (<= 0: io); one row of colsum_part [codae_variable_loss_blocks(B)][io] per 32 batch rows (partial column sums
 * of the fp32 dy; may be NULL); scalars [CODAE_S_COUNT] doubles: LAST_LOSS = L, SQ_FULL / SQ_PARTIAL += the unweighted sums, the
 * per-step norm accumulators zeroed.  `loss` is validated as by the setter (against batch->io and batch->B) and its table copied to
 * ws first.  No atomics: the same inputs give the same bits.  On an error nothing is launched and nothing is written. */
int64_t codae_variable_loss_ws_bytes(int32_t n_var, int32_t max_batch);     /* -1 out of range */
int codae_variable_loss_blocks(int32_t B);
int codae_variable_loss_fwd_bwd(const codae_batch* batch, const codae_variable_loss* loss, const float* y, void* dy, int32_t dy_bf16,
                                int64_t dy_ld, float* colsum_part, double* scalars, void* stream);
/* Slot contrast on its own (the launchers the engine uses; "Slot contrast" above has the definition).
 * codae_slot_contrast_ws_bytes: bytes of codae_slot_contrast.ws for S slots, K negatives, E columns per slot, bf16 != 0 for the bf16
 * engine (-1 out of range): the normalised candidates in the operand type, once [K][E] and once [E][K], K and E padded to
 * multiples of 32, and one int32 id per candidate.  Nothing grows with the batch.
 * codae_slot_contrast_prepare: samples, gathers and normalises the S x K candidates of `step` from data [n_rows][io] into ws.
 * codae_slot_contrast_fwd_bwd: dy is in and out - it holds what the criterion's kernel left and receives round(dy + scale W dl/dy),
 * the sum formed in fp32 and rounded once to the stored type, scale = weight / (rows S); dy_bf16 also picks the operand type of
 * the two products and must match what prepare was given.  Columns >= io and rows >= B are never written.  One block per 32
 * batch rows - codae_slot_contrast_blocks(B) of them -, each leaving one row of colsum_part [blocks][io] (column sums of the FINAL
 * stored values, widened to fp32, added in a fixed order; may be NULL) and one double of parts [blocks]: sum W l over its rows.
 * `noise` / `step` / `emphasis` say which elements carry which emphasis weight, as for codae_recon_loss_fwd_bwd.  No atomics: the
 * same inputs give the same bits.  On an error nothing is launched and nothing is written. */
int64_t codae_slot_contrast_ws_bytes(int32_t n_slots, int32_t n_neg, int32_t E, int32_t bf16);
int codae_slot_contrast_prepare(const float* data, int32_t io, const codae_slot_contrast* contrast, int32_t step, int32_t bf16, void* stream);
int codae_slot_contrast_fwd_bwd(const codae_batch* batch, const codae_noise* noise, int32_t step, const codae_emphasis* emphasis,
                                const codae_slot_contrast* contrast, const float* y, void* dy, int32_t dy_bf16, int64_t dy_ld, float scale,
                                float* colsum_part, double* parts, void* stream);
int codae_slot_contrast_blocks(int32_t B);
/* The same primitives under a presence table ("Slot presence"; the launchers the engine uses, the PRES instantiations of the same
 * kernels): arguments as their namesakes, with present [n_rows][n_slots] (NULL: exactly the namesake) in front of the stream.
 * codae_corrupt_batch_present keys the table by the row the noise counter uses (noise_rows[b] when given, which needs a noise kind).
 * codae_mse_loss_present is the un-weighted kernel of the evaluation sums: parts [blocks][2] = sum (x-y)^2, sum (1-fmask)(x-y)^2 over
 * present elements; dy NULL = sums only.  A SLOT_COSINE criterion or a contrast whose n_slots differs from the table's is refused. */
int codae_corrupt_batch_present(const codae_batch* batch, const codae_noise* noise, int32_t step, const int32_t* noise_rows, void* out,
                                int32_t out_bf16, int64_t out_ld, const uint8_t* present, int32_t n_slots, void* stream);
int codae_mse_loss_present(const codae_batch* batch, const float* y, void* dy, int32_t dy_bf16, int64_t dy_ld, float inv_n,
                           float* colsum_part, double* parts, const uint8_t* present, int32_t n_slots, void* stream);
int codae_emph_loss_present(const codae_batch* batch, const codae_noise* noise, int32_t step, const codae_emphasis* emphasis, const float* y,
                            void* dy, int32_t dy_bf16, int64_t dy_ld, float inv_n, float* colsum_part, double* parts,
                            const uint8_t* present, int32_t n_slots, void* stream);
int codae_recon_loss_fwd_bwd_present(const codae_batch* batch, const codae_noise* noise, int32_t step, const codae_emphasis* emphasis,
                                     const codae_recon_loss* loss, const float* y, void* dy, int32_t dy_bf16, int64_t dy_ld, float inv_n,
                                     float* colsum_part, double* parts, const uint8_t* present, int32_t n_slots, void* stream);
int codae_slot_contrast_prepare_present(const float* data, int32_t io, const codae_slot_contrast* contrast, int32_t step, int32_t bf16,
                                        const uint8_t* present, int32_t n_slots, void* stream);
int codae_slot_contrast_fwd_bwd_present(const codae_batch* batch, const codae_noise* noise, int32_t step, const codae_emphasis* emphasis,
                                        const codae_slot_contrast* contrast, const float* y, void* dy, int32_t dy_bf16, int64_t dy_ld,
                                        float scale, float* colsum_part, double* parts, const uint8_t* present, int32_t n_slots, void* stream);
/* The same primitives under swap noise ("Swap noise"; the launchers the engine uses).  codae_corrupt_batch_swap: arguments as
 * codae_corrupt_batch_present, noise->kind == CODAE_NOISE_SWAP, plus `dataset` - the matrix [n_rows][io] the swapped slots are read
 * from (NULL: batch->data; required with noise_rows, where batch->data is a batch that has already been gathered) - and `swap`;
 * present (may be NULL) has swap->n_slots slots.  image != 0: `batch->data` and `dataset` are bf16 images of the rows and out is
 * bf16 (the image gather; io % 8 == 0, no noise_rows).  codae_emph_loss_swap / codae_recon_loss_fwd_bwd_swap: arguments as their
 * _present namesakes with `swap` in front of the presence table; swap NULL is exactly the namesake.  The namesakes themselves stay
 * callable with unchanged behaviour (they refuse CODAE_NOISE_SWAP: it needs the descriptor). */
int codae_corrupt_batch_swap(const codae_batch* batch, const codae_noise* noise, int32_t step, const int32_t* noise_rows, const void* dataset,
                             const codae_swap* swap, void* out, int32_t out_bf16, int64_t out_ld, const uint8_t* present, int32_t image,
                             void* stream);
int codae_emph_loss_swap(const codae_batch* batch, const codae_noise* noise, int32_t step, const codae_emphasis* emphasis, const float* y,
                         void* dy, int32_t dy_bf16, int64_t dy_ld, float inv_n, float* colsum_part, double* parts, const codae_swap* swap,
                         const uint8_t* present, int32_t n_slots, void* stream);
int codae_recon_loss_fwd_bwd_swap(const codae_batch* batch, const codae_noise* noise, int32_t step, const codae_emphasis* emphasis,
                                  const codae_recon_loss* loss, const float* y, void* dy, int32_t dy_bf16, int64_t dy_ld, float inv_n,
                                  float* colsum_part, double* parts, const codae_swap* swap, const uint8_t* present, int32_t n_slots,
                                  void* stream);
/* The two hidden-dropout kernels on their own (the launchers the engine uses; "Hidden dropout" above has the definition): in
 * place on rows < B and columns < width of a [B][ld] matrix, fp32 or (bf16 != 0) bf16; pad columns and pad rows are never
 * written.  16-byte accesses where the base address, ld and width allow (bf16 x 8, fp32 x 4), element accesses otherwise.
 * layer in [0, 254] (the counter's fourth word is 1 + layer), p in [0, 1), step >= 0.  The backward form takes one block per 64
 * batch rows - codae_dropout_blocks(B) of them - and each leaves one row of colsum_part [blocks][width] (column sums of the
 * final values, widened to fp32; may be NULL) with plain stores added in a fixed order: the same inputs give the same bits. */
int codae_dropout_fwd(void* a, int32_t bf16, int64_t ld, int32_t B, int32_t width, const int32_t* row_idx, int32_t layer,
                      int32_t step, float p, uint64_t seed, void* stream);
int codae_dropout_bwd(void* d, int32_t bf16, int64_t ld, int32_t B, int32_t width, const int32_t* row_idx, int32_t layer,
                      int32_t step, float p, uint64_t seed, float* colsum_part, void* stream);
int codae_dropout_blocks(int32_t B);     /* part rows codae_dropout_bwd writes: one per 64 batch rows */
/* The two residual kernels on their own (the launchers the engine uses; "Residual connections" above has the definition), on rows
 * < B and columns < width of [B][ld] matrices, fp32 or (bf16 != 0) bf16; pad columns and pad rows are never written.  16-byte
 * accesses where every base address, every ld and the width allow (bf16 x 8, fp32 x 4), element accesses otherwise.
 * forward: y <- rne(y + x) in place; bits != NULL: first bits[b][j] <- the mask byte of columns 8 j .. 8 j + 7 of the y it read
 * (bits past the width clear), rows ld_bits >= ceil(width / 8) bytes apart.
 * backward: U = d; G = U + g_in (one fp32 add; g_in may be NULL); g_out <- G (may be NULL, may be g_in; rows ld_g floats apart);
 * d <- D rounded to the working type, D = G times the derivative, which comes from `bits` (act_kind CODAE_ACT_RELU: G or 0,
 * CODAE_ACT_LEAKY: G or G act_param[0]), from the saved activation `src` ([B][ld_src] in working precision, any CODAE_ACT_* kind
 * with its three act_param; RELU selects by the mask predicate) or is 1 (both NULL); not both.  One block per 64 batch rows -
 * codae_residual_blocks(B) of them - and each leaves one row of colsum_part [blocks][width] (column sums of the STORED D widened
 * to fp32; may be NULL) with plain stores added in a fixed order: the same inputs give the same bits. */
int codae_residual_fwd(void* y, const void* x, int32_t bf16, int64_t ldy, int64_t ldx, int32_t B, int32_t width, uint8_t* bits,
                       int64_t ld_bits, void* stream);
int codae_residual_bwd(void* d, int32_t bf16, int64_t ld, int32_t B, int32_t width, const float* g_in, float* g_out, int64_t ld_g,
                       const uint8_t* bits, int64_t ld_bits, const void* src, int64_t ld_src, int32_t act_kind, const float* act_param,
                       float* colsum_part, void* stream);
int codae_residual_blocks(int32_t B);    /* part rows codae_residual_bwd writes: one per 64 batch rows */
/* The two normalisation kernels on their own (the launchers the engine uses; "Normalisation" above has the definition), on rows
 * < B and columns < width of [B][ld] matrices, fp32 or (bf16 != 0) bf16; pad columns and pad rows are never written.  A wave owns
 * a row and reads it once per pass (sum, centred squares, write-out) - the passes after the first find it in the caches; 16-byte
 * accesses where every base address, every ld and the width allow (bf16 x 8, fp32 x 4), element accesses otherwise.
 * forward: bits != NULL: first bits[b][j] <- the mask byte of columns 8 j .. 8 j + 7 of the y it read (bits past the width clear),
 * rows ld_bits >= ceil(width / 8) bytes apart; then y <- xhat in place and rstd[b] <- r.
 * backward: U = d; Gh = U + g_in (one fp32 add; g_in may be NULL); Gs from Gh, xhat ([B][ld_x], working precision) and rstd;
 * g_out <- Gs (may be NULL, may be g_in; rows ld_g floats apart); d <- D = Gs times the derivative rounded to the working type,
 * the derivative from `bits` (act_kind CODAE_ACT_RELU: Gs or 0, CODAE_ACT_LEAKY: Gs or Gs act_param[0]) or 1 (bits NULL).  One block
 * per 64 batch rows - codae_norm_blocks(B) of them - and each leaves one row of colsum_part [blocks][width] (column sums of the
 * STORED D widened to fp32; may be NULL) with plain stores added in a fixed order: the same inputs give the same bits, and a row's
 * results do not depend on the other rows of the call. */
int codae_norm_fwd(void* y, int32_t bf16, int64_t ld, int32_t B, int32_t width, int32_t kind, float eps, float* rstd, uint8_t* bits,
                   int64_t ld_bits, void* stream);
int codae_norm_bwd(void* d, int32_t bf16, int64_t ld, int32_t B, int32_t width, int32_t kind, const void* xhat, int64_t ld_x,
                   const float* rstd, const float* g_in, float* g_out, int64_t ld_g, const uint8_t* bits, int64_t ld_bits,
                   int32_t act_kind, const float* act_param, float* colsum_part, void* stream);
int codae_norm_blocks(int32_t B);        /* part rows codae_norm_bwd writes: one per 64 batch rows */
/* The two sparse-code kernels on their own (the launchers the engine uses; "Sparse code" above has the definition), on rows < B and
 * columns < width of a [B][ld] matrix, fp32 or (bf16 != 0) bf16; pad columns and pad rows are never touched.  Both move bits, not
 * floats; 16-byte accesses where the base address, ld and the width allow (bf16 x 8, fp32 x 4), element accesses otherwise.
 * forward: a wave owns a row and finds its keep-th key by a radix select over the 15 / 31 magnitude bits (8-bit digits, a histogram
 * of integer counts per wave; the row is re-read per pass, so any width >= 1 works), resolves ties at that key by ascending column
 * and rewrites the row in place; 1 <= keep <= width (keep == width keeps every bit).  bits != NULL: bits[b][j] <- the keep mask of
 * columns 8 j .. 8 j + 7 (bits past the width clear), rows ld_bits >= ceil(width / 8) bytes apart; bits == NULL (an evaluation
 * forward) gives the same values.
 * backward: d <- kept ? d : +0 in place from `bits`.  One block per 64 batch rows - codae_sparse_code_blocks(B) of them - and each
 * leaves one row of colsum_part [blocks][width] (column sums of the STORED d widened to fp32; may be NULL) with plain stores added
 * in a fixed order.  The same inputs give the same bits, and a row's results do not depend on the other rows of the call. */
int codae_sparse_code_fwd(void* y, int32_t bf16, int64_t ld, int32_t B, int32_t width, int32_t keep, uint8_t* bits, int64_t ld_bits,
                          void* stream);
int codae_sparse_code_bwd(void* d, int32_t bf16, int64_t ld, int32_t B, int32_t width, const uint8_t* bits, int64_t ld_bits,
                          float* colsum_part, void* stream);
int codae_sparse_code_blocks(int32_t B); /* part rows codae_sparse_code_bwd writes: one per 64 batch rows */
/* The Gaussian kind's device arithmetic on given words (tools/noise_accuracy.py sweeps all 2^24 values of u1 and of u2 through
 * it): rho[i] = sqrt(-2 ln u1(ra[i])), c[i] = cos(2 pi u2(rb[i])), s[i] = sin(2 pi u2(rb[i])); the unit normals of a pair are
 * rho c and rho s. */
int codae_noise_box_muller(const uint32_t* ra, const uint32_t* rb, float* rho, float* c, float* s, int64_t n, void* stream);
/* Corrupter.get_masks (data_tool.py:239-262): masks[k][b][:] = table[id_b] if k_of_mask[id_b]==k+1 else 0;
 * fmask = sum_k masks[k].  masks_out is [k_max][B][io] contiguous, fmask_out [B][io]. */
int codae_expand_masks(const int32_t* mask_id, const uint8_t* mask_table, const int32_t* k_of_mask,
                       int32_t B, int32_t io, int32_t k_max, float* masks_out, float* fmask_out,
                       void* stream);
/* MSELoss fwd+bwd + metric sums on dense tensors: dy = 2 (y-x) * inv_n; scalars as CODAE_S_*.
 * fmask may be NULL (then SQ_PARTIAL is not touched). */
int codae_mse_loss_fwd_bwd(const float* x, const float* y, const float* fmask, float* dy, int64_t n,
                           float inv_n, double* scalars, void* stream);
/* clip_grad_norm_ + Adam on flat vectors (train_dae_on_embedding.py:212-215) */
int codae_clip_adam(float* params, float* grads, float* adam_m, float* adam_v, int64_t n,
                    const codae_hyper* hyper, double* scalars, void* stream);
/* The same with an optimizer setting ("Optimizer and schedule"; opt NULL = codae_clip_adam): v may be NULL under SGD, vmax is
 * read and written under amsgrad only (opt->vmax is not used here).  t = hyper->step. */
int codae_optimizer_update(float* p, float* g, float* m, float* v, float* vmax, int64_t n, const codae_hyper* hyper,
                           const codae_optimizer* opt, double* scalars, void* stream);

/* LAMB / LARS on one tensor: [0, n) is ONE matrix (opt->kind one of the two; opt->trust_ws is not used here).  trust_ws: 16-byte
 * aligned, ws_bytes >= codae_trust_ws_bytes_flat(n) = 256 + 16 ceil(n / CODAE_TRUST_CHUNK); the ratio is left in ((float*)trust_ws)[0].
 * v may be NULL under LARS.  For loops that keep their own backward, and for tests that plant state at odd sizes. */
int64_t codae_trust_ws_bytes_flat(int64_t n);
int codae_trust_update(float* p, float* g, float* m, float* v, int64_t n, const codae_hyper* hyper, const codae_optimizer* opt,
                       double* scalars, void* trust_ws, int64_t ws_bytes, void* stream);

/* The weight average on its own, for loops that keep another optimizer: avg[i] <- the definition of "Weight average" with p' = p[i],
 * i in [0, n), t = step; wa->avg is not used here.  A step that does not sample launches nothing.  float4 accesses for the body,
 * scalar ones for the tail; avg and p 16-byte aligned, nothing else demanded.  Validated as the setter validates. */
int codae_weight_average_update(float* avg, const float* p, int64_t n, const codae_weight_average* wa, int32_t step, void* stream);

/* The fold of "Tied weights" on caller-supplied buffers: for every pair, grads[enc_off + i cols + j] += grads[dec_off + j rows + i]
 * (fp32, that operand order), then the decoder range <- +0.  Nothing outside the paired ranges is touched.  Ranges must not
 * overlap; any n_pairs >= 1 (64 per launch).  16-byte accesses when every offset, rows and cols are multiples of 4. */
int codae_tie_fold(float* grads, const codae_tie_pair* pairs, int32_t n_pairs, void* stream);
/* The mirror of "Tied weights" on caller-supplied buffers: for every pair, params[dec_off + j rows + i] = params[enc_off + i cols + j];
 * with shadow_w (bf16 [>= the parameter layout], may be NULL) shadow_w[dec_off ..] = bf16 of those values; with shadow_wt (may be
 * NULL) shadow_wt[dec_off + i cols + j] = bf16(params[enc_off + i cols + j]) - the decoder matrix transposed.  Nothing else is
 * written.  With a shadow, every offset, rows and cols must be multiples of 8 (what the bf16 engine's layout guarantees). */
int codae_tie_mirror(float* params, void* shadow_w, void* shadow_wt, const codae_tie_pair* pairs, int32_t n_pairs, void* stream);

/* ---- "next" rows: abalone loss and validation rank metric ---- */
/* CombinedCriterion(reduction="mean") forward + gradient (codae/tool/metering.py:155-180): per variable v with
 * span [var_pos[v], +var_size[v]): type 0 regression -> w_v * sqrt(mean (x-y)^2), type 1 classification ->
 * w_v * mean_B NLL(log_softmax(y_span), argmax x_span); loss = sum / n_var.  acc: n_var doubles of scratch;
 * dy [B][io] (may be NULL), loss_out: one double. */
int codae_combined_loss_fwd_bwd(const float* x, const float* y, int32_t B, int32_t io, int32_t n_var, const int32_t* var_pos,
                                const int32_t* var_size, const int32_t* var_type, const float* var_weight, double* acc,
                                float* dy, double* loss_out, void* stream);
/* CombinedCriterion(reduction="none") (metering.py:131-152): out[B][n_var] = squared error (size-1 regression) or NLL */
int codae_combined_loss_full(const float* x, const float* y, int32_t B, int32_t io, int32_t n_var, const int32_t* var_pos,
                             const int32_t* var_size, const int32_t* var_type, float* out, void* stream);
/* The abalone script's per-step accounting (script/train_dae_on_abalone.py:227-236 of the reference; metering.py:131-152,
 * 187-204) without leaving the device: the monitor criterion L[b][v] of (x', y') - squared error of a size-1 regression
 * variable, NLL of a one-hot block - where x' = x * undo_scale + undo_min per column (Normalizer.undo, data_tool.py:80-90;
 * both NULL = identity; a one-hot column has scale 1, min 0), added into
 *   acc[0]                       f   += sum_{b,v} L[b][v]
 *   acc[1]                       p   += sum_{b,v} L[b][v] [variable v is blanked in sample b]        (get_partial)
 *   acc[2 + k*n_var + v]         f_k += sum_{b: k_b = k+1} L[b][v]                                    (get_per_k)
 *   acc[2 + (k_max+k)*n_var + v] p_k += sum_{b: k_b = k+1} L[b][v] [v blanked in b]
 * with k_b = k_of_mask[mask_id[b]] and "blanked" = mask_table[mask_id[b]][var_pos[v]] == 0 (the Corrupter's tables).  fp64
 * accumulators, one workgroup, additions in a fixed order (the same bits every run); read them once per epoch.  k_max <= 16. */
int codae_monitor_accumulate(const float* x, const float* y, int32_t B, int32_t io, int32_t n_var, const int32_t* var_pos,
                             const int32_t* var_size, const int32_t* var_type, const float* undo_scale, const float* undo_min,
                             const int32_t* mask_id, const uint8_t* mask_table, const int32_t* k_of_mask, int32_t k_max,
                             double* acc, void* stream);
/* out[r] = ||m[r][:]||_2 */
int codae_row_norms(const float* m, int64_t rows, int32_t E, float* out, void* stream);
/* RankingLoss.get (metering.py:46-79): *out += sum_b 1 - rank_b / (n_val - 1); inventory [n_slots][n_obs][E] =
 * dataset.data_per_category (unscaled), inventory_norm [n_slots][n_obs] its row norms, idx[B] dataset index of
 * each sample, val_idx[n_val] the validation indices. */
int codae_ranking_loss(const float* pred, const float* fmask, const int32_t* idx, int32_t B, int32_t io, int32_t n_slots,
                       int32_t E, const float* inventory, const float* inventory_norm, int64_t n_obs, const int32_t* val_idx,
                       int32_t n_val, double* out, void* stream);

/* RankingLoss.get for a whole validation batch as GEMMs (metering.py:46-79), nothing through the host:
 * blanked slot of sample b from mask_table[id_b] with id_b = mask_id[b] or mask_to_use[row_idx[b] * nb_run + run] (the
 * Corrupter's device tables, as codae_batch); similarities pred[:, slot] . inv_val^T by the fp32 GEMM of the parity engine, chunk
 * validation rows at a time; *out += sum_b 1 - rank_b / (n_val - 1) (accumulates over the batches of an epoch).
 * inv_val [n_slots][n_val][E] = codae_gather_inventory_rows(inventory, val_idx), inv_val_norm its row norms;
 * val_pos [n_obs]: position of an observation in val_idx or -1 (a sample's own validation row is never counted: the
 * reference compares s[idx] with itself there), may be NULL.  val_group [n_slots][n_val] (or NULL): rows of one slot's
 * validation inventory with the same group id hold the same bytes; the reference never counts such a row against the
 * sample it duplicates either (its two similarities come out of ONE cosine_similarity call and s[idx] > s[j] is false for
 * equal values), while here the sample's own similarity and the GEMM's column are summed in different orders - so exact
 * duplicates are skipped by identity, not by arithmetic coincidence.  Every slot's GEMM runs over the rows that blank THAT slot
 * only (compacted on the device).  Workspaces: work B * chunk floats; row_state 32 * B bytes; perm_ws (n_slots * B +
 * n_slots) int32; q_ws B * E floats. */
int codae_ranking_loss_batched(const float* pred, int32_t B, int32_t io, int32_t n_slots, int32_t E, const int32_t* row_idx,
                               const int32_t* mask_id, const int32_t* mask_to_use, int32_t nb_run, int32_t run,
                               const uint8_t* mask_table, const float* inventory, const float* inventory_norm, int64_t n_obs,
                               const float* inv_val, const float* inv_val_norm, const int32_t* val_pos, const int32_t* val_group,
                               int32_t n_val, float* work, int32_t chunk, void* row_state, int32_t* perm_ws, float* q_ws, double* out,
                               void* stream);
/* dst[c][j][:] = inventory[c][val_idx[j]][:]  (inventory [n_slots][n_obs][E]) */
int codae_gather_inventory_rows(const float* inventory, int64_t n_obs, int32_t E, int32_t n_slots, const int32_t* val_idx,
                                int32_t n_val, float* dst, void* stream);

/* ---- complementarity inference: the k best inventory items for a blanked slot (README step IV) ------------------------
 * Order: score descending, equal scores by ascending candidate position (-0 == +0); NaN scores are never selected; a row
 * with fewer than k candidates ends in (-1, -inf).  1 <= k <= 256.  Deterministic: no float atomics, no host
 * synchronisation, the same bits every run.
 * Selection primitive (running top-k over chunks of a score matrix).  state: B * k (score, index) pairs, one uint64 key each
 * (8 * B * k bytes), owned by the caller and carried across merge calls.
 *   codae_topk_init    state <- empty
 *   codae_topk_merge   rows r < rows of scores[rows][ld] (n columns = candidates col0 .. col0 + n - 1) merged into state row
 *                      row_map[r] (NULL: r); skip_col [B] (NULL: none): the candidate (a global column, -1 = none) that row
 *                      b never selects
 *   codae_topk_finish  out_idx [B][k] = cand_row_id[position] (NULL: the position itself), out_score [B][k] */
int codae_topk_init(void* state, int32_t B, int32_t k, void* stream);
int codae_topk_merge(const float* scores, int64_t ld, int32_t rows, int32_t n, int32_t col0, int32_t k, const int32_t* row_map,
                     const int32_t* skip_col, void* state, void* stream);
int codae_topk_finish(const void* state, int32_t B, int32_t k, const int32_t* cand_row_id, int32_t* out_idx, float* out_score,
                      void* stream);
/* End to end, modelled on codae_ranking_loss_batched: query b is pred[b][c E : (c+1) E] for its slot c, either slot[b] (a
 * slot outside [0, n_slots) gives an all (-1, -inf) row) or, with slot NULL, the blanked slot of mask_table[id_b], id_b =
 * mask_id[b] or mask_to_use[row_idx[b] * nb_run + run] (as rank_prep).  Candidates of slot c: rows [0, cand_count[c]) of
 * cand [n_slots][n_cand][E] (cand_count: HOST array [n_slots], NULL = n_cand each), cand_norm [n_slots][n_cand] their norms,
 * cand_row_id [n_slots][n_cand] their dataset row ids (ascending within a slot).  Score = <q, v> / (max(|q|, 1e-8)
 * max(|v|, 1e-8)).  exclude [B] (NULL: none): query b never gets the candidate cand_pos[c][exclude[b]] (cand_pos
 * [n_slots][n_obs]: dataset row -> candidate position of slot c, or -1).  Per slot: the slot's queries compacted on the
 * device, one fp32 GEMM (the parity engine's, CODAE_F32_GEMM applies) per chunk of candidates, one selection pass over it;
 * then one finish pass.  Workspaces: work B * chunk floats; row_state 12 * B bytes; perm_ws (n_slots * B + n_slots) int32;
 * q_ws B * E floats; topk_state 8 * B * k bytes.  out_idx [B][k] int32 dataset rows, out_score [B][k]. */
int codae_complete_topk(const float* pred, int32_t B, int32_t io, int32_t n_slots, int32_t E, const int32_t* slot,
                        const int32_t* row_idx, const int32_t* mask_id, const int32_t* mask_to_use, int32_t nb_run, int32_t run,
                        const uint8_t* mask_table, const float* cand, const float* cand_norm, const int32_t* cand_row_id,
                        int32_t n_cand, const int32_t* cand_count, const int32_t* exclude, const int32_t* cand_pos, int64_t n_obs,
                        int32_t k, float* work, int32_t chunk, void* row_state, int32_t* perm_ws, float* q_ws, void* topk_state,
                        int32_t* out_idx, float* out_score, void* stream);

/* ---- Retrieval metrics: hit@k, MRR, rank error and a position histogram of a validation batch, per slot ---------------
 * What codae_complete_topk serves, scored: modelled on it, and fed the same candidate tables.
 * Items.  Slot c's items are rows [0, cand_count[c]) of cand [n_slots][n_cand][E] (cand_count: HOST array), cand_norm
 * [n_slots][n_cand] their norms, cand_pos [n_slots][n_obs] the item a dataset row belongs to in slot c, or -1.  Rows holding
 * the same bytes have already been folded into one item by whoever built the tables (or not: then an item is a row).
 * Query pairs.  (b, c) is a pair iff mask_table[id_b][c E] == 0 (id_b = mask_id[b] or mask_to_use[row_idx[b] * nb_run + run], as
 * codae_batch), presence[row_idx[b]][c] != 0 (presence uint8 [n_obs][n_slots], NULL = every slot of every row) and the slot has a
 * competitor.  EVERY blanked slot the row has is a pair: a mask that blanks two slots gives two.
 * Scores.  own = cos(pred[b][cE:(c+1)E], inventory[c][row_idx[b]]), s_j the same cosine against item j (the GEMM's dot product
 * over |q| max(|v_j|, 1e-8)), both norms clamped at 1e-8; fp32.
 * Position.  Competitors: every item of slot c but the one row_idx[b] belongs to (cand_pos >= 0), n of them;
 * beaten = #{competitors: own > s_j}; p = 1 + n - beaten in [1, n + 1].  Ties and NaN on either side count against the model.
 * acc: double [n_slots][CODAE_RM_STRIDE], ADDED to (the caller zeroes it; it accumulates over the batches of an epoch):
 *   [CODAE_RM_PAIRS] pairs   [CODAE_RM_RRE] sum (p - 1) / n   [CODAE_RM_RR] sum 1 / p
 *   [CODAE_RM_HIT + i] #{p <= ks[i]}, i < n_ks <= CODAE_RM_MAX_KS (ks: HOST array, ascending positive ints)
 *   [CODAE_RM_HIST + i] #{floor(log2 p) == i}, i < 32
 * Counts are exact integers; the two sums are added per slot by one workgroup in a fixed order: the same bits every run, no
 * float atomics, no host synchronisation.
 * Three kernels: prepare (one wave per batch row; the pairs of a slot compacted with one atomic per slot and workgroup), per
 * slot and chunk of items gemm_f32 over the slot's pairs only (row count on the device) followed by the compare-and-count pass
 * (every score read once with 16-byte loads: chunk % 4 == 0, n_cand % 4 == 0, work and cand_norm 16-byte aligned), then one
 * finish workgroup per slot.
 * Workspaces: work B * chunk floats; pair_state 16 * n_slots * B bytes; perm_ws (n_slots * B + n_slots) int32; q_ws B * E floats. */
#define CODAE_RM_PAIRS 0
#define CODAE_RM_RRE 1
#define CODAE_RM_RR 2
#define CODAE_RM_HIT 3
#define CODAE_RM_MAX_KS 8
#define CODAE_RM_HIST 16
#define CODAE_RM_STRIDE 48
int codae_retrieval_metrics_batched(const float* pred, int32_t B, int32_t io, int32_t n_slots, int32_t E, const int32_t* row_idx,
                                    const int32_t* mask_id, const int32_t* mask_to_use, int32_t nb_run, int32_t run,
                                    const uint8_t* mask_table, const uint8_t* presence, const float* inventory,
                                    const float* inventory_norm, int64_t n_obs, const float* cand, const float* cand_norm,
                                    int32_t n_cand, const int32_t* cand_count, const int32_t* cand_pos, const int32_t* ks, int32_t n_ks,
                                    float* work, int32_t chunk, void* pair_state, int32_t* perm_ws, float* q_ws, double* acc,
                                    void* stream);

/* ---- Assembled outfits and compatibility --------------------------------------------------------------------------------
 * S slots, E columns per slot, io = S E.  data [n_rows][io] fp32, optionally with its bf16 image (codae_cast_f32_to_bf16).
 * Assembled outfit.  items int32 [Q][S]: items[q][s] = r >= 0 says slot s of outfit q holds the slot-s item of dataset row r; a
 * negative value (and, in the kernels, a value >= n_rows: no index reaches memory unchecked) says the outfit has no item there.  With
 * a presence table (uint8 [n_rows][S], "Slot presence"), present[r][s] == 0 makes the pair absent exactly as a negative entry does:
 * selection, what data holds there is never read into a result and may be NaN.  n_q = present slots of outfit q.
 * Assemble.  X[row][s E + e] = +0 if the pair (q, s) is absent or slot s is blanked for this row, else src[items[q][s]][s E + e];
 * src = the fp32 rows or (src_bf16) the bf16 image, which assembles into bf16 rows only.  Two forms: blank int32 [Q] or NULL - one
 * output row per outfit, slot blank[q] blanked (negative: none); leave_one_out != 0 - S rows per outfit, row q S + v has slot v
 * blanked (blank must be NULL).  A copy: bit-exact (fp32 -> bf16 rounds to nearest even as every gather here), a NaN in a present
 * unblanked element is copied.  out rows out_ld elements apart (<= 0: io).  16 bytes per lane where E, the strides and the pointers
 * allow (8 columns into bf16, 4 into fp32), narrower forms elsewhere; a blanked or absent group is stored as zeros and never loaded.
 * Slot scores.  Y [Q S][y_ld] fp32 = the evaluation forward of the leave-one-out rows (live or averaged weights, no noise, no
 * dropout, no criterion, no metric sums touched, no presence lookup by batch position).  For a present pair, y = Y[q S + s][slot s],
 * x = data[items[q][s]][slot s]:
 *   cos[q][s] = dot / (max(|x|, eps) max(|y|, eps)), eps = CODAE_COS_EPS, as CODAE_LOSS_SLOT_COSINE defines it
 *   sq[q][s]  = sum (x - y)^2
 * fp32 products and sums in an order that depends on E (and on whether the 16-byte form applies) alone: the bits do not depend on Q,
 * on the position in the batch or on the chunking.  Absent pairs: cos = sq = 0, not counted.
 * Outfit score.  score[q] = (sum over present s, ascending, of cos[q][s]) / n_q in fp32; NaN when n_q < 2 (an outfit of one item has
 * no context to be reconstructed from); a NaN in Y propagates.  n_present[q] = n_q.
 * AUC.  Positive scores pos [P], negative scores neg [M], neg_slot [M] the slot that was swapped, neg_parent [M] (or NULL) the
 * positive each negative was made from.  pos_on uint8 [P] (or NULL = all): a positive that is off takes part in nothing, nor does a
 * negative whose slot lies outside [0, n_slots) or whose parent is off.  A pair (i, j) is a win iff pos_i > neg_j, a tie iff pos_i ==
 * neg_j, everything else - every comparison with a NaN on either side included - a loss: a collapsed model scores last, as in the
 * retrieval metrics.  counts int64 [n_slots + 1][CODAE_AUC_STRIDE], overwritten:
 *   counts[s] = {wins, ties, pairs = live positives x live negatives of slot s, paired wins = #{j of slot s: pos[parent_j] > neg_j}}
 *   counts[n_slots] = {live positives, live negatives, 0, 0}
 * auc = (wins + ties / 2) / pairs per slot and in total (the caller divides: pairs 0 has no AUC); paired accuracy = paired wins /
 * live negatives.  Exact 64-bit integers: per-workgroup partial counts with plain stores (parts_ws: codae_auc_blocks(M) * n_slots * 3
 * 64-bit words), one finish workgroup adding them in a fixed order; the same bits every run.
 * codae_score_outfits: assemble (leave-one-out) -> the engine's forward launches of an evaluation step -> slot scores for Q outfits,
 * Q n_slots <= max_batch, in the engine's own workspaces, without a host synchronisation; data = the dataset the items index (bf16
 * engine: its registered image is read when there is one), the presence table = the engine's (codae_set_slot_presence), b = the live
 * buffers or those of the weight average.  cos, sq [Q][n_slots], score [Q], n_present int32 [Q].
 * CODAE_E_INVALID with the offending value in codae_last_error(): n_slots outside 1 .. 128 or not dividing io, Q < 1, Q n_slots >
 * max_batch (codae_score_outfits), a presence table of another shape, P or M < 1. */
#define CODAE_AUC_WINS 0
#define CODAE_AUC_TIES 1
#define CODAE_AUC_PAIRS 2
#define CODAE_AUC_PAIRED 3
#define CODAE_AUC_STRIDE 4
int codae_assemble_outfits(const void* src, int32_t src_bf16, int64_t n_rows, int32_t io, int32_t n_slots, const int32_t* items, int32_t Q,
                           const int32_t* blank, int32_t leave_one_out, const uint8_t* present, void* out, int32_t out_bf16, int64_t out_ld,
                           void* stream);
int codae_outfit_scores(const float* data, int64_t n_rows, int32_t io, int32_t n_slots, const int32_t* items, int32_t Q,
                        const uint8_t* present, const float* Y, int64_t y_ld, float* cos, float* sq, float* score, int32_t* n_present,
                        void* stream);
int codae_auc_blocks(int32_t M);
int codae_auc_counts(const float* pos, const uint8_t* pos_on, int32_t P, const float* neg, const int32_t* neg_slot,
                     const int32_t* neg_parent, int32_t M, int32_t n_slots, void* parts_ws, int64_t* counts, void* stream);
int codae_score_outfits(codae_handle h, const codae_buffers* b, const float* data, int64_t n_rows, const int32_t* items, int32_t Q,
                        int32_t n_slots, float* cos, float* sq, float* score, int32_t* n_present, void* stream);

/* ---- Outfit codes -----------------------------------------------------------------------------------------------------------
 * The latent vector of an outfit, and the way back from it.  L Linears, h_0 the input, h_{l+1} as "Normalisation" defines it.
 * Layer count.  A forward over the first k Linears, 1 <= k <= L - 1, yields h_k: the tensor the engine keeps in act[k] - the output
 * of Linear k - 1 after its activation, its skip and its norm, where the settings put one - and exactly what Linear k reads.  It is
 * an evaluation forward: no noise, no dropout, no criterion, no loss kernel, the metric sums are not touched.
 * Values.  bf16 engine: bf16 numbers widened to fp32 (the low 16 bits of every word are zero), the bits the decoder consumes; fp32
 * engine: the fp32 activations.
 * codae_export_rows: dst[b][c] <- the stored src[b][c] widened to fp32, exactly (-0 and NaN payloads included), for b < B, c < width;
 * src [B][ld_src] fp32 or (bf16 != 0) bf16, dst [B][ld_dst] fp32.  norm (or NULL) [B]: norm[b] = sqrt(sum_c v^2) in fp32 - the
 * cand_norm of codae_complete_topk for a bank of codes, without a second pass (codae_row_norms) over it.  Columns of dst at or past
 * width and rows at or past B are never written; src is never written.  A wave owns a row; 16-byte accesses where src and dst are
 * 16-byte aligned, ld_src and width whole chunks (bf16 x 8, fp32 x 4) and ld_dst a multiple of 4, element accesses otherwise.  A
 * lane adds its columns in ascending order and the 64 lanes are combined in one fixed tree: the bits of norm[b] depend on the row's
 * values and width alone - not on B, the row's position, the leading dimensions or the access path.  No atomics: a NaN or Inf
 * element gives its own row a NaN or Inf norm and touches no other.  CODAE_E_INVALID before any launch: a NULL or aliased src / dst,
 * bf16 outside {0, 1}, B or width < 1, a leading dimension below width.
 * codae_encode: x [B][io] dense fp32 -> act[0] as codae_forward ingests it, Linears 0 .. layers - 1 each into act[l + 1] - so every
 * skip and norm of those layers runs, which a partial codae_forward cannot offer and refuses -, then code [B][out[layers - 1]]
 * contiguous <- act[layers] through codae_export_rows, with norm [B] (or NULL).
 * codae_decode: code [B][in[layer_lo]] dense fp32 -> act[layer_lo] the same way, Linears layer_lo .. L - 1 with their skips and
 * norms (a skip around Linear layer_lo reads the code itself), the last one into y [B][io] fp32.  decode(encode(x)) has the bits of
 * an evaluation forward of x at the same B.
 * Both take b = the live buffers or those of the weight average; neither touches scalars, the parameters, the optimizer state, the
 * step count or any random stream.  BOTH OVERWRITE THE ACTIVATIONS OF THE LAST FORWARD, as an evaluation does: a
 * codae_step_backward must not follow one of them.  CODAE_E_INVALID, with the engine's state unchanged: layers / layer_lo outside
 * [1, L - 1], B outside [1, max_batch], a NULL argument. */
int codae_export_rows(const void* src, int32_t bf16, int64_t ld_src, int32_t B, int32_t width, float* dst, int64_t ld_dst, float* norm,
                      void* stream);
int codae_encode(codae_handle h, const codae_buffers* b, const float* x, int32_t B, int32_t layers, float* code, float* norm, void* stream);
int codae_decode(codae_handle h, const codae_buffers* b, const float* code, int32_t B, int32_t layer_lo, float* y, void* stream);

/* ---- Code clusters ----------------------------------------------------------------------------------------------------------
 * Spherical k-means over a bank of codes: "which kinds of outfit are there, and to which does this one belong?".  The metric is the
 * cosine, as in codae_complete_topk and the per-slot cosine loss.  codae.tool.CodeClusters is the Python side and states the same
 * definitions in whole-tensor torch ops for host tensors.
 * Notation.  x [M][Z] the bank (fp32), n_r its fp32 row norms as codae_export_rows leaves them, c [K][Z] fp32 centroids,
 * eps = CODAE_COS_EPS.  op(v) is v as the product sees it: v itself in the f32 form (op_bf16 = 0), v rounded to bf16, nearest even, in
 * the bf16 form (op_bf16 = 1).  A bank exported by the bf16 engine is bf16-valued already: only the centroids are rounded there.
 * Nearest centroid (codae_nearest_centroid).
 *   d[r][j] = sum_z op(x[r][z]) op(c[j][z]), accumulated in fp32 on the matrix cores.  The order of accumulation depends on Z alone: a
 *   row's result does not depend on M, on the row's position, on its neighbours in a tile, on K's padding or on how the caller chunks
 *   the rows; nor on the leading dimensions or the access path.
 *   assign[r] = the lowest j whose d[r][j] equals the maximum over the non-NaN d[r][.]: -0 == +0, a tie goes to the lower index, a NaN
 *   never wins.  assign[r] = -1 when every d[r][.] is NaN.
 *   best[r] = d[r][assign[r]] / max(n_r, eps); the raw dot product when norm is NULL; NaN when assign[r] = -1.
 *   Pad centroids and pad columns never take part: a pad's zero score does not beat a row whose real scores are all negative.
 *   The [M][K] scores are never written: a wave keeps a running (max, index) pair per row across groups of 128 centroids.
 *   ws: codae_nearest_centroid_ws_bytes(Z, K, op_bf16) bytes, 16-byte aligned: the centroids in the operand type, padded with zeros, staged
 *   once per call.  x is read 16 bytes at a time where x is 16-byte aligned and ld_x and Z are multiples of 4, element by element
 *   otherwise; padding is the library's business: caller memory past Z or K is never read and may hold NaN.  assign is int64 [M].
 * Centroid update (codae_centroid_update).
 *   sum_j = sum_{r : assign[r] = j} x[r] / max(n_r, eps): one fp32 division per element, fp32 adds; count_j = the number of members.
 *   count_j > 0: c'[j] = sum_j / max(|sum_j|, eps), |sum_j| in fp32 in a fixed order.  count_j == 0: c'[j] = c[j] bit for bit - an empty
 *   cluster keeps its centroid.  Rows with assign = -1 (or outside [0, K)) belong to nobody.
 *   No float atomics: the rows are ordered by (cluster, row) with a counting sort (integer atomics count), every cluster's members are
 *   added in ascending row order in a fixed tree.  The bits of c' are the same on every run and depend on no chunk or work space size.
 *   counts int64 [K] <- count_j.  c_out may alias c_in.  ws: codae_centroid_update_ws_bytes(M, Z, K) bytes, 16-byte aligned.
 * Fit (codae.tool.CodeClusters.fit).  Given c_0 and iters >= 0, for i = 0 .. iters - 1: a_i = nearest(c_i); changed[i] =
 * #{r : a_i[r] != a_{i-1}[r]}, changed[0] = M; objective[i] = the float64 mean of best over the assigned rows (NaN without any);
 * c_{i+1} = update(a_i, c_i).  Then assign = nearest(c_iters), score its best, objective[iters] its mean, counts its member counts: the
 * returned assign always belongs to the returned centroids.  Everything is enqueued without a host synchronisation.
 * Limits: 1 <= K <= 4096, M >= 1, Z >= 1, ld_x >= Z, ld_c >= Z.  Anything else, a NULL argument or op_bf16 outside {0, 1} is
 * CODAE_E_INVALID with the offending value in codae_last_error(), before any launch; the _ws_bytes queries return -1.
 * Neither entry is booked under a profiling kind: CODAE_K_COUNT stays as it is. */
int64_t codae_nearest_centroid_ws_bytes(int32_t Z, int32_t K, int32_t op_bf16);
int codae_nearest_centroid(const float* x, int64_t ld_x, int32_t M, int32_t Z, const float* c, int64_t ld_c, int32_t K, int32_t op_bf16,
                           const float* norm, int64_t* assign, float* best, void* ws, void* stream);
int64_t codae_centroid_update_ws_bytes(int32_t M, int32_t Z, int32_t K);
int codae_centroid_update(const float* x, int64_t ld_x, int32_t M, int32_t Z, const float* norm, const int64_t* assign, const float* c_in,
                          float* c_out, int64_t ld_c, int32_t K, int64_t* counts, void* ws, void* stream);

/* ---- State digest -------------------------------------------------------------------------------------------------------
 * A 128-bit fingerprint of a device buffer, computed on the device in one pass, and - with dst - a copy of the buffer made in that
 * same pass (the snapshot of a checkpoint: codae.train.HipEmbeddingTrainer.snapshot).  It verifies a loaded state where it lies and
 * lets data-parallel replicas be compared 16 bytes at a time.  It is NOT cryptographic: it detects accidents, not adversaries.
 * Definition.  The n_bytes of src (a multiple of 4) are read as little-endian uint32 words w_0 .. w_{n-1}, zero-padded to a multiple
 * of four words; all arithmetic is mod 2^64:
 *   G      = 0x9E3779B97F4A7C15
 *   mix(x) : z = x + G;  z = (z ^ z>>30) * 0xBF58476D1CE4E5B9;  z = (z ^ z>>27) * 0x94D049BB133111EB;  return z ^ z>>31
 *   group g = words 4g .. 4g+3:   a = w0 | w1<<32,   b = w2 | w3<<32,   h_g = mix(a ^ mix(b + g*G))
 *   out[0] = (sum_g h_g) ^ mix(n_bytes)          out[1] = xor_g mix(h_g ^ g)
 * Bitwise, not by value: -0.0 differs from +0.0 and NaN payloads count; positional: swapping two words changes it.  The empty buffer
 * has out = {mix(0), 0}.  codae.tool.checkpoint.StateDigest is the numpy restatement.
 * Order.  Sum and xor are associative and commutative, so the lanes, waves and workgroups combine in whatever order they finish and
 * the bits are the same every run: per-lane 64-bit accumulators, a wave64 butterfly, one 64-bit integer atomic add and xor per
 * workgroup into the zeroed out (a buffer one workgroup covers is finished by that workgroup, in one launch).  The training step's
 * "no float atomics" rule is untouched: these are integers.
 * Paths.  src (and dst) 16-byte aligned: one 16-byte load (and store) per group; 4-byte aligned only: four dword accesses per group,
 * same result.  The 1 .. 3 words behind the last whole group are padded in registers; nothing is read or written past n_bytes.  dst
 * (or NULL) must not overlap src.  out: two 64-bit words on the device, written on the stream; no host synchronisation.
 * CODAE_E_INVALID before any launch, with the offending value in codae_last_error(): n_bytes negative or not a multiple of 4, out
 * NULL, src NULL with n_bytes > 0, a pointer that is not 4-byte (out: 8-byte) aligned.  n_bytes == 0 is valid (src may be NULL). */
int codae_state_digest(const void* src, void* dst, int64_t n_bytes, uint64_t* out, void* stream);

/* ---- GEMM primitives (exported for kernel-level parity tests / benchmarks) - */
/* y[M][N] = act(x[M][K] . W[N][K]^T + b[N]), fp32 in / fp32 out (the parity engine's GEMM: CODAE_PREC_F32 above) */
int codae_linear_f32(const float* x, const float* W, const float* b, float* y, int32_t M, int32_t N,
                     int32_t K, int32_t relu, void* stream);
/* dx[M][K] = (dy[M][N] . W[N][K]) * [relu_src > 0]   (relu_src [M][K] or NULL) */
int codae_dgrad_f32(const float* dy, const float* W, const float* relu_src, float* dx, int32_t M,
                    int32_t N, int32_t K, void* stream);
/* dW[N][K] = dy[M][N]^T . x[M][K] ; db[N] = colsum(dy) (db may be NULL) */
int codae_wgrad_f32(const float* dy, const float* x, float* dW, float* db, int32_t M, int32_t N,
                    int32_t K, void* stream);
/* bf16 counterparts; x, W, dy, y, dx are bf16 (uint16 storage) unless noted.
 * y_f32 != 0 -> y is fp32. */
int codae_linear_bf16(const void* x, const void* W, const float* b, void* y, int32_t y_f32, int32_t M,
                      int32_t N, int32_t K, int32_t relu, void* stream);
/* db_prev (optional, [K]) = column sums of the stored dx; needs db_ws: ceil(M / 128) * K floats of scratch */
int codae_dgrad_bf16(const void* dy, const void* W, const void* relu_src, void* dx, float* db_prev, float* db_ws,
                     int32_t M, int32_t N, int32_t K, void* stream);
int codae_wgrad_bf16(const void* dy, const void* x, float* dW, void* slabs, int64_t slab_bytes,
                     int32_t M, int32_t N, int32_t K, void* stream);
/* The same forward / data-gradient GEMMs with any CODAE_ACT_* and its parameters (p0, p1, p2 as in codae_spec.act_param):
 * y = act(x . W^T + b); dx = (dy . W) * act'(act_src), act_src = the saved output of the activation (NULL: no factor).
 * act = NONE runs the plain kernels above; every other kind (RELU included) the generic-activation instantiations. */
int codae_linear_act_f32(const float* x, const float* W, const float* b, float* y, int32_t M, int32_t N, int32_t K,
                         int32_t act, float p0, float p1, float p2, void* stream);
int codae_dgrad_act_f32(const float* dy, const float* W, const float* act_src, float* dx, int32_t M, int32_t N, int32_t K,
                        int32_t act, float p0, float p1, float p2, void* stream);
int codae_linear_act_bf16(const void* x, const void* W, const float* b, void* y, int32_t y_f32, int32_t M, int32_t N,
                          int32_t K, int32_t act, float p0, float p1, float p2, void* stream);
int codae_dgrad_act_bf16(const void* dy, const void* W, const void* act_src, void* dx, float* db_prev, float* db_ws,
                         int32_t M, int32_t N, int32_t K, int32_t act, float p0, float p1, float p2, void* stream);
/* Host-only query (no HIP call, no device needed): which kernel a bf16 GEMM launch with these descriptor facts takes under the
 * CODAE_* variables as last read, and the counts the engine derives from that choice.  It pins the dispatch in tests.
 *   desc[13]: a_mode, b_mode (0 = k contiguous, 1 = k strided), c_f32, M, N, K, split_k, act (CODAE_ACT_*), fused loss on / off,
 *             backward epilogue (mask source or column sums) yes / no, coscheduled, store_policy (0 plain, 1 write-through,
 *             -1 by the output's size as the engine sets it), ldc
 *   out[CODAE_GEMM_PLAN_FIELDS]: family (0 one-barrier kernel, 1 phase-pipelined), bm, bn, stages
 *             (one-barrier: 2 / 4), loader layout (pipelined: 1 / 6 = 256 x 192 with every wave / one wave per SIMD loading,
 *             7 = 128 x 192), epilogue (1 forward, 2 backward, 3 fused loss, 0 fp32 output or one-barrier kernel), phase schedule (0 pinned, 64 the
 *             compiler's), generic-activation instantiation, effective store policy, tiles_m,
 *             tiles_n, workgroups, colsum_rows, loss_parts (0 without the fused loss), takes_relu_bits (of an M x N forward-form
 *             launch)
 * capacity: room in out, >= CODAE_GEMM_PLAN_FIELDS. */
#define CODAE_GEMM_PLAN_FIELDS 15
int codae_debug_gemm_bf16_plan(const int32_t* desc, int32_t* out, int32_t capacity);
/* One bf16 GEMM launch with the operand modes and leading dimensions spelled out (kernel-level tests of the operand staging; the
 * entries above fix them per role): C[M][N] = A . B^T (+ bias, ReLU).  a_mode / b_mode 0 = k contiguous (A [M][lda], B [N][ldb]),
 * 1 = k strided (A [K][lda], B [K][ldb]); ld* in elements.  c_f32 != 0: fp32 C, no bias, no ReLU; split_k > 1 then writes split_k
 * partial products, M * ldc floats apart, for the caller to add up.  The kernel is the one gemm_bf16's plan picks under the CODAE_*
 * variables as last read; the descriptor passes the same validation as every other launch. */
int codae_debug_gemm_bf16(const void* A, int64_t lda, int32_t a_mode, const void* B, int64_t ldb, int32_t b_mode, void* C, int64_t ldc,
                          int32_t c_f32, int32_t M, int32_t N, int32_t K, int32_t split_k, const float* bias, int32_t relu, void* stream);
int codae_cast_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream);
/* The image form of the plain gather on its own (the launcher the engine uses): out[b][:] = mask(image[row_idx[b]][:]) in bf16, rows
 * out_ld elements apart (<= 0: io), bit for bit what codae_corrupt_batch_present(batch, NULL, ..., out_bf16 = 1) writes when image =
 * codae_cast_f32_to_bf16(batch->data).  batch->data is not read.  present NULL: no presence table.  CODAE_E_INVALID unless io and
 * out_ld are multiples of 8, image and out 16-byte and the mask table 8-byte aligned. */
int codae_corrupt_batch_image(const codae_batch* batch, const void* image_bf16, const uint8_t* present, int32_t n_slots, void* out,
                              int64_t out_ld, void* stream);
/* dst[c][r] = src[r][c] on bf16 matrices (rows, cols multiples of 8): the kernel that refreshes codae_buffers.shadow_wt
 * after an EXTERNAL parameter update (codae_sync_shadows); codae_step_update writes it inside its Adam pass
 * (W.t() in torch.nn.Linear's data gradient, embedding_denoising_autoencoder.py:137-151). */
int codae_transpose_bf16(const void* src, void* dst, int32_t rows, int32_t cols, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CODAE_HIP_H */
