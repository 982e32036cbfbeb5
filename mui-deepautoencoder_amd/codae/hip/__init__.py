"""ctypes binding of libcodae_hip.so (include/codae_hip.h).

The shared object is built in-tree by `__graft_entry__.build()` /
`make -C mui-deepautoencoder_amd/csrc`.  There is no CPU fallback: if the
library is missing, every compute entry point of the package raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# CODAE_HIP_LIB: load another build of the library (same-box A/B of kernel variants)
LIB_PATH = os.environ.get("CODAE_HIP_LIB") or os.path.join(_HERE, "libcodae_hip.so")

PREC_F32 = 0
PREC_BF16 = 1

ABI_VERSION = 11
# CODAE_S_* of include/codae_hip.h (tests/test_host_logic.py parses the header and compares)
S_SQ_FULL, S_SQ_PARTIAL, S_GRAD_SQ, S_LAST_LOSS, S_STEP_SQ, S_CLIP_COEF = 0, 1, 2, 3, 4, 5
S_GRAD_SQ_SLOTS, S_N_SLOTS, S_ADAM_STEP, S_COUNT = 8, 64, 72, 80
# CODAE_ACT_* of include/codae_hip.h: the activation after a Linear (codae.model.activation maps torch modules to these)
ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_RELU6, ACT_ELU, ACT_SOFTPLUS, ACT_HARDSIGMOID = 0, 1, 2, 3, 4, 5, 6
# CODAE_NOISE_* of include/codae_hip.h: the input noise of the training steps (codae.tool.InputNoise builds the struct)
NOISE_NONE, NOISE_GAUSSIAN, NOISE_MASKING, NOISE_SALT_PEPPER, NOISE_SWAP = 0, 1, 2, 3, 4
# CODAE_LOSS_* of include/codae_hip.h: the training criterion (codae.tool.ReconstructionLoss builds the struct)
LOSS_MSE, LOSS_L1, LOSS_SMOOTH_L1, LOSS_HUBER, LOSS_SLOT_COSINE = 0, 1, 2, 3, 4
# CODAE_VAR_* of include/codae_hip.h: the type of a variable of the mixed-variable criterion (codae.tool.VariableLoss builds the struct)
VAR_REGRESSION, VAR_CLASSIFICATION, VAR_MAX = 0, 1, 65536
# CODAE_OPT_* / CODAE_SCHED_* of include/codae_hip.h: the update's optimizer and schedule (codae.tool.Optimizer builds the struct)
OPT_ADAM, OPT_ADAMW, OPT_SGD, OPT_LAMB, OPT_LARS = 0, 1, 2, 3, 4
# the work space of the trust kinds: CODAE_TRUST_MAX_MATRICES fp32 ratios at its head, a partial pair per CODAE_TRUST_CHUNK elements
TRUST_MAX_MATRICES, TRUST_CHUNK = 64, 4096
SCHED_CONSTANT, SCHED_COSINE, SCHED_LINEAR, SCHED_STEP = 0, 1, 2, 3
# CODAE_AVG_* of include/codae_hip.h: the average of the iterates the update keeps (codae.tool.WeightAverage builds the struct)
AVG_OFF, AVG_EMA, AVG_SWA = 0, 1, 2
# CODAE_RM_* of include/codae_hip.h: the fields of one slot's block of retrieval-metric sums (codae.tool.RetrievalMetrics reads them)
RM_PAIRS, RM_RRE, RM_RR, RM_HIT, RM_MAX_KS, RM_HIST, RM_STRIDE = 0, 1, 2, 3, 8, 16, 48
# CODAE_AUC_* of include/codae_hip.h: the fields of one slot's row of AUC counts (codae.tool.Compatibility reads them)
AUC_WINS, AUC_TIES, AUC_PAIRS, AUC_PAIRED, AUC_STRIDE = 0, 1, 2, 3, 4
KERNEL_CLASSES = ("gemm_fwd", "gemm_dgrad", "gemm_wgrad", "loss", "gather", "sumsq", "adam", "slab_reduce", "chain",
                  "bias_finish", "dropout")


class HipError(RuntimeError):
    pass


class Spec(C.Structure):
    _fields_ = [("n_layers", C.c_int32),
                ("in_features", C.POINTER(C.c_int32)),
                ("out_features", C.POINTER(C.c_int32)),
                ("relu", C.POINTER(C.c_uint8)),
                ("max_batch", C.c_int32),
                ("precision", C.c_int32),
                ("act_kind", C.POINTER(C.c_uint8)),
                ("act_param", C.POINTER(C.c_float))]


class Sizes(C.Structure):
    _fields_ = [("n_param", C.c_int64), ("n_weight", C.c_int64), ("act_bytes", C.c_int64),
                ("dact_bytes", C.c_int64), ("slab_bytes", C.c_int64), ("bias_part_bytes", C.c_int64),
                ("n_scalars", C.c_int32)]


class Buffers(C.Structure):
    _fields_ = [("params", C.c_void_p), ("grads", C.c_void_p), ("adam_m", C.c_void_p),
                ("adam_v", C.c_void_p), ("shadow_w", C.c_void_p), ("acts", C.c_void_p),
                ("dacts", C.c_void_p), ("slabs", C.c_void_p), ("scalars", C.c_void_p), ("shadow_wt", C.c_void_p),
                ("bias_parts", C.c_void_p)]


class Batch(C.Structure):
    _fields_ = [("data", C.c_void_p), ("row_idx", C.c_void_p), ("mask_id", C.c_void_p),
                ("mask_table", C.c_void_p), ("B", C.c_int32), ("io", C.c_int32),
                ("mask_to_use", C.c_void_p), ("nb_run", C.c_int32), ("run", C.c_int32)]


class Hyper(C.Structure):
    _fields_ = [("lr", C.c_float), ("weight_decay", C.c_float), ("beta1", C.c_float),
                ("beta2", C.c_float), ("eps", C.c_float), ("max_grad_norm", C.c_float),
                ("step", C.c_int32), ("loss_scale_rows", C.c_float)]


class Noise(C.Structure):
    _fields_ = [("kind", C.c_int32), ("p0", C.c_float), ("p1", C.c_float), ("p2", C.c_float), ("seed", C.c_uint64)]


# codae_swap: the pool and the slot count of swap noise: a pointer and two 4-byte fields, 16 bytes
class Swap(C.Structure):
    _fields_ = [("pool", C.c_void_p), ("n_pool", C.c_int32), ("n_slots", C.c_int32)]


class Emphasis(C.Structure):
    _fields_ = [("alpha", C.c_float), ("beta", C.c_float), ("col_weight", C.c_void_p)]


class ReconLoss(C.Structure):
    _fields_ = [("kind", C.c_int32), ("param", C.c_float), ("mse_weight", C.c_float), ("n_slots", C.c_int32)]


# codae_variable_loss: two 4-byte fields, four host arrays, the device work space and its size: 56 bytes
class VariableLossStruct(C.Structure):
    _fields_ = [("n_var", C.c_int32), ("reserved", C.c_int32), ("position", C.POINTER(C.c_int32)), ("size", C.POINTER(C.c_int32)),
                ("type", C.POINTER(C.c_int32)), ("weight", C.POINTER(C.c_float)), ("ws", C.c_void_p), ("ws_bytes", C.c_int64)]


class SlotContrast(C.Structure):
    _fields_ = [("n_slots", C.c_int32), ("n_neg", C.c_int32), ("tau", C.c_float), ("weight", C.c_float), ("seed", C.c_uint64),
                ("n_rows", C.c_int32), ("n_pool", C.c_int32), ("ws_bytes", C.c_int64), ("pool", C.c_void_p),
                ("item_id", C.c_void_p), ("ws", C.c_void_p)]


class Optimizer(C.Structure):
    _fields_ = [("kind", C.c_int32), ("amsgrad", C.c_int32), ("momentum", C.c_float), ("nesterov", C.c_int32), ("sched", C.c_int32),
                ("warmup", C.c_int32), ("total", C.c_int32), ("period", C.c_int32), ("min_factor", C.c_float), ("gamma", C.c_float),
                ("vmax", C.c_void_p),
                # LAMB / LARS, appended: 48 -> 72 bytes (four bytes of padding in front of trust_ws); a struct built from the first
                # eleven values alone has them zero
                ("trust_clip", C.c_float), ("trust_coef", C.c_float), ("decay_bias", C.c_int32), ("trust_ws", C.c_void_p)]


# codae_weight_average: five 4-byte fields, four bytes of padding, the pointer: 32 bytes (tests/test_weight_average_host.py)
class WeightAverage(C.Structure):
    _fields_ = [("kind", C.c_int32), ("decay", C.c_float), ("debias", C.c_int32), ("start", C.c_int32), ("every", C.c_int32),
                ("avg", C.c_void_p)]


# codae_tie_pair.  Like every struct added since ABI 8 (Noise, Emphasis, ReconLoss, SlotContrast, Optimizer, Dropout) it is not in
# codae_struct_sizes(), whose seven entries are fixed (tests pin them): four fixed-width fields without padding, 24 bytes, pinned
# by tests/test_tied_host.py.
class TiePair(C.Structure):
    _fields_ = [("enc_off", C.c_int64), ("dec_off", C.c_int64), ("rows", C.c_int32), ("cols", C.c_int32)]


class Dropout(C.Structure):
    _fields_ = [("p", C.POINTER(C.c_float)), ("n", C.c_int32), ("seed", C.c_uint64)]


class ResidualFlags(C.Structure):
    """codae_residual: n == n_layers, on[l] != 0 = a skip around layer l (a host array the setter copies)"""
    _fields_ = [("n", C.c_int32), ("on", C.POINTER(C.c_uint8))]


class NormFlags(C.Structure):
    """codae_norm: n == n_layers, on[l] != 0 = layer l's output is normalised (a host array the setter copies), kind = CODAE_NORM_LAYER
    (1) or CODAE_NORM_RMS (2), eps > 0"""
    _fields_ = [("n", C.c_int32), ("on", C.POINTER(C.c_uint8)), ("kind", C.c_int32), ("eps", C.c_float)]


class SparseCodeCfg(C.Structure):
    """codae_sparse_code: layer = the Linear that reads the code (1 .. n_layers - 1), keep = the units kept per row (Z = off)"""
    _fields_ = [("layer", C.c_int32), ("keep", C.c_int32)]


_P, _I32, _I64, _F = C.c_void_p, C.c_int32, C.c_int64, C.c_float

# name -> (restype, argtypes); mirrors include/codae_hip.h one to one
PROTOTYPES = {
    "codae_last_error": (C.c_char_p, []),
    "codae_abi_version": (C.c_int, []),
    "codae_struct_sizes": (C.c_int, [C.POINTER(C.c_int32), _I32]),
    "codae_reload_env": (C.c_int, []),
    "codae_create": (C.c_int, [C.POINTER(Spec), C.POINTER(_P)]),
    "codae_destroy": (C.c_int, [_P]),
    "codae_get_sizes": (C.c_int, [_P, C.POINTER(Sizes)]),
    "codae_param_offsets": (C.c_int, [_P, _I32, C.POINTER(_I64), C.POINTER(_I64), C.POINTER(_I64)]),
    "codae_forward": (C.c_int, [_P, C.POINTER(Buffers), _P, _P, _I32, _I32, _I32, _I32, _P]),
    "codae_backward": (C.c_int, [_P, C.POINTER(Buffers), _P, _P, _I32, _I32, _I32, _P]),
    "codae_sync_shadows": (C.c_int, [_P, C.POINTER(Buffers), _P]),
    "codae_step_forward_loss": (C.c_int, [_P, C.POINTER(Buffers), C.POINTER(Batch), C.POINTER(Hyper), _P, _P]),
    "codae_step_backward": (C.c_int, [_P, C.POINTER(Buffers), _I32, _I32, _I32, _P]),
    "codae_step_update": (C.c_int, [_P, C.POINTER(Buffers), C.POINTER(Hyper), _P]),
    "codae_step_backward_async": (C.c_int, [_P, C.POINTER(Buffers), _I32, _I32, _I32, _P]),
    "codae_side_stream": (C.c_int, [_P, C.POINTER(C.c_void_p)]),
    "codae_profile_stride": (C.c_int, [_P, _I32]),
    "codae_join": (C.c_int, [_P, _P]),
    "codae_span_sumsq": (C.c_int, [_P, _I64, _P, _P]),
    "codae_step_update_span": (C.c_int, [_P, C.POINTER(Buffers), C.POINTER(Hyper), _I64, _I64, _P, _P]),
    "codae_sync_transposed": (C.c_int, [_P, C.POINTER(Buffers), _P]),
    "codae_train_step": (C.c_int, [_P, C.POINTER(Buffers), C.POINTER(Batch), C.POINTER(Hyper), _P]),
    "codae_train_step_graph": (C.c_int, [_P, C.POINTER(Buffers), C.POINTER(Batch), C.POINTER(Hyper), _P]),
    "codae_set_input_noise": (C.c_int, [_P, C.POINTER(Noise)]),
    "codae_set_swap_pool": (C.c_int, [_P, _P, _I32, _I32]),
    "codae_corrupt_batch_swap": (C.c_int, [C.POINTER(Batch), C.POINTER(Noise), _I32, _P, _P, C.POINTER(Swap), _P, _I32, _I64, _P, _I32, _P]),
    "codae_emph_loss_swap": (C.c_int, [C.POINTER(Batch), C.POINTER(Noise), _I32, C.POINTER(Emphasis), _P, _P, _I32, _I64, _F, _P, _P,
                                       C.POINTER(Swap), _P, _I32, _P]),
    "codae_recon_loss_fwd_bwd_swap": (C.c_int, [C.POINTER(Batch), C.POINTER(Noise), _I32, C.POINTER(Emphasis), C.POINTER(ReconLoss), _P, _P,
                                                _I32, _I64, _F, _P, _P, C.POINTER(Swap), _P, _I32, _P]),
    "codae_set_loss_emphasis": (C.c_int, [_P, C.POINTER(Emphasis)]),
    "codae_set_recon_loss": (C.c_int, [_P, C.POINTER(ReconLoss)]),
    "codae_set_variable_loss": (C.c_int, [_P, C.POINTER(VariableLossStruct)]),
    "codae_variable_loss_ws_bytes": (_I64, [_I32, _I32]),
    "codae_variable_loss_blocks": (C.c_int, [_I32]),
    "codae_variable_loss_fwd_bwd": (C.c_int, [C.POINTER(Batch), C.POINTER(VariableLossStruct), _P, _P, _I32, _I64, _P, _P, _P]),
    "codae_set_hidden_dropout": (C.c_int, [_P, C.POINTER(Dropout)]),
    "codae_set_slot_contrast": (C.c_int, [_P, C.POINTER(SlotContrast)]),
    "codae_set_optimizer": (C.c_int, [_P, C.POINTER(Optimizer)]),
    "codae_optimizer_update": (C.c_int, [_P, _P, _P, _P, _P, _I64, C.POINTER(Hyper), C.POINTER(Optimizer), _P, _P]),
    "codae_trust_ws_bytes": (_I64, [_P]),
    "codae_trust_ws_bytes_flat": (_I64, [_I64]),
    "codae_trust_update": (C.c_int, [_P, _P, _P, _P, _I64, C.POINTER(Hyper), C.POINTER(Optimizer), _P, _P, _I64, _P]),
    "codae_graph_captures": (C.c_int, [_P]),
    "codae_set_weight_average": (C.c_int, [_P, C.POINTER(WeightAverage)]),
    "codae_weight_average_update": (C.c_int, [_P, _P, _I64, C.POINTER(WeightAverage), _I32, _P]),
    "codae_set_tied_weights": (C.c_int, [_P, _I32]),
    "codae_tie_fold": (C.c_int, [_P, C.POINTER(TiePair), _I32, _P]),
    "codae_tie_mirror": (C.c_int, [_P, _P, _P, C.POINTER(TiePair), _I32, _P]),
    "codae_set_slot_presence": (C.c_int, [_P, _P, _I64, _I32]),
    "codae_set_dataset_image": (C.c_int, [_P, _P, _P, _I64, _I32]),
    "codae_corrupt_batch_present": (C.c_int, [C.POINTER(Batch), C.POINTER(Noise), _I32, _P, _P, _I32, _I64, _P, _I32, _P]),
    "codae_mse_loss_present": (C.c_int, [C.POINTER(Batch), _P, _P, _I32, _I64, _F, _P, _P, _P, _I32, _P]),
    "codae_emph_loss_present": (C.c_int, [C.POINTER(Batch), C.POINTER(Noise), _I32, C.POINTER(Emphasis), _P, _P, _I32, _I64, _F, _P, _P,
                                          _P, _I32, _P]),
    "codae_recon_loss_fwd_bwd_present": (C.c_int, [C.POINTER(Batch), C.POINTER(Noise), _I32, C.POINTER(Emphasis), C.POINTER(ReconLoss), _P,
                                                   _P, _I32, _I64, _F, _P, _P, _P, _I32, _P]),
    "codae_slot_contrast_prepare_present": (C.c_int, [_P, _I32, C.POINTER(SlotContrast), _I32, _I32, _P, _I32, _P]),
    "codae_slot_contrast_fwd_bwd_present": (C.c_int, [C.POINTER(Batch), C.POINTER(Noise), _I32, C.POINTER(Emphasis),
                                                      C.POINTER(SlotContrast), _P, _P, _I32, _I64, _F, _P, _P, _P, _I32, _P]),
    "codae_slot_contrast_ws_bytes": (_I64, [_I32, _I32, _I32, _I32]),
    "codae_slot_contrast_prepare": (C.c_int, [_P, _I32, C.POINTER(SlotContrast), _I32, _I32, _P]),
    "codae_slot_contrast_fwd_bwd": (C.c_int, [C.POINTER(Batch), C.POINTER(Noise), _I32, C.POINTER(Emphasis), C.POINTER(SlotContrast), _P, _P,
                                              _I32, _I64, _F, _P, _P, _P]),
    "codae_slot_contrast_blocks": (C.c_int, [_I32]),
    "codae_dropout_fwd": (C.c_int, [_P, _I32, _I64, _I32, _I32, _P, _I32, _I32, _F, C.c_uint64, _P]),
    "codae_dropout_bwd": (C.c_int, [_P, _I32, _I64, _I32, _I32, _P, _I32, _I32, _F, C.c_uint64, _P, _P]),
    "codae_dropout_blocks": (C.c_int, [_I32]),
    "codae_residual_ws_bytes": (_I64, [_P, C.POINTER(ResidualFlags)]),
    "codae_set_residual": (C.c_int, [_P, C.POINTER(ResidualFlags), _P, _I64]),
    "codae_residual_fwd": (C.c_int, [_P, _P, _I32, _I64, _I64, _I32, _I32, _P, _I64, _P]),
    "codae_residual_bwd": (C.c_int, [_P, _I32, _I64, _I32, _I32, _P, _P, _I64, _P, _I64, _P, _I64, _I32, _P, _P, _P]),
    "codae_residual_blocks": (C.c_int, [_I32]),
    "codae_norm_ws_bytes": (_I64, [_P, C.POINTER(NormFlags)]),
    "codae_set_norm": (C.c_int, [_P, C.POINTER(NormFlags), _P, _I64]),
    "codae_norm_fwd": (C.c_int, [_P, _I32, _I64, _I32, _I32, _I32, _F, _P, _P, _I64, _P]),
    "codae_norm_bwd": (C.c_int, [_P, _I32, _I64, _I32, _I32, _I32, _P, _I64, _P, _P, _P, _I64, _P, _I64, _I32, _P, _P, _P]),
    "codae_norm_blocks": (C.c_int, [_I32]),
    "codae_sparse_code_ws_bytes": (_I64, [_P, C.POINTER(SparseCodeCfg)]),
    "codae_set_sparse_code": (C.c_int, [_P, C.POINTER(SparseCodeCfg), _P, _I64]),
    "codae_sparse_code_fwd": (C.c_int, [_P, _I32, _I64, _I32, _I32, _I32, _P, _I64, _P]),
    "codae_sparse_code_bwd": (C.c_int, [_P, _I32, _I64, _I32, _I32, _P, _I64, _P, _P]),
    "codae_sparse_code_blocks": (C.c_int, [_I32]),
    "codae_emph_loss": (C.c_int, [C.POINTER(Batch), C.POINTER(Noise), _I32, C.POINTER(Emphasis), _P, _P, _I32, _I64, _F, _P, _P, _P]),
    "codae_emph_loss_blocks": (C.c_int, [_I32]),
    "codae_recon_loss_fwd_bwd": (C.c_int, [C.POINTER(Batch), C.POINTER(Noise), _I32, C.POINTER(Emphasis), C.POINTER(ReconLoss), _P, _P, _I32, _I64,
                                           _F, _P, _P, _P]),
    "codae_recon_loss_blocks": (C.c_int, [_I32]),
    "codae_corrupt_batch": (C.c_int, [C.POINTER(Batch), C.POINTER(Noise), _I32, _P, _P, _I32, _I64, _P]),
    "codae_noise_box_muller": (C.c_int, [_P, _P, _P, _P, _P, _I64, _P]),
    "codae_eval_step": (C.c_int, [_P, C.POINTER(Buffers), C.POINTER(Batch), _P, _P]),
    "codae_profile_begin": (C.c_int, [_P, C.c_uint32, _I32]),
    "codae_profile_end": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_float), _I32, C.POINTER(C.c_int32)]),
    "codae_corrupt": (C.c_int, [_P, _P, _P, _I64, _P]),
    "codae_expand_masks": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, _P, _P, _P]),
    "codae_mse_loss_fwd_bwd": (C.c_int, [_P, _P, _P, _P, _I64, _F, _P, _P]),
    "codae_clip_adam": (C.c_int, [_P, _P, _P, _P, _I64, C.POINTER(Hyper), _P, _P]),
    "codae_combined_loss_fwd_bwd": (C.c_int, [_P, _P, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P, _P]),
    "codae_combined_loss_full": (C.c_int, [_P, _P, _I32, _I32, _I32, _P, _P, _P, _P, _P]),
    "codae_row_norms": (C.c_int, [_P, _I64, _I32, _P, _P]),
    "codae_ranking_loss": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, _I32, _P, _P, _I64, _P, _I32, _P, _P]),
    "codae_ranking_loss_batched": (C.c_int, [_P, _I32, _I32, _I32, _I32, _P, _P, _P, _I32, _I32, _P, _P, _P, _I64, _P, _P, _P, _P, _I32, _P,
                                             _I32, _P, _P, _P, _P, _P]),
    "codae_dp_unique_id": (C.c_int, [_P, _I32]),
    "codae_dp_init": (C.c_int, [_P, _P, _I32, _I32]),
    "codae_dp_destroy": (C.c_int, [_P]),
    "codae_train_step_dp": (C.c_int, [_P, C.POINTER(Buffers), C.POINTER(Batch), C.POINTER(Hyper), _I32, _P, _P, _P]),
    "codae_monitor_accumulate": (C.c_int, [_P, _P, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _P, _P]),
    "codae_gather_inventory_rows": (C.c_int, [_P, _I64, _I32, _I32, _P, _I32, _P, _P]),
    "codae_topk_init": (C.c_int, [_P, _I32, _I32, _P]),
    "codae_topk_merge": (C.c_int, [_P, _I64, _I32, _I32, _I32, _I32, _P, _P, _P, _P]),
    "codae_topk_finish": (C.c_int, [_P, _I32, _I32, _P, _P, _P, _P]),
    "codae_complete_topk": (C.c_int, [_P, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _I32, _I32, _P, _P, _P, _P, _I32, _P, _P, _P, _I64,
                                      _I32, _P, _I32, _P, _P, _P, _P, _P, _P, _P]),
    "codae_retrieval_metrics_batched": (C.c_int, [_P, _I32, _I32, _I32, _I32, _P, _P, _P, _I32, _I32, _P, _P, _P, _P, _I64, _P, _P, _I32, _P,
                                                  _P, _P, _I32, _P, _I32, _P, _P, _P, _P, _P]),
    "codae_assemble_outfits": (C.c_int, [_P, _I32, _I64, _I32, _I32, _P, _I32, _P, _I32, _P, _P, _I32, _I64, _P]),
    "codae_outfit_scores": (C.c_int, [_P, _I64, _I32, _I32, _P, _I32, _P, _P, _I64, _P, _P, _P, _P, _P]),
    "codae_auc_blocks": (C.c_int, [_I32]),
    "codae_auc_counts": (C.c_int, [_P, _P, _I32, _P, _P, _P, _I32, _I32, _P, _P, _P]),
    "codae_score_outfits": (C.c_int, [_P, C.POINTER(Buffers), _P, _I64, _P, _I32, _I32, _P, _P, _P, _P, _P]),
    "codae_export_rows": (C.c_int, [_P, _I32, _I64, _I32, _I32, _P, _I64, _P, _P]),
    "codae_encode": (C.c_int, [_P, C.POINTER(Buffers), _P, _I32, _I32, _P, _P, _P]),
    "codae_decode": (C.c_int, [_P, C.POINTER(Buffers), _P, _I32, _I32, _P, _P]),
    "codae_nearest_centroid_ws_bytes": (_I64, [_I32, _I32, _I32]),
    "codae_nearest_centroid": (C.c_int, [_P, _I64, _I32, _I32, _P, _I64, _I32, _I32, _P, _P, _P, _P, _P]),
    "codae_centroid_update_ws_bytes": (_I64, [_I32, _I32, _I32]),
    "codae_centroid_update": (C.c_int, [_P, _I64, _I32, _I32, _P, _P, _P, _P, _I64, _I32, _P, _P, _P]),
    "codae_state_digest": (C.c_int, [_P, _P, _I64, _P, _P]),
    "codae_step_path": (C.c_int, [_P, _P, _I32]),
    "codae_step_stores_output": (C.c_int, [_P, _P, _I32]),
    "codae_debug_step_plan": (C.c_int, [_P, C.POINTER(Buffers), _P, _P, _I32]),
    "codae_linear_f32": (C.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _P]),
    "codae_dgrad_f32": (C.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, _P]),
    "codae_wgrad_f32": (C.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, _P]),
    "codae_linear_bf16": (C.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P]),
    "codae_dgrad_bf16": (C.c_int, [_P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _P]),
    "codae_wgrad_bf16": (C.c_int, [_P, _P, _P, _P, _I64, _I32, _I32, _I32, _P]),
    "codae_linear_act_f32": (C.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _F, _F, _F, _P]),
    "codae_dgrad_act_f32": (C.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _F, _F, _F, _P]),
    "codae_linear_act_bf16": (C.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _F, _F, _F, _P]),
    "codae_dgrad_act_bf16": (C.c_int, [_P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _F, _F, _F, _P]),
    "codae_cast_f32_to_bf16": (C.c_int, [_P, _P, _I64, _P]),
    "codae_corrupt_batch_image": (C.c_int, [C.POINTER(Batch), _P, _P, _I32, _P, _I64, _P]),
    "codae_debug_gemm_bf16_plan": (C.c_int, [_P, _P, _I32]),
    "codae_debug_gemm_bf16": (C.c_int, [_P, _I64, _I32, _P, _I64, _I32, _P, _I64, _I32, _I32, _I32, _I32, _I32, _P, _I32, _P]),
    "codae_transpose_bf16": (C.c_int, [_P, _P, _I32, _I32, _P]),
}

_lib = None


def lib():
    """Load libcodae_hip.so (once).  Raises HipError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipError(
            "libcodae_hip.so is missing (%s). Build it with `python -c \"import __graft_entry__ as g; "
            "g.build()\"` or `make -C mui-deepautoencoder_amd/csrc`. There is no CPU fallback." % LIB_PATH)
    import torch  # noqa: F401  -- loads the HIP runtime this library must share with torch
    handle = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(handle, name)
        fn.restype = res
        fn.argtypes = args
    if handle.codae_abi_version() != ABI_VERSION:
        raise HipError("libcodae_hip.so ABI version %d, this binding is written for %d: rebuild the library"
                       % (handle.codae_abi_version(), ABI_VERSION))
    check_struct_sizes(handle)
    _lib = handle
    return _lib


def struct_sizes_expected():
    """What this binding declares, in codae_struct_sizes() order."""
    return [C.sizeof(Spec), C.sizeof(Sizes), C.sizeof(Buffers), C.sizeof(Batch), C.sizeof(Hyper), S_COUNT,
            len(KERNEL_CLASSES)]


def check_struct_sizes(handle):
    """A ctypes struct shorter than the library's makes the engine read past the caller's memory
    (codae_buffers gained shadow_wt in ABI 2): compare every layout before the first call."""
    n = 7
    got = (C.c_int32 * n)()
    rc = handle.codae_struct_sizes(got, n)
    if rc != 0:
        raise HipError("codae_struct_sizes failed (%d)" % rc)
    want = struct_sizes_expected()
    names = ("codae_spec", "codae_sizes", "codae_buffers", "codae_batch", "codae_hyper", "CODAE_S_COUNT", "CODAE_K_COUNT")
    bad = ["%s: library %d, binding %d" % (nm, g, w) for nm, g, w in zip(names, list(got), want) if g != w]
    if bad:
        raise HipError("libcodae_hip.so and its ctypes binding disagree: " + "; ".join(bad))


def check(rc):
    if rc != 0:
        msg = lib().codae_last_error()
        raise HipError("codae_hip error %d: %s" % (rc, msg.decode() if msg else "?"))


def ptr(t):
    """data pointer of a torch tensor (or None)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def current_stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
