"""Python owner of one codae_handle and of the device buffers it borrows.

torch is used here for what the boundary allows: allocating device memory and
naming the current HIP stream.  All arithmetic happens in libcodae_hip.so.
"""
import ctypes as C

import torch

from . import (PREC_BF16, PREC_F32, S_COUNT, S_GRAD_SQ, S_GRAD_SQ_SLOTS, S_LAST_LOSS, S_N_SLOTS, S_SQ_FULL, S_SQ_PARTIAL,
               Batch, Buffers, Dropout, Emphasis,
               HipError, Hyper, Sizes, Spec, TiePair, WeightAverage, check, current_stream, lib, ptr)


def precision_code(precision):
    if precision in (PREC_F32, "f32", "fp32", "parity"):
        return PREC_F32
    if precision in (PREC_BF16, "bf16", "throughput"):
        return PREC_BF16
    raise ValueError("unknown precision %r (use 'f32' or 'bf16')" % (precision,))


def _tie_pair_array(pairs):
    """pairs: [(enc_off, dec_off, rows, cols)] -> a ctypes array of codae_tie_pair."""
    arr = (TiePair * max(len(pairs), 1))()
    for i, (e, d, r, c) in enumerate(pairs):
        arr[i] = TiePair(int(e), int(d), int(r), int(c))
    return arr


def tie_fold(grads, pairs):
    """codae_tie_fold on a flat fp32 device tensor, in place: for every (enc_off, dec_off, rows, cols) the decoder range, read as
    [cols][rows], is added transposed onto the encoder range [rows][cols] and left +0."""
    if grads.dtype != torch.float32 or not grads.is_cuda or not grads.is_contiguous():
        raise HipError("tie_fold: grads must be a contiguous fp32 tensor on a HIP device")
    with torch.cuda.device(grads.device):
        check(lib().codae_tie_fold(ptr(grads), _tie_pair_array(pairs), len(pairs), current_stream()))
    return grads


def tie_mirror(params, pairs, shadow=None, shadow_t=None):
    """codae_tie_mirror on a flat fp32 device tensor, in place: every decoder range becomes the transpose of its encoder range;
    shadow / shadow_t (flat bf16 tensors in the parameter layout, optional) get the decoder's bf16 shadow and transposed shadow."""
    if params.dtype != torch.float32 or not params.is_cuda or not params.is_contiguous():
        raise HipError("tie_mirror: params must be a contiguous fp32 tensor on a HIP device")
    for t in (shadow, shadow_t):
        if t is not None and (t.dtype != torch.bfloat16 or t.device != params.device or not t.is_contiguous()):
            raise HipError("tie_mirror: the shadows must be contiguous bf16 tensors on %s" % params.device)
    with torch.cuda.device(params.device):
        check(lib().codae_tie_mirror(ptr(params), ptr(shadow), ptr(shadow_t), _tie_pair_array(pairs), len(pairs), current_stream()))
    return params


class DaeEngine:
    """Handle + flat parameter / gradient / Adam / workspace buffers on one HIP device.

    schedule: list of (in_features, out_features, relu_after) per Linear, as built by
    the model classes (embedding_denoising_autoencoder.py:49-129 of the reference).
    """

    def __init__(self, schedule, max_batch, precision, device, with_optimizer_state=True, activation=None):
        """activation: None = ReLU after every layer whose schedule flag is set (as always); else what follows those
        layers instead - an activation factory called as activation(True) (the model classes' convention), or a
        (CODAE_ACT_* kind, p0, p1, p2) tuple, or one such tuple per layer (the flags are then ignored)."""
        device = torch.device(device)
        if device.type != "cuda":
            raise HipError("the codae HIP engine needs a HIP device (got %s); there is no CPU path" % device)
        self._lib = lib()
        self.device = device
        self.schedule = [(int(a), int(b), bool(r)) for a, b, r in schedule]
        self.L = len(self.schedule)
        self.max_batch = int(max_batch)
        self.precision = precision_code(precision)
        ins = (C.c_int32 * self.L)(*[s[0] for s in self.schedule])
        outs = (C.c_int32 * self.L)(*[s[1] for s in self.schedule])
        relu = (C.c_uint8 * self.L)(*[1 if s[2] else 0 for s in self.schedule])
        self.activation = self._layer_acts(activation)
        spec = Spec(self.L, ins, outs, relu, self.max_batch, self.precision)
        if self.activation is not None:
            spec.act_kind = (C.c_uint8 * self.L)(*[a[0] for a in self.activation])
            spec.act_param = (C.c_float * (3 * self.L))(*[float(p) for a in self.activation for p in a[1:]])
        h = C.c_void_p()
        check(self._lib.codae_create(C.byref(spec), C.byref(h)))
        self._h = h
        sz = Sizes()
        check(self._lib.codae_get_sizes(self._h, C.byref(sz)))
        self.n_param = int(sz.n_param)
        with torch.cuda.device(device):
            f32 = dict(dtype=torch.float32, device=device)
            self._params = torch.zeros(self.n_param, **f32)
            self.grads = torch.zeros(self.n_param, **f32)
            self.adam_m = torch.zeros(self.n_param, **f32) if with_optimizer_state else None
            self.adam_v = torch.zeros(self.n_param, **f32) if with_optimizer_state else None
            self.shadow = (torch.zeros(int(sz.n_weight), dtype=torch.bfloat16, device=device)
                           if sz.n_weight > 0 else None)
            # transposed bf16 weights [in][out] per layer: lets the data-gradient GEMM run in the forward form
            self.shadow_t = (torch.zeros(int(sz.n_weight), dtype=torch.bfloat16, device=device)
                             if sz.n_weight > 0 else None)
            self.acts = torch.zeros(max(int(sz.act_bytes), 16), dtype=torch.uint8, device=device)
            self.dacts = torch.zeros(max(int(sz.dact_bytes), 16), dtype=torch.uint8, device=device)
            self.slabs = (torch.zeros(int(sz.slab_bytes), dtype=torch.uint8, device=device)
                          if sz.slab_bytes > 0 else None)
            # partial column sums of the bias gradients (one small deterministic finish kernel per backward call)
            self.bias_parts = torch.zeros(max(int(sz.bias_part_bytes) // 4, 16), dtype=torch.float32, device=device)
            if int(sz.n_scalars) != S_COUNT:
                raise HipError("library reports %d scalars, binding expects %d" % (int(sz.n_scalars), S_COUNT))
            self.scalars = torch.zeros(int(sz.n_scalars), dtype=torch.float64, device=device)
        self.bufs = Buffers(ptr(self._params), ptr(self.grads), ptr(self.adam_m), ptr(self.adam_v), ptr(self.shadow),
                            ptr(self.acts), ptr(self.dacts), ptr(self.slabs), ptr(self.scalars), ptr(self.shadow_t),
                            ptr(self.bias_parts))
        self.w_off, self.b_off = [], []
        for l in range(self.L):
            w, b, s = C.c_int64(), C.c_int64(), C.c_int64()
            check(self._lib.codae_param_offsets(self._h, l, C.byref(w), C.byref(b), C.byref(s)))
            self.w_off.append(w.value)
            self.b_off.append(b.value)
        self.input_noise = None
        self.loss_emphasis = None
        self._emph_weights = None     # the device tensor codae_emphasis.col_weight borrows
        self.hidden_dropout = None
        self.residual = None          # the codae.tool.Residual in force (None = off)
        self.residual_layers = []     # the skipped layers it resolved to on this stack
        self._residual_ws = None      # the device tensor codae_set_residual borrows (G and the 1-bit masks)
        self.norm = None              # the codae.tool.Norm in force (None = off)
        self.norm_layers = []         # the normalised layers it resolved to on this stack
        self._norm_ws = None          # the device tensor codae_set_norm borrows (r per row and the 1-bit masks)
        self.sparse_code = None       # the codae.tool.SparseCode in force (None = off)
        self.sparse_resolved = None   # (m, Z) it resolved to on this stack: the producing layer and the width of the code
        self._sparse_ws = None        # the device tensor codae_set_sparse_code borrows (the 1-bit keep mask)
        self.recon_loss = None
        self.variable_loss = None     # the codae.tool.VariableLoss in force (None = off)
        self._variable_ws = None      # the device tensor codae_set_variable_loss borrows (table, coefficients, partial sums)
        self.slot_contrast = None
        self._contrast_pins = None    # the device tensors codae_slot_contrast borrows (pool, item ids, work space)
        self.slot_presence = None
        self._presence_table = None   # the device tensor codae_set_slot_presence borrows
        self.tied_weights = False
        self._dataset_image = None    # (data, image): the device tensors codae_set_dataset_image borrows
        self.optimizer = None
        self.trust_ws = None          # lamb / lars: ratios and partial norms (codae_optimizer.trust_ws borrows it), allocated on first use
        self.adam_vmax = None         # AMSGrad's running maximum (codae_optimizer.vmax borrows it), allocated on first use
        self.weight_average = None    # the codae.tool.WeightAverage in force (None = off)
        self.weight_avg = None        # the average itself: n_param floats in the layout of params, allocated on first use and kept
        self.avg_shadow = None        # its bf16 image (bf16 precision), written by sync_average()
        self.avg_bufs = None          # self.bufs with params / shadow_w pointing at the average: what an averaged evaluation reads
        self._avg_stale = True        # the average moved since the last sync_average()
        self.step_count = 0
        self.generation = 0   # bumped by every forward: guards stale backward calls

    def _layer_acts(self, activation):
        """[(kind, p0, p1, p2)] per layer, or None (the relu flags alone)."""
        if activation is None:
            return None
        if isinstance(activation, (list, tuple)) and len(activation) == self.L and all(
                isinstance(a, (list, tuple)) for a in activation):
            acts = [tuple(a) for a in activation]
        else:
            if isinstance(activation, (list, tuple)):
                one = tuple(activation)
            else:
                from ..model.activation import from_factory
                one = from_factory(activation)
            acts = [one if s[2] else (0, 0.0, 0.0, 0.0) for s in self.schedule]
        for a in acts:
            if len(a) != 4:
                raise HipError("activation per layer must be (kind, p0, p1, p2), got %r" % (a,))
        return [(int(a[0]), float(a[1]), float(a[2]), float(a[3])) for a in acts]

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                self._lib.codae_destroy(h)
            except Exception:
                pass
            self._h = None

    # ---- views into the flat vectors --------------------------------------------------
    def join(self):
        """The last update's per-layer Adam kernels may still run on the engine's side stream: make the
        current stream wait for them (call before reading parameters / Adam state / gradients)."""
        with torch.cuda.device(self.device):
            check(self._lib.codae_join(self._h, current_stream()))

    @property
    def params(self):
        self.join()
        return self._params

    def _view(self, flat, l, bias):
        self.join()
        k, n, _ = self.schedule[l]
        if bias:
            return flat[self.b_off[l]:self.b_off[l] + n]
        return flat[self.w_off[l]:self.w_off[l] + n * k].view(n, k)

    def weight(self, l): return self._view(self._params, l, False)
    def bias(self, l): return self._view(self._params, l, True)
    def weight_grad(self, l): return self._view(self.grads, l, False)
    def bias_grad(self, l): return self._view(self.grads, l, True)

    def load_params(self, params):
        """params: list of (W[out,in], b[out]) tensors/arrays."""
        with torch.no_grad():
            for l, (w, b) in enumerate(params):
                self.weight(l).copy_(torch.as_tensor(w, dtype=torch.float32))
                self.bias(l).copy_(torch.as_tensor(b, dtype=torch.float32))
        self.sync_shadows()
        self.reset_average()

    def sync_shadows(self):
        with torch.cuda.device(self.device):
            check(self._lib.codae_sync_shadows(self._h, C.byref(self.bufs), current_stream()))

    # ---- drop-in path -----------------------------------------------------------------
    def forward(self, x, layer_lo=0, layer_hi=None, weights="live"):
        """weights: "live", or "average" to run on the weight average (as eval_step)."""
        layer_hi = self.L if layer_hi is None else layer_hi
        bufs = self._eval_bufs(weights)
        if x.dim() != 2 or x.shape[1] != self.schedule[layer_lo][0]:
            raise HipError("forward: input shape %s does not match layer %d (%d features)"
                           % (tuple(x.shape), layer_lo, self.schedule[layer_lo][0]))
        if x.shape[0] > self.max_batch:
            raise HipError("forward: batch %d exceeds the engine's max_batch %d" % (x.shape[0], self.max_batch))
        x = x.detach().to(dtype=torch.float32).contiguous()
        y = torch.empty((x.shape[0], self.schedule[layer_hi - 1][1]), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(self._lib.codae_forward(self._h, C.byref(bufs), ptr(x), ptr(y), x.shape[0], layer_lo, layer_hi,
                                          1, current_stream()))
        self.generation += 1
        return y

    def backward(self, dy, layer_lo=0, layer_hi=None, need_dx=False):
        layer_hi = self.L if layer_hi is None else layer_hi
        dy = dy.detach().to(dtype=torch.float32).contiguous()
        dx = (torch.empty((dy.shape[0], self.schedule[layer_lo][0]), dtype=torch.float32, device=self.device)
              if need_dx else None)
        with torch.cuda.device(self.device):
            check(self._lib.codae_backward(self._h, C.byref(self.bufs), ptr(dy), ptr(dx), dy.shape[0], layer_lo,
                                           layer_hi, current_stream()))
        return dx

    # ---- fused step path --------------------------------------------------------------
    def make_batch(self, data, row_idx, mask_id, mask_table, B=None, mask_to_use=None, run=0):
        """data [N,io] fp32; row_idx / mask_id int32 [B] or None; mask_table uint8 [n_masks, io] or None;
        mask_to_use int32 [N, nb_run] + run: device-side id lookup when mask_id is None."""
        if data.dtype != torch.float32 or not data.is_contiguous() or data.device != self.device:
            raise HipError("batch data must be a contiguous fp32 tensor on %s" % self.device)
        for name, t in (("row_idx", row_idx), ("mask_id", mask_id)):
            if t is not None and (t.dtype != torch.int32 or t.device != self.device or not t.is_contiguous()):
                raise HipError("%s must be a contiguous int32 tensor on %s" % (name, self.device))
        if mask_table is not None and (mask_table.dtype != torch.uint8 or mask_table.device != self.device):
            raise HipError("mask_table must be a uint8 tensor on %s" % self.device)
        if B is None:
            B = int(row_idx.numel()) if row_idx is not None else int(data.shape[0])
        nb_run = 0
        if mask_to_use is not None:
            if mask_to_use.dtype != torch.int32 or mask_to_use.device != self.device or not mask_to_use.is_contiguous() \
                    or mask_to_use.dim() != 2 or mask_to_use.shape[0] != data.shape[0]:
                raise HipError("mask_to_use must be a contiguous int32 [n_rows, nb_run] tensor on %s" % self.device)
            nb_run = int(mask_to_use.shape[1])
        b = Batch(ptr(data), ptr(row_idx), ptr(mask_id), ptr(mask_table), int(B), int(data.shape[1]),
                  ptr(mask_to_use), nb_run, int(run))
        # the struct only carries raw pointers: pin the tensors to it, or a temporary (mask_id) is
        # returned to the caching allocator and handed to the next torch.empty() while the kernels
        # that read it are still queued
        b._pinned = (data, row_idx, mask_id, mask_table, mask_to_use)
        return b

    def hyper(self, lr, weight_decay, clip=1.0, global_rows=0, betas=(0.9, 0.999), eps=1e-8, step=None):
        return Hyper(lr, weight_decay, betas[0], betas[1], eps, clip if clip else 0.0,
                     self.step_count + 1 if step is None else step, float(global_rows))

    def set_input_noise(self, noise, n_slots=None, n_rows=None):
        """noise: a codae.tool.InputNoise, or None to switch it off.  Every training step form that follows applies it to
        the gathered input before the slot mask (the loss target stays clean; eval steps are never noised); with
        graph=True the next step re-captures.  While it is on, step_path() is 'layers'.
        Swap noise takes the dataset's slot count and row count (n_slots, n_rows); its pool is checked against n_rows and
        moved to the device once, here; a bf16 engine keeps gathering from the registered dataset image."""
        if noise is not None and not hasattr(noise, "as_struct"):
            raise HipError("set_input_noise: expected a codae.tool.InputNoise or None, got %r" % (noise,))
        st = None if noise is None else noise.as_struct()
        pool = None
        if noise is not None and getattr(noise, "kind", None) == "swap":
            # the slots and the pool first: the library refuses the kind without them (a refusal below leaves them set, unused)
            if not n_slots or not n_rows:
                raise HipError("set_input_noise: swap noise needs n_slots and n_rows (the dataset's slot count and rows)")
            rows = noise.pool_rows(int(n_rows))
            with torch.cuda.device(self.device):
                pool = None if rows is None else torch.from_numpy(rows.astype("int32")).to(self.device).contiguous()
            check(self._lib.codae_set_swap_pool(self._h, ptr(pool), int(n_rows) if pool is None else int(pool.numel()), int(n_slots)))
        check(self._lib.codae_set_input_noise(self._h, None if st is None else C.byref(st)))
        swap = noise is not None and getattr(noise, "kind", None) == "swap"
        if not swap and getattr(self, "_swap_set", False):
            check(self._lib.codae_set_swap_pool(self._h, None, 0, 0))      # (the borrowed pool goes with the kind)
        self._swap_pool, self._swap_set = pool, swap
        self.input_noise = noise

    def set_loss_emphasis(self, emphasis, n_slots=None):
        """emphasis: a codae.tool.LossEmphasis, or None to switch it off.  Every training step form that follows minimises
        sum w (x - y)^2 / (global rows * io) with w = column weight * (alpha on a corrupted element, beta elsewhere); the metric
        sums stay unweighted and eval steps are never weighted; with graph=True the next step re-captures.  While it is on,
        step_path() is 'layers'.  n_slots: the number of slots its slot_weight must match (when known).  All defaults
        (LossEmphasis()) = off: the engine runs exactly what it ran before."""
        if emphasis is not None and not hasattr(emphasis, "column_weights"):
            raise HipError("set_loss_emphasis: expected a codae.tool.LossEmphasis or None, got %r" % (emphasis,))
        weights = None
        if emphasis is not None:
            cw = emphasis.column_weights(self.schedule[-1][1], n_slots)
            if cw is not None:
                weights = torch.from_numpy(cw).to(self.device).contiguous()
        self._set_emphasis_struct(None if emphasis is None else Emphasis(emphasis.alpha, emphasis.beta, ptr(weights)))
        self._emph_weights = weights
        self.loss_emphasis = emphasis

    def _set_emphasis_struct(self, st):
        check(self._lib.codae_set_loss_emphasis(self._h, None if st is None else C.byref(st)))

    def set_recon_loss(self, criterion, n_slots=None):
        """criterion: a codae.tool.ReconstructionLoss, or None for the mean squared error.  Every training step form that follows
        minimises it (include/codae_hip.h, "Training criterion"), with the emphasis weights when emphasis is on; epoch_sums()
        stays the unweighted squared-error sums and eval steps never see it; with graph=True the next step re-captures.  While
        a criterion other than the MSE is set, step_path() is 'layers'.  n_slots: slots per row, for slot_cosine.  The default
        (ReconstructionLoss()) = off: the engine runs exactly what it ran before."""
        if criterion is not None and not hasattr(criterion, "as_struct"):
            raise HipError("set_recon_loss: expected a codae.tool.ReconstructionLoss or None, got %r" % (criterion,))
        self._set_recon_struct(None if criterion is None else criterion.as_struct(n_slots))
        self.recon_loss = criterion

    def _set_recon_struct(self, st):
        check(self._lib.codae_set_recon_loss(self._h, None if st is None else C.byref(st)))

    def set_variable_loss(self, criterion):
        """criterion: a codae.tool.VariableLoss, or None to switch it off.  Every training step form of a single process that
        follows minimises the mixed-variable criterion (include/codae_hip.h, "Mixed-variable criterion"): RMSE per regression
        variable, NLL per classification variable, weighted and averaged over the variables; epoch_sums() stays the unweighted
        squared-error sums over all columns and eval steps never see it; with graph=True the next step re-captures.  While it is
        on, step_path() is 'layers' and every step stores its reconstruction (output_view).  graph=True replays the criterion on
        its own only: together with input noise, hidden dropout, an optimizer setting, skips, a norm, the sparse code, tied weights
        or the weight average train_step(graph=True) is refused (HipError naming the option).  Refused (HipError naming the
        option) together with loss emphasis, a ReconstructionLoss kind, the slot contrast, a presence table, swap noise and
        data parallel; on a refusal the previous setting stays."""
        if criterion is None:
            check(self._lib.codae_set_variable_loss(self._h, None))
            self.variable_loss, self._variable_ws = None, None
            return
        if not hasattr(criterion, "predict") or not hasattr(criterion, "as_struct"):
            raise HipError("set_variable_loss: expected a codae.tool.VariableLoss or None, got %r" % (criterion,))
        io = self.schedule[-1][1]
        if criterion.io != io:
            raise HipError("variable loss: the variables cover %d columns, the model has %d" % (criterion.io, io))
        need = int(self._lib.codae_variable_loss_ws_bytes(criterion.n_var, self.max_batch))
        if need < 0:
            raise HipError("set_variable_loss: no work space for %d variables" % criterion.n_var)
        with torch.cuda.device(self.device):
            # (not zero-filled: the setter's blocking copy of the table must not be overtaken by a fill still queued on torch's current
            #  stream, and the kernels write every coefficient and partial sum before they read it)
            ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            st = criterion.as_struct(ws)
            check(self._lib.codae_set_variable_loss(self._h, C.byref(st)))
        self.variable_loss, self._variable_ws = criterion, ws

    def set_slot_contrast(self, contrast, data=None, n_slots=None):
        """contrast: a codae.tool.SlotContrast, or None to switch it off.  Every training step form that follows adds
        weight * sum W l / (rows S) to the criterion's loss (include/codae_hip.h, "Slot contrast"): a softmax over the true item of
        each slot and `negatives` rows sampled per step from `data` (the resident dataset the batches are gathered from, [N, io]
        fp32 on this device); epoch_sums() stays the unweighted squared-error sums and eval steps never see it; with graph=True the
        next step re-captures.  While it is on, step_path() is 'layers'.  weight = 0 = off: the engine runs exactly what it ran
        before.  On a refusal (HipError) the previous setting stays."""
        if contrast is not None and not hasattr(contrast, "candidate_rows"):
            raise HipError("set_slot_contrast: expected a codae.tool.SlotContrast or None, got %r" % (contrast,))
        if contrast is None or contrast.is_default:
            self._set_contrast_struct(None)
            self.slot_contrast, self._contrast_pins = contrast, None
            return
        if data is None or data.dtype != torch.float32 or not data.is_contiguous() or data.device != self.device or data.dim() != 2:
            raise HipError("set_slot_contrast: data must be the contiguous fp32 [N, io] dataset on %s" % self.device)
        io = self.schedule[-1][1]
        if int(data.shape[1]) != io:
            raise HipError("set_slot_contrast: data has %d columns, the model %d" % (int(data.shape[1]), io))
        S = contrast._check_slots(n_slots, io)
        N = int(data.shape[0])
        contrast.check_rows(N)
        with torch.cuda.device(self.device):
            pool = None if contrast.candidates is None else torch.from_numpy(contrast.candidates).to(self.device)
            ids = None
            if contrast.distinct:
                from ..tool.contrast import item_ids
                ids = item_ids(data, S).to(torch.int32).contiguous()
            need = int(self._lib.codae_slot_contrast_ws_bytes(S, contrast.negatives, io // S, int(self.precision == PREC_BF16)))
            if need < 0:
                raise HipError("set_slot_contrast: no work space for S = %d, K = %d, E = %d" % (S, contrast.negatives, io // S))
            ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        self._set_contrast_struct(contrast.as_struct(S, N, pool, ids, ws))
        self.slot_contrast, self._contrast_pins = contrast, (data, pool, ids, ws)

    def _set_contrast_struct(self, st):
        with torch.cuda.device(self.device):      # (the setter raises a per-device kernel attribute: this engine's device)
            check(self._lib.codae_set_slot_contrast(self._h, None if st is None else C.byref(st)))

    def set_slot_presence(self, presence):
        """presence: a codae.tool.SlotPresence, or None to switch it off.  Every step that follows - training in every step form
        AND eval_step - treats the absent slots of a dataset row as missing (include/codae_hip.h, "Slot presence"): 0 in the
        gathered input, no term in the loss, +0 in dL/dy, not in epoch_sums(), not a contrast pair nor a contrast candidate;
        whatever the data holds there is never used.  With graph=True the next step re-captures.  While a table is set,
        step_path() is 'layers' and the loss runs in its stand-alone kernels.  None, or a table without an absent slot
        (SlotPresence.is_default), = off: the engine runs exactly what it ran before.  On a refusal (HipError: slots that do not
        divide io or disagree with slot_cosine / the slot contrast) the previous setting stays."""
        if presence is not None and not hasattr(presence, "assign_masks"):
            raise HipError("set_slot_presence: expected a codae.tool.SlotPresence or None, got %r" % (presence,))
        if presence is None or presence.is_default:
            self._set_presence_table(None)
            self.slot_presence, self._presence_table = presence, None
            return
        table = presence.to(self.device)
        self._set_presence_table(table)
        self.slot_presence, self._presence_table = presence, table

    def _set_presence_table(self, table, n_rows=None, n_slots=None):
        if table is None:
            check(self._lib.codae_set_slot_presence(self._h, None, 0, 0))
            return
        check(self._lib.codae_set_slot_presence(self._h, ptr(table), int(table.shape[0]) if n_rows is None else int(n_rows),
                                                int(table.shape[1]) if n_slots is None else int(n_slots)))

    def set_dataset_image(self, data):
        """data: the resident fp32 [N, io] dataset the batches are gathered from, or None to clear the registration.  bf16 engine only
        (the fp32 engine: a no-op that registers nothing): casts `data` to a bf16 image once (codae_cast_f32_to_bf16, half the
        dataset's bytes) and registers it (include/codae_hip.h, codae_set_dataset_image); every un-noised gather of a batch made
        from this very tensor then reads the image.  No result changes.  A caller that rewrites `data` in place calls this again.
        -> the image tensor, or None."""
        if data is None or self.precision != PREC_BF16:
            check(self._lib.codae_set_dataset_image(self._h, None, None, 0, 0))
            self._dataset_image = None
            return None
        if data.dtype != torch.float32 or not data.is_contiguous() or data.device != self.device or data.dim() != 2:
            raise HipError("set_dataset_image: data must be the contiguous fp32 [N, io] dataset on %s" % self.device)
        with torch.cuda.device(self.device):
            image = torch.empty(data.shape, dtype=torch.bfloat16, device=self.device)
            check(self._lib.codae_cast_f32_to_bf16(ptr(data), ptr(image), data.numel(), current_stream()))
        check(self._lib.codae_set_dataset_image(self._h, ptr(data), ptr(image), int(data.shape[0]), int(data.shape[1])))
        self._dataset_image = (data, image)
        return image

    def set_optimizer(self, optimizer):
        """optimizer: a codae.tool.Optimizer, or None for the default.  Every update that follows - train_step (plain and graph=True),
        step_update, step_update_span, train_step_dp - runs it (include/codae_hip.h, "Optimizer and schedule"): AdamW, SGD with
        (Nesterov) momentum or AMSGrad instead of Adam with L2 decay, the learning rate scaled by the schedule's factor, which the
        update kernel evaluates from the device's own step count - the lr handed to hyper() stays the base rate, and a schedule
        never re-captures a graph (a change of the setting does).  step_path() is unaffected.  AMSGrad's running maximum
        (adam_vmax, n_param floats, zero) is allocated on first use and kept.  The default (Optimizer()) = off: the engine runs
        exactly what it ran before.  "lamb" / "lars" scale every weight matrix's step by its layer-wise trust ratio ("Layer-wise
        trust ratios"): their work space (trust_ws: 64 ratios and the norms pass's partial sums, zero) is allocated on first use and
        kept, trust_ratios() reads the ratios of the last update, and step_update_span is refused while either is set.  On a
        refusal (HipError) the previous setting stays."""
        if optimizer is not None and not hasattr(optimizer, "lr_at"):
            raise HipError("set_optimizer: expected a codae.tool.Optimizer or None, got %r" % (optimizer,))
        if optimizer is None or optimizer.is_default:
            self._set_optimizer_struct(None)
            self.optimizer = optimizer
            return
        vmax, ws = self.adam_vmax, self.trust_ws
        if optimizer.amsgrad and vmax is None:
            with torch.cuda.device(self.device):
                vmax = torch.zeros(self.n_param, dtype=torch.float32, device=self.device)
        if getattr(optimizer, "is_trust", False):
            if ws is None:
                # the trust kinds' work space: 64 fp32 ratios, then the norms pass's partial pairs (codae_trust_ws_bytes), zero
                with torch.cuda.device(self.device):
                    ws = torch.zeros(int(self._lib.codae_trust_ws_bytes(self._h)) // 4, dtype=torch.float32, device=self.device)
            self._set_optimizer_struct(optimizer.as_struct(ptr(vmax), ptr(ws)))
        else:
            self._set_optimizer_struct(optimizer.as_struct(ptr(vmax)))
        self.optimizer, self.adam_vmax, self.trust_ws = optimizer, vmax, ws

    def trust_ratios(self):
        """The layer-wise trust ratios of the last update under lamb / lars: an fp32 device tensor, one value per weight matrix
        (with tied weights per free matrix), a view of the work space's head - zeros before the first update.  Nothing
        synchronises unless the caller reads it.  HipError under another kind."""
        if self.optimizer is None or not getattr(self.optimizer, "is_trust", False):
            raise HipError("trust_ratios: the optimizer is neither lamb nor lars")
        return self.trust_ws[:(self.L + 1) // 2 if self.tied_weights else self.L]

    def _set_optimizer_struct(self, st):
        check(self._lib.codae_set_optimizer(self._h, None if st is None else C.byref(st)))

    # ---- weight average ----------------------------------------------------------------------
    def set_weight_average(self, average):
        """average: a codae.tool.WeightAverage, or None to switch it off.  Every update that follows - train_step (plain and
        graph=True), step_update, train_step_dp - also keeps an EMA or the equal-weight mean of the parameters it produces
        (include/codae_hip.h, "Weight average"), in the same launch; eval_step(weights="average") evaluates on it.  The average
        (weight_avg, n_param floats; avg_shadow, its bf16 image in bf16 precision) is allocated on first use and starts as a copy of
        the current parameters, so it is always a valid model; switching the setting off and on again keeps it (reset_average()
        starts over).  step_path() is unaffected, a new weight never re-captures a graph, a changed setting does.  Parameters,
        moments and shadows keep the bits they have without it.  Refused (HipError, the previous setting stays): a setting out of
        range, and step_update_span while it is on."""
        if average is not None and not hasattr(average, "weight"):
            raise HipError("set_weight_average: expected a codae.tool.WeightAverage or None, got %r" % (average,))
        if average is None or average.is_default:
            self._set_average_struct(None)
            self.weight_average = average
            return
        avg, shadow, fresh = self.weight_avg, self.avg_shadow, self.weight_avg is None
        if fresh:
            with torch.cuda.device(self.device):
                avg = self.params.clone()
                if self.shadow is not None:
                    shadow = torch.zeros_like(self.shadow)
        self._set_average_struct(average.as_struct(ptr(avg)))
        self.weight_average, self.weight_avg, self.avg_shadow = average, avg, shadow
        if fresh:
            self.avg_bufs = Buffers(ptr(avg), ptr(self.grads), ptr(self.adam_m), ptr(self.adam_v), ptr(shadow), ptr(self.acts),
                                    ptr(self.dacts), ptr(self.slabs), ptr(self.scalars), None, ptr(self.bias_parts))
            self._avg_stale = True

    def _set_average_struct(self, st):
        check(self._lib.codae_set_weight_average(self._h, None if st is None else C.byref(st)))

    def averaging(self):
        return self.weight_average is not None and not self.weight_average.is_default

    def reset_average(self):
        """average <- the current parameters (nothing happens before the first set_weight_average)."""
        if self.weight_avg is not None:
            with torch.no_grad():
                self.weight_avg.copy_(self.params)
            self._avg_stale = True

    def load_average(self, params):
        """params: list of (W[out,in], b[out]) tensors/arrays, as load_params takes them, into the average."""
        if self.weight_avg is None:
            raise HipError("load_average: no weight average is kept (set_weight_average first)")
        with torch.no_grad():
            for l, (w, b) in enumerate(params):
                self._view(self.weight_avg, l, False).copy_(torch.as_tensor(w, dtype=torch.float32))
                self._view(self.weight_avg, l, True).copy_(torch.as_tensor(b, dtype=torch.float32))
        self._avg_stale = True

    def sync_average(self):
        """What an averaged evaluation reads, from the fp32 average: with tied weights the decoder matrices of the average as
        mirrors of its encoder's, then (bf16 precision) the bf16 image.  Lazy: only when the average has moved since the last call -
        a training step, load_params, load_average and reset_average mark it."""
        if self.weight_avg is None:
            raise HipError("sync_average: no weight average is kept (set_weight_average first)")
        if self._avg_stale:
            with torch.cuda.device(self.device):
                check(self._lib.codae_sync_shadows(self._h, C.byref(self.avg_bufs), current_stream()))
            self._avg_stale = False

    def average_weight(self, l):
        self.sync_average()
        return self._view(self.weight_avg, l, False)

    def average_bias(self, l):
        self.sync_average()
        return self._view(self.weight_avg, l, True)

    def _eval_bufs(self, weights):
        if weights == "live":
            return self.bufs
        if weights != "average":
            raise HipError("weights must be 'live' or 'average', got %r" % (weights,))
        if not self.averaging() or self.weight_avg is None:
            raise HipError("weights='average': no weight average is kept (set_weight_average first)")
        self.sync_average()
        return self.avg_bufs

    def set_tied_weights(self, on):
        """on: True ties the decoder to the encoder (include/codae_hip.h, "Tied weights"): Linear L-1-l uses the transpose of Linear
        l < L/2, kept in memory as a mirror.  The free parameters are the encoder matrices, the middle matrix of an odd stack and
        every bias; every update that follows - train_step (plain and graph=True), step_update, train_step_dp - folds the decoder
        gradients into the encoder's, takes the norm of the folded vector, updates the free parameters alone and mirrors them
        back.  Switching it on overwrites the decoder matrices and their shadows from the encoder's, as load_params and
        sync_shadows do while it is on.  step_path() is unaffected; with graph=True the next step re-captures.  None / False = off:
        the engine runs exactly what it ran before.  A stack that is not mirror-symmetric is refused (HipError naming the layer
        pair; the previous setting stays), as is step_update_span while tying is on."""
        on = bool(on)
        check(self._lib.codae_set_tied_weights(self._h, 1 if on else 0))
        self.tied_weights = on
        if on:
            self.sync_shadows()

    def tie_pairs(self):
        """[(enc_off, dec_off, rows, cols)] of the tied layer pairs in this engine's flat layout (whether or not tying is on)."""
        from ..tool.tied import TiedWeights
        return TiedWeights.flat_pairs(self.schedule, self.w_off)

    def graph_captures(self):
        """How many times train_step(graph=True) has captured a graph on this engine."""
        return int(self._lib.codae_graph_captures(self._h))

    def set_hidden_dropout(self, dropout):
        """dropout: a codae.tool.HiddenDropout, or None to switch it off.  Every training step form that follows multiplies the
        output of hidden layer l by 0 (probability p_l) or 1 / (1 - p_l), forward and backward, keyed by (seed, dataset row,
        column, step, layer); eval steps never drop; with graph=True the next step re-captures.  While it is on, step_path()
        is 'layers'.  Accepted after no activation, ReLU and LeakyReLU only (HipError otherwise; the previous setting stays).
        All zeros = off: the engine runs exactly what it ran before."""
        if dropout is not None and not hasattr(dropout, "per_layer"):
            raise HipError("set_hidden_dropout: expected a codae.tool.HiddenDropout or None, got %r" % (dropout,))
        self._set_dropout_values(None if dropout is None else dropout.per_layer(self.L), 0 if dropout is None else dropout.seed)
        self.hidden_dropout = dropout

    def _set_dropout_values(self, p, seed=0):
        st = None
        if p is not None:
            arr = (C.c_float * max(len(p), 1))(*[float(v) for v in p])
            st = Dropout(arr, len(p), int(seed))
        check(self._lib.codae_set_hidden_dropout(self._h, None if st is None else C.byref(st)))

    def layer_activations(self):
        """[(kind, p0, p1, p2)] per layer: what follows each Linear, as codae.tool.Residual.resolve takes it."""
        if self.activation is not None:
            return list(self.activation)
        return [(1 if s[2] else 0, 0.0, 0.0, 0.0) for s in self.schedule]

    def set_residual(self, residual):
        """residual: a codae.tool.Residual, or None to switch the skips off.  Every call that follows - training steps in every
        step form, eval steps, forward, score_outfits, with the engine's own or the averaged weights - adds h_l to the output of
        every skipped layer l (include/codae_hip.h, "Residual connections"); with graph=True the next step re-captures.  While a
        skip is on, step_path() is 'layers'; backward() and a forward over a partial layer range raise.  Accepted around layers
        of equal widths other than the last, after no activation, ReLU and LeakyReLU only (HipError naming the layer otherwise;
        the previous setting stays).  None, or no layer = off: the engine runs exactly what it ran before.  The work space (G and
        the 1-bit masks) is allocated here and borrowed by the library until the setting is replaced."""
        if residual is not None and not hasattr(residual, "resolve"):
            raise HipError("set_residual: expected a codae.tool.Residual or None, got %r" % (residual,))
        flags = None
        if residual is not None:
            flags = residual.resolve([s[0] for s in self.schedule], [s[1] for s in self.schedule], self.layer_activations())
        if flags is None or not any(flags):
            check(self._lib.codae_set_residual(self._h, None, None, 0))
            self.residual, self.residual_layers, self._residual_ws = residual, [], None
            return
        from . import ResidualFlags
        arr = (C.c_uint8 * self.L)(*flags)
        st = ResidualFlags(self.L, arr)
        # (flags the library refuses give -1 here: no work space then, and the setter itself reports the error with its own code)
        need = max(int(self._lib.codae_residual_ws_bytes(self._h, C.byref(st))), 0)
        with torch.cuda.device(self.device):
            ws = torch.empty(need, dtype=torch.uint8, device=self.device) if need else None
            check(self._lib.codae_set_residual(self._h, C.byref(st), ptr(ws), need))
        self.residual, self.residual_layers, self._residual_ws = residual, [l for l, f in enumerate(flags) if f], ws

    def set_norm(self, norm):
        """norm: a codae.tool.Norm, or None to switch it off.  Every call that follows - training steps in every step form, eval
        steps, forward, score_outfits, with the engine's own or the averaged weights - normalises the output of every chosen layer
        per batch row (include/codae_hip.h, "Normalisation"); with graph=True the next step re-captures.  While a norm is on,
        step_path() is 'layers'; backward() and a forward over a partial layer range raise.  Accepted on every layer but the last,
        after no activation, ReLU and LeakyReLU only (HipError naming the layer otherwise; the previous setting stays).  None, or
        no layer = off: the engine runs exactly what it ran before.  The work space (r and the 1-bit masks) is allocated here and
        borrowed by the library until the setting is replaced."""
        if norm is not None and not (hasattr(norm, "resolve") and hasattr(norm, "kind_id")):
            raise HipError("set_norm: expected a codae.tool.Norm or None, got %r" % (norm,))
        flags = None
        if norm is not None:
            flags = norm.resolve([s[0] for s in self.schedule], [s[1] for s in self.schedule], self.layer_activations())
        if flags is None or not any(flags):
            check(self._lib.codae_set_norm(self._h, None, None, 0))
            self.norm, self.norm_layers, self._norm_ws = norm, [], None
            return
        from . import NormFlags
        arr = (C.c_uint8 * self.L)(*flags)
        st = NormFlags(self.L, arr, norm.kind_id, float(norm.eps))
        # (flags the library refuses give -1 here: no work space then, and the setter itself reports the error with its own code)
        need = max(int(self._lib.codae_norm_ws_bytes(self._h, C.byref(st))), 0)
        with torch.cuda.device(self.device):
            ws = torch.empty(need, dtype=torch.uint8, device=self.device) if need else None
            check(self._lib.codae_set_norm(self._h, C.byref(st), ptr(ws), need))
        self.norm, self.norm_layers, self._norm_ws = norm, [l for l, f in enumerate(flags) if f], ws

    def set_sparse_code(self, sparse):
        """sparse: a codae.tool.SparseCode, or None to switch it off.  Every call that follows - training steps in every step form,
        eval steps, forward, score_outfits, encode, with the engine's own or the averaged weights - keeps the `keep` first-ranked
        units of the code layer's output per batch row and stores +0 elsewhere (include/codae_hip.h, "Sparse code"); with
        graph=True the next step re-captures.  While it is on, step_path() is 'layers'; backward() and a forward over a partial
        layer range raise.  The producing layer m takes neither skip nor norm, has no activation, ReLU or LeakyReLU and is never
        the last (HipError naming the layer otherwise; the previous setting stays).  None, or keep == Z = off: the engine runs
        exactly what it ran before.  The work space (the 1-bit keep mask of the last training forward, sparse_bits) is allocated
        here and borrowed by the library until the setting is replaced."""
        if sparse is not None and not (hasattr(sparse, "resolve") and hasattr(sparse, "keep")):
            raise HipError("set_sparse_code: expected a codae.tool.SparseCode or None, got %r" % (sparse,))
        if sparse is None:
            check(self._lib.codae_set_sparse_code(self._h, None, None, 0))
            self.sparse_code, self.sparse_resolved, self._sparse_ws = None, None, None
            return
        m, Z = sparse.resolve([s[0] for s in self.schedule], [s[1] for s in self.schedule], self.layer_activations(), self.residual, self.norm)
        from . import SparseCodeCfg
        st = SparseCodeCfg(m + 1, int(sparse.keep))
        # (a setting the library refuses gives -1 here: no work space then, and the setter itself reports the error with its own code)
        need = max(int(self._lib.codae_sparse_code_ws_bytes(self._h, C.byref(st))), 0)
        with torch.cuda.device(self.device):
            ws = torch.empty(need, dtype=torch.uint8, device=self.device) if need else None
            check(self._lib.codae_set_sparse_code(self._h, C.byref(st), ptr(ws), need))
        # (keep == Z is accepted and is off: nothing resolved, no work space)
        self.sparse_code, self.sparse_resolved, self._sparse_ws = sparse, (m, Z) if sparse.keep < Z else None, ws

    def sparse_bits(self, B):
        """The 1-bit keep mask the last training forward left: uint8 [B, ceil(Z / 8)] (a view of the work space; column 8 j + i in
        bit i of byte j, pad bits 0).  For tests and diagnostics."""
        if self._sparse_ws is None:
            raise HipError("sparse_bits: no sparse code is on")
        if not 1 <= int(B) <= self.max_batch:
            raise HipError("sparse_bits: batch %d outside [1, %d]" % (B, self.max_batch))
        ldb = (self.sparse_resolved[1] + 7) // 8
        return self._sparse_ws[:int(B) * ldb].view(int(B), ldb)

    def train_step(self, batch, hyper, graph=False):
        """graph=True: replay the step from a hipGraph (captured on first use; batch.row_idx / mask_id must be
        buffers whose contents, not addresses, change between calls)."""
        fn = self._lib.codae_train_step_graph if graph else self._lib.codae_train_step
        with torch.cuda.device(self.device):
            check(fn(self._h, C.byref(self.bufs), C.byref(batch), C.byref(hyper), current_stream()))
        self.step_count += 1
        self._avg_stale = True

    # ---- data parallel with the library's own RCCL communicator (codae_dp_*) ----------------------------------------
    def dp_unique_id(self):
        """bytes of a fresh ncclUniqueId (call on rank 0, ship to the other ranks)."""
        buf = (C.c_char * 128)()
        check(self._lib.codae_dp_unique_id(buf, 128))
        return bytes(buf)

    def dp_init(self, unique_id, rank, world):
        """Collective: every rank calls it with rank 0's id.  Creates this engine's communicator and collective stream."""
        buf = (C.c_char * 128).from_buffer_copy(unique_id)
        with torch.cuda.device(self.device):
            check(self._lib.codae_dp_init(self._h, buf, int(rank), int(world)))

    def train_step_dp(self, batch, hyper, buckets):
        """codae_train_step_dp: forward + loss, bucketed backward with the all-reduces issued by the library on its own stream,
        clip + Adam - one call, no Python between the buckets."""
        n = len(buckets)
        lo = (C.c_int32 * n)(*[int(a) for a, _ in buckets])
        hi = (C.c_int32 * n)(*[int(b) for _, b in buckets])
        with torch.cuda.device(self.device):
            check(self._lib.codae_train_step_dp(self._h, C.byref(self.bufs), C.byref(batch), C.byref(hyper), n, lo, hi, current_stream()))
        self.step_count += 1
        self._avg_stale = True

    def step_forward_loss(self, batch, hyper, out_y=None):
        with torch.cuda.device(self.device):
            check(self._lib.codae_step_forward_loss(self._h, C.byref(self.bufs), C.byref(batch), C.byref(hyper),
                                                    ptr(out_y), current_stream()))

    def step_backward(self, B, layer_lo, layer_hi, join=True):
        """join=False (data parallel): return without making the current stream wait for the side stream; the
        weight gradients of the range are then ordered on `side_stream()` (see codae_step_backward_async)."""
        fn = self._lib.codae_step_backward if join else self._lib.codae_step_backward_async
        with torch.cuda.device(self.device):
            check(fn(self._h, C.byref(self.bufs), B, layer_lo, layer_hi, current_stream()))

    def side_stream(self):
        """torch view of the engine's side stream (None when it runs everything on the caller's stream)."""
        if getattr(self, "_side_ext", None) is None:
            out = C.c_void_p()
            with torch.cuda.device(self.device):
                check(self._lib.codae_side_stream(self._h, C.byref(out)))
            self._side_ext = torch.cuda.ExternalStream(out.value, device=self.device) if out.value else False
        return self._side_ext or None

    def step_update(self, hyper):
        with torch.cuda.device(self.device):
            check(self._lib.codae_step_update(self._h, C.byref(self.bufs), C.byref(hyper), current_stream()))
        self.step_count += 1
        self._avg_stale = True

    # ---- sharded data-parallel update (codae.train.DataParallel(sharded=True)) -------------------
    def span_sumsq(self, lo, hi, acc):
        """acc (1-element float64 device tensor) += sum grads[lo:hi]^2."""
        with torch.cuda.device(self.device):
            check(self._lib.codae_span_sumsq(C.c_void_p(self.grads.data_ptr() + 4 * lo), hi - lo, ptr(acc), current_stream()))

    def step_update_span(self, hyper, lo, hi, total_sq):
        """clip + Adam on flat elements [lo, hi) with the global sum g^2 in `total_sq` (float64 device tensor)."""
        with torch.cuda.device(self.device):
            check(self._lib.codae_step_update_span(self._h, C.byref(self.bufs), C.byref(hyper), lo, hi, ptr(total_sq),
                                                   current_stream()))

    def replica_tensors(self):
        """Flat tensors (parameter layout) every rank must hold in full for the next forward / backward: the bf16 weight
        shadow in BF16 mode (biases are updated on every rank), the fp32 parameters in F32 mode."""
        return [self.shadow] if self.precision == PREC_BF16 else [self._params]

    def after_replica_sync(self):
        """The shadows were all-gathered: rebuild the transposed copies the data-gradient GEMMs read."""
        with torch.cuda.device(self.device):
            check(self._lib.codae_sync_transposed(self._h, C.byref(self.bufs), current_stream()))

    def new_accumulator(self):
        return torch.zeros(1, dtype=torch.float64, device=self.device)

    def step_stores_output(self, B):
        """True if a fused training step of B rows leaves its fp32 output in the work space (output_view): the engine's own step
        plan, not a guess from the settings."""
        return self._lib.codae_step_stores_output(self._h, C.byref(self.bufs), int(B)) == 1

    def step_path(self, B):
        """'chain' if a fused step of B rows runs the persistent chain kernel, 'layers' for per-layer launches."""
        return "chain" if self._lib.codae_step_path(self._h, C.byref(self.bufs), int(B)) == 1 else "layers"

    def eval_step(self, batch, out_y=None, weights="live"):
        """weights: "live" = the parameters the last step left; "average" = the weight average (synchronised first when it has
        moved): the same kernels and workspaces, reading the average's images."""
        bufs = self._eval_bufs(weights)
        with torch.cuda.device(self.device):
            check(self._lib.codae_eval_step(self._h, C.byref(bufs), C.byref(batch), ptr(out_y), current_stream()))

    def score_outfits(self, data, items, weights="live", n_slots=None):
        """codae_score_outfits (include/codae_hip.h, "Assembled outfits and compatibility"): items int32 [Q, S] on this device, rows of
        `data` (the contiguous fp32 [N, io] dataset on this device) per (outfit, slot), negative = no item; Q * S <= max_batch.  The S
        leave-one-out rows of every outfit go through the evaluation forward (weights: "live" or "average") and each left-out item is
        compared with its reconstruction -> {"score": [Q], "cos": [Q, S], "sq": [Q, S], "n_present": [Q] int32}.  The presence table in
        force (set_slot_presence) makes the pairs it marks absent.  The metric sums, the parameters and the optimizer state are not
        touched; no host synchronisation.  n_slots: S when items is not given as [Q, S]."""
        if data.dtype != torch.float32 or not data.is_contiguous() or data.device != self.device or data.dim() != 2:
            raise HipError("score_outfits: data must be the contiguous fp32 [N, io] dataset on %s" % self.device)
        if not torch.is_tensor(items) or items.dtype != torch.int32 or items.device != self.device or not items.is_contiguous() \
                or items.dim() != 2:
            raise HipError("score_outfits: items must be a contiguous int32 [Q, S] tensor on %s" % self.device)
        Q, S = int(items.shape[0]), int(items.shape[1] if n_slots is None else n_slots)
        bufs = self._eval_bufs(weights)
        with torch.cuda.device(self.device):
            f32 = dict(dtype=torch.float32, device=self.device)
            out = {"score": torch.empty(max(Q, 1), **f32), "cos": torch.empty((max(Q, 1), S), **f32), "sq": torch.empty((max(Q, 1), S), **f32),
                   "n_present": torch.empty(max(Q, 1), dtype=torch.int32, device=self.device)}
            check(self._lib.codae_score_outfits(self._h, C.byref(bufs), ptr(data), int(data.shape[0]), ptr(items), Q, S, ptr(out["cos"]),
                                                ptr(out["sq"]), ptr(out["score"]), ptr(out["n_present"]), current_stream()))
        self.generation += 1
        self._keep_outfits = (data, items)        # (raw pointers: alive until the next call's kernels are queued behind these)
        return out

    def _dense_rows(self, who, t, width):
        """t -> the contiguous fp32 [B, width] device tensor codae_encode / codae_decode read, 1 <= B <= max_batch"""
        if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != width or t.device != self.device:
            raise HipError("%s: input must be a [B, %d] tensor on %s, got %s" % (
                who, width, self.device, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
        if not 1 <= t.shape[0] <= self.max_batch:
            raise HipError("%s: batch %d outside [1, %d]" % (who, t.shape[0], self.max_batch))
        return t.detach().to(dtype=torch.float32).contiguous()

    def _code_layer(self, who, k):
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= self.L - 1:
            raise HipError("%s: layer must be an int in [1, %d], got %r" % (who, self.L - 1, k))
        return k

    def encode(self, x, layers, want_norm=False, weights="live", out=None, norm_out=None):
        """codae_encode (include/codae_hip.h, "Outfit codes"): h_layers of an evaluation forward of x [B, io] -> [B, out[layers - 1]]
        fp32, through every skip and norm of those layers (weights: "live" or "average"); want_norm: -> (code, norm [B]), the fp32
        row norms the export kernel leaves in the same pass.  out / norm_out: contiguous fp32 [B, width] / [B] device tensors to
        write to (a chunk of a preallocated bank and of its norms).  The metric sums, the parameters and the optimizer state are
        not touched; the activations of the last forward are overwritten: no step_backward may follow.  No host synchronisation."""
        k = self._code_layer("encode", layers)
        x = self._dense_rows("encode", x, self.schedule[0][0])
        B, Z = int(x.shape[0]), int(self.schedule[k - 1][1])
        bufs = self._eval_bufs(weights)
        if out is None:
            out = torch.empty((B, Z), dtype=torch.float32, device=self.device)
        elif not torch.is_tensor(out) or out.dtype != torch.float32 or out.device != self.device or tuple(out.shape) != (B, Z) or not out.is_contiguous():
            raise HipError("encode: out must be a contiguous fp32 [%d, %d] tensor on %s" % (B, Z, self.device))
        norm = None
        if want_norm:
            norm = torch.empty(B, dtype=torch.float32, device=self.device) if norm_out is None else norm_out
            if norm.dtype != torch.float32 or norm.device != self.device or tuple(norm.shape) != (B,) or not norm.is_contiguous():
                raise HipError("encode: norm_out must be a contiguous fp32 [%d] tensor on %s" % (B, self.device))
        with torch.cuda.device(self.device):
            check(self._lib.codae_encode(self._h, C.byref(bufs), ptr(x), B, k, ptr(out), ptr(norm), current_stream()))
        self.generation += 1
        self._keep_codes = x                      # (a raw pointer: alive until the next call's kernels are queued behind these)
        return (out, norm) if want_norm else out

    def decode(self, z, layer_lo, weights="live"):
        """codae_decode: Linears layer_lo .. L - 1 on the code z [B, in[layer_lo]] - with their skips and norms; a skip around Linear
        layer_lo reads z itself - -> the fp32 reconstruction [B, io].  Leaves what encode leaves."""
        k = self._code_layer("decode", layer_lo)
        z = self._dense_rows("decode", z, self.schedule[k][0])
        bufs = self._eval_bufs(weights)
        y = torch.empty((z.shape[0], self.schedule[self.L - 1][1]), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(self._lib.codae_decode(self._h, C.byref(bufs), ptr(z), int(z.shape[0]), k, ptr(y), current_stream()))
        self.generation += 1
        self._keep_codes = z
        return y

    def profile_begin(self, classes=("gemm_fwd", "gemm_dgrad", "gemm_wgrad"), max_records=4096, every=1):
        from . import KERNEL_CLASSES
        check(self._lib.codae_profile_stride(self._h, int(every)))
        mask = 0
        for c in classes:
            mask |= 1 << KERNEL_CLASSES.index(c)
        self._prof_cap = int(max_records)
        check(self._lib.codae_profile_begin(self._h, mask, self._prof_cap))

    def profile_end(self):
        """{class name: [milliseconds per launch]} (synchronises on the recorded events)."""
        from . import KERNEL_CLASSES
        kinds = (C.c_int32 * self._prof_cap)()
        ms = (C.c_float * self._prof_cap)()
        n = C.c_int32()
        check(self._lib.codae_profile_end(self._h, kinds, ms, self._prof_cap, C.byref(n)))
        out = {}
        for i in range(n.value):
            out.setdefault(KERNEL_CLASSES[kinds[i]], []).append(float(ms[i]))
        return out

    def output_view(self, B):
        """fp32 [B, io] view of the reconstruction the last step left in the workspace."""
        n = self.schedule[-1][1]
        # y lives after the L activation buffers; recompute its offset like the C side does
        rows = (self.max_batch + 63) // 64 * 64
        es = 2 if self.precision == PREC_BF16 else 4
        off = 0
        for (k, _, _) in self.schedule:
            ld = (k + 63) // 64 * 64 if self.precision == PREC_BF16 else k      # (bf16 rows are padded to whole 64-deep K tiles)
            off += (rows * ld * es + 255) // 256 * 256
        return self.acts[off:off + B * n * 4].view(torch.float32).view(B, n)

    def read_scalars(self):
        """(sq_full, sq_partial, grad_sq, last_loss) — synchronises."""
        s = self.scalars.cpu()
        gsq = float(s[S_GRAD_SQ]) + float(s[S_GRAD_SQ_SLOTS:S_GRAD_SQ_SLOTS + S_N_SLOTS].sum())
        return float(s[S_SQ_FULL]), float(s[S_SQ_PARTIAL]), gsq, float(s[S_LAST_LOSS])

    def record_grad_sq(self, acc):
        """The sharded data-parallel update gathers the global sum g^2 in its own accumulator: keep it where a fused
        step leaves it (scalars[GRAD_SQ]; the slots stay zero on that path)."""
        self.scalars[S_GRAD_SQ:S_GRAD_SQ + 1].copy_(acc.reshape(1))

    def zero_metric_sums(self):
        self.scalars[:2].zero_()

    # ---- state: what defines the run (checkpoint, replica comparison; include/codae_hip.h, "State digest") ---------------------
    def state_tensors(self):
        """Ordered {name: flat tensor} of what defines the run: params, adam_m, adam_v, adam_vmax and weight_avg when allocated, and the
        whole float64 scalars vector (it carries the running epoch sums).  The bf16 shadows (shadow, shadow_t, avg_shadow) are derived:
        sync_shadows() / sync_average() rebuild them from these with the bits the update kernels leave.  Joins the side stream."""
        self.join()
        out = {"params": self._params}
        for name in ("adam_m", "adam_v", "adam_vmax", "weight_avg"):
            if getattr(self, name) is not None:
                out[name] = getattr(self, name)
        out["scalars"] = self.scalars
        return out

    def digest_into(self, src, out, dst=None):
        """Enqueue codae_state_digest on the current stream: out (2 int64 on this device) <- the digest of the contiguous device tensor
        src; dst (same bytes, or None) <- a copy made in the same pass.  No host synchronisation."""
        if not src.is_contiguous() or src.device != self.device:
            raise HipError("digest: the tensor must be contiguous and on %s" % self.device)
        n_bytes = src.numel() * src.element_size()
        if dst is not None and (not dst.is_contiguous() or dst.device != self.device or dst.numel() * dst.element_size() != n_bytes):
            raise HipError("digest: dst must be a contiguous tensor of the same %d bytes on %s" % (n_bytes, self.device))
        if out.dtype != torch.int64 or out.numel() != 2 or out.device != self.device or not out.is_contiguous():
            raise HipError("digest: out must be 2 contiguous int64 on %s" % self.device)
        with torch.cuda.device(self.device):
            check(self._lib.codae_state_digest(ptr(src) if n_bytes else None, ptr(dst) if n_bytes else None, n_bytes, ptr(out),
                                               current_stream()))

    @staticmethod
    def _digest_pairs(host_i64):
        """int64 [n, 2] host tensor -> [(out0, out1)] as unsigned Python ints."""
        return [(int(a) & 0xFFFFFFFFFFFFFFFF, int(b) & 0xFFFFFFFFFFFFFFFF) for a, b in host_i64.tolist()]

    def digest(self, tensor_or_name):
        """(out[0], out[1]) of a state tensor's name or of any contiguous device tensor whose byte count is a multiple of 4;
        synchronises."""
        t = self.state_tensors()[tensor_or_name] if isinstance(tensor_or_name, str) else tensor_or_name
        out = torch.empty(2, dtype=torch.int64, device=self.device)
        self.digest_into(t, out)
        return self._digest_pairs(out.cpu().reshape(1, 2))[0]

    def digests(self):
        """{name: (out[0], out[1])} of every state tensor, in state_tensors() order, in one read; synchronises."""
        st = self.state_tensors()
        out = torch.empty((len(st), 2), dtype=torch.int64, device=self.device)
        for i, t in enumerate(st.values()):
            self.digest_into(t, out[i])
        return dict(zip(st, self._digest_pairs(out.cpu())))

    def set_step_count(self, n):
        """The number of optimizer steps taken (a restored run): the next step is n + 1 for the schedule, the noise, the dropout,
        the contrast's candidates and the weight average."""
        if isinstance(n, bool) or int(n) != n or n < 0:
            raise HipError("set_step_count: expected a count >= 0, got %r" % (n,))
        self.step_count = int(n)
