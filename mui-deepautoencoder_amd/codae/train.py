"""Device-resident training loop for the embedding DAE: the fast counterpart of the inner loop of
script/train_dae_on_embedding.py:194-223 (reference), one fused HIP step per minibatch.

What differs from the drop-in path (model(c_input) + torch loss/optimizer):
  - the dataset matrix stays in HBM and a batch is a vector of int32 row indices
    (DataLoader + collate_embedding, data_tool.py:96-103, become a gather inside the kernels);
  - the corruption mask is a per-sample mask id (Corrupter.mask_to_use[idx][run]) plus the small
    uint8 table, applied on load; the [B, io] fp32 fmask is never built;
  - loss, dL/dy, the epoch metrics (ftl / ptl sums), grad-norm clip and Adam are kernels of
    libcodae_hip.so; nothing is copied to the host per step (the reference moves a [B, io] fp32
    tensor to the host every step, :218-223).

Data parallel (one process per GPU, torch.distributed; backend "nccl" is RCCL over xGMI):
the minibatch is sharded by rows, parameters and Adam state are replicated, the loss is scaled
by the GLOBAL batch so that a SUM all-reduce of the gradients gives the global-batch mean
gradient; gradients are reduced in layer buckets, each launched as soon as its layers'
backward kernels are enqueued, so the reduction of late layers overlaps the backward GEMMs of
early ones; clip + Adam then run identically on every rank.

Sharded update (DataParallel(sharded=True)): the bucket collectives become reduce-scatters, every rank runs clip + Adam
on its 1/N of each bucket only (the bias block, 15 K floats, stays replicated), and the bf16 weight shadows - what the
next forward / backward actually read - are all-gathered: 25 % fewer bytes on xGMI than the all-reduce (4 + 2 instead of
4 + 4 bytes per parameter), Adam's 750 MB pass shrinks N-fold, and the fp32 master parameters / moments of a rank stay
valid for its own shards only until gather_params() is called (checkpoint, read-out).
"""
import os

import torch

from .hostcpu import fit_host_threads, host_cpu_share  # noqa: F401  (re-exported: scripts and bench.py import them here)
from .hip import HipError


class SubsetEpochSampler:
    """Batches of dataset row indices in the order
    DataLoader(dataset, batch_size, sampler=SubsetRandomSampler(indices)) yields them
    (script/train_dae_on_embedding.py:118-128 of the reference): one draw of the loader's base
    seed, then torch.randperm over the subset, both from torch's default generator — so a seeded
    run visits the same batches.  Indices come back as one int64 tensor per batch; nothing is
    gathered on the host."""

    def __init__(self, indices, batch_size):
        self.indices = torch.as_tensor(list(indices), dtype=torch.long)
        self.batch_size = int(batch_size)

    def __len__(self):
        return (len(self.indices) + self.batch_size - 1) // self.batch_size

    def _epoch_order(self):
        torch.empty((), dtype=torch.int64).random_()          # DataLoader iterator's base seed
        # torch.randperm on the CPU draws the same permutation whatever the thread count; with one thread it takes 0.4 ms for
        # 131 072 rows, with one per visible cpu of a GPU box 4-10 ms and the container's CPU quota (fit_host_threads above;
        # tools/abl/randperm_cost.py, tools/bench_script_loop.py)
        n_threads = torch.get_num_threads()
        if n_threads > 1:
            torch.set_num_threads(1)
        try:
            perm = torch.randperm(len(self.indices))
        finally:
            if n_threads > 1:
                torch.set_num_threads(n_threads)
        return self.indices[perm]

    def __iter__(self):
        order = self._epoch_order()
        for o in range(0, len(order), self.batch_size):
            yield order[o:o + self.batch_size]

    def device_batches(self, device, dtype=torch.int32):
        """The same batches as iterating the sampler (same draws from torch's default generator), as views of ONE device tensor
        holding the epoch's whole order: one host-to-device copy per epoch instead of one per step.  (A per-step `.to(device)`
        of a pageable host tensor is a synchronous copy ordered behind the previous step's kernels: the host can never run
        ahead of the device, which costs the step its enqueue time - tools/bench_script_loop.py.)"""
        order = self._epoch_order().to(dtype)
        if torch.device(device).type == "cuda":
            # one pinned staging buffer and one device buffer, both kept: the copy is ordered on the current stream behind the
            # steps that still read the previous epoch's order, and the host only waits for the PREVIOUS copy before reusing the
            # staging buffer (allocating / freeing pinned memory per epoch synchronises the device)
            st = getattr(self, "_stage", None)
            if st is None or st[0].numel() != order.numel() or st[0].dtype != order.dtype or st[1].device != torch.device(device):
                st = (torch.empty(order.numel(), dtype=order.dtype).pin_memory(), torch.empty(order.numel(), dtype=order.dtype, device=device),
                      torch.cuda.Event())
                self._stage = st
            else:
                st[2].synchronize()
            st[0].copy_(order)
            st[1].copy_(st[0], non_blocking=True)
            st[2].record()
            order = st[1]
        else:
            order = order.to(device)
        for o in range(0, len(order), self.batch_size):
            yield order[o:o + self.batch_size]


def shard_batch(batch_indices, rank, world):
    """This rank's rows of one global minibatch (strided: rank, rank + world, ...), or None when the batch has fewer
    rows than there are ranks (the ragged last batch of an epoch): EVERY rank then skips it - a rank with an empty shard
    would fail its launch while the others block forever in the gradient collectives."""
    if world <= 1:
        return batch_indices
    if len(batch_indices) < world:
        return None
    return batch_indices[rank::world]


def seed_all_ranks(seed):
    """Data parallel runs need the same sampler order, mask tables (Python's `random`, data_tool.py:222-226) and initial
    weights on every rank: seed the three generators the reference leaves unseeded (RNG)."""
    import random
    import numpy as np
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def default_buckets(n_layers, n_buckets=4):
    """[(lo, hi)] layer ranges in backward order, sizes decreasing: 10 layers -> (6,10) (3,6) (1,3) (0,1).
    The first buckets' all-reduces hide under the remaining backward GEMMs; the last bucket's cannot, so it
    is the smallest (one layer = 9.4 MB at 1536^2)."""
    n_buckets = max(1, min(n_buckets, n_layers))
    weights = list(range(n_buckets, 0, -1))                     # n, n-1, ..., 1
    total = sum(weights)
    sizes = [max(1, round(n_layers * w / total)) for w in weights]
    while sum(sizes) > n_layers:                                # trim from the biggest
        sizes[sizes.index(max(sizes))] -= 1
    while sum(sizes) < n_layers:                                # pad the first (best hidden) bucket
        sizes[0] += 1
    out, hi = [], n_layers
    for sz in sizes:
        if sz > 0:
            out.append((hi - sz, hi))
            hi -= sz
    return out


def init_rccl_process_group(device, **kw):
    """`torch.distributed.init_process_group("nccl")` (= RCCL on ROCm) with the collectives on HIGH-priority streams.

    Why it matters here: the ROCm runtime multiplexes the streams of one priority level onto a few hardware queues,
    and a `hipStreamWaitEvent` is a barrier packet that holds up EVERYTHING behind it on its hardware queue.  With
    torch's default (normal-priority) collective stream sharing the queue of the compute stream, each bucket
    all-reduce's wait for the engine's side stream stalled the dgrad chain for ~90 us (rocprofv3 trace, forced
    one-rank collectives).  High priority puts the collective stream in its own queue pool: compute stream normal,
    engine side stream low, collectives high."""
    import torch.distributed as dist
    opts = None
    try:
        opts = dist.ProcessGroupNCCL.Options(is_high_priority_stream=True)
    except Exception:                                   # builds without the NCCL/RCCL process group
        opts = None
    if opts is not None:
        kw.setdefault("pg_options", opts)
    dist.init_process_group(backend="nccl", device_id=device, **kw)


class DataParallel:
    """Bucketed gradient all-reduce around an engine's step_* phases.

    `engine` needs: L, grads (flat tensor), w_off (list), b_off (list), n_param,
    step_forward_loss(batch, hyper), step_backward(B, lo, hi), step_update(hyper).
    """

    def __init__(self, engine, process_group=None, n_buckets=None, sharded=False, native=False):
        """n_buckets: 1 .. engine.L; None = one bucket per layer (the first collective starts one layer into the
        backward, the exposed tail is one layer's gradient); sharded: see the module docstring."""
        if n_buckets is None:
            # (the sharded update issues five calls per bucket - reduce-scatter, span norm, span Adam, two shadow all-gathers - and
            #  becomes host-bound with ten of them: 1.86 ms/step in the one-rank rehearsal against 1.36 for the all-reduce path)
            n_buckets = 4 if sharded else engine.L
        import torch.distributed as dist
        self.dist = dist
        self.engine = engine
        self.group = process_group
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(process_group) if dist.is_initialized() else 0
        self.buckets = default_buckets(engine.L, n_buckets)
        self.sharded = bool(sharded)
        # native: the library owns the RCCL communicator (codae_dp_init) and issues the bucket all-reduces itself, on its own
        # stream, inside ONE call per step (codae_train_step_dp) - no Python between the buckets.  torch.distributed is then
        # used only to ship rank 0's ncclUniqueId and for the per-epoch scalar reductions.  Opt-in (CODAE_DP_NATIVE=1 / native=
        # True): it has only ever run with one rank on this build's single-GPU test boxes.
        import os as _os
        self.native = bool(native) or _os.environ.get("CODAE_DP_NATIVE") == "1"
        # tied weights: the fold runs inside the engine's update, behind every reduce of the non-sharded paths (torch.distributed,
        # bucketed, native); a shard of the sharded update would hold one half of a tied pair
        self._refuse_sharded_tie()
        self._refuse_sharded_average()
        self._refuse_sharded_trust()
        if self.native:
            if self.sharded:
                raise ValueError("native RCCL data parallel: the sharded update goes through torch.distributed only")
            if not hasattr(engine, "dp_init"):
                raise ValueError("native RCCL data parallel needs the HIP engine")
            ids = [engine.dp_unique_id() if self.rank == 0 else None]
            if dist.is_initialized() and self.world > 1:
                dist.broadcast_object_list(ids, src=0, group=process_group)
            engine.dp_init(ids[0], self.rank, self.world)
        if self.sharded:
            for lo, hi in self.buckets:
                n = self._weight_span_bounds(lo, hi)
                if (n[1] - n[0]) % (4 * self.world) != 0:
                    raise ValueError("sharded update: bucket of %d elements does not split into %d shards of whole float4s"
                                     % (n[1] - n[0], self.world))
        # CODAE_DP_FORCE_ALLREDUCE=1: issue the bucketed collectives even with one rank (lets a
        # single-GPU box exercise the RCCL path end to end)
        import os
        self.always_reduce = dist.is_initialized() and os.environ.get("CODAE_DP_FORCE_ALLREDUCE") == "1"
        self._tw_every, self._tw_step, self._tw = 0, 0, []

    def _refuse_sharded_tie(self):
        eng = self.engine
        if self.sharded and getattr(eng, "tied_weights", False) and eng.L >= 2:
            from .tool.tied import TiedWeights
            raise TiedWeights.sharded_refusal(eng.L)

    def _refuse_sharded_average(self):
        eng = self.engine
        if self.sharded and getattr(eng, "averaging", None) is not None and eng.averaging():
            raise HipError("weight average: the sharded update is not supported: the average of a shard would have to be "
                           "all-gathered too")

    def _refuse_sharded_trust(self, optimizer=None):
        """lamb / lars (the engine's setting, or the one about to be set): a matrix's norm spans shards."""
        opt = optimizer if optimizer is not None else getattr(self.engine, "optimizer", None)
        if self.sharded and opt is not None and getattr(opt, "is_trust", False):
            raise HipError("%s: the sharded update is not supported: a matrix's norm spans shards" % opt.kind)

    # ---- exposed-wait timing (bench.py --gpus N) ------------------------------------------
    def time_waits(self, every=4):
        """In every `every`-th step bracket each bucket's wait with a hipEvent pair on the compute stream: the
        elapsed time is how long the step was held up by that bucket's all-reduce (0 = fully hidden)."""
        self._tw_every, self._tw_step, self._tw = max(1, int(every)), 0, []

    def wait_report(self):
        """[mean exposed milliseconds per step] per bucket (last entry: the bias block); synchronises."""
        if not self._tw:
            return None
        import torch
        torch.cuda.synchronize()
        n = len(self._tw[0])
        return [sum(rec[i][0].elapsed_time(rec[i][1]) for rec in self._tw) / len(self._tw) for i in range(n)]

    def _weight_span_bounds(self, lo, hi):
        # weights of consecutive layers are contiguous in the flat vector
        end = self.engine.w_off[hi] if hi < self.engine.L else self.engine.b_off[0]
        return self.engine.w_off[lo], end

    def _weight_span(self, lo, hi):
        a, b = self._weight_span_bounds(lo, hi)
        return self.engine.grads[a:b]

    def _shard_bounds(self, lo, hi):
        """element range of THIS rank's shard of bucket (lo, hi)"""
        a, b = self._weight_span_bounds(lo, hi)
        n = (b - a) // self.world
        return a + self.rank * n, a + (self.rank + 1) * n

    def backward_and_reduce(self, B):
        eng = self.engine
        if self.world == 1 and not self.always_reduce:
            eng.step_backward(B, 0, eng.L)
            return
        works = []
        side = eng.side_stream() if hasattr(eng, "side_stream") else None
        if side is not None:
            # No join between buckets: the bucket's weight gradients are complete on the engine's side stream, so the
            # collective is ordered behind THAT stream while the main stream goes straight on with the next bucket.
            import torch
            for lo, hi in self.buckets:
                eng.step_backward(B, lo, hi, join=False)
                with torch.cuda.stream(side):
                    works.append(self.dist.all_reduce(self._weight_span(lo, hi), op=self.dist.ReduceOp.SUM,
                                                      group=self.group, async_op=True))
            eng.join()
        else:
            for lo, hi in self.buckets:
                eng.step_backward(B, lo, hi)
                works.append(self.dist.all_reduce(self._weight_span(lo, hi), op=self.dist.ReduceOp.SUM,
                                                  group=self.group, async_op=True))
        # bias gradients of layer l are finished by the dgrad of layer l+1: reduce the block last
        works.append(self.dist.all_reduce(eng.grads[eng.b_off[0]:eng.n_param], op=self.dist.ReduceOp.SUM,
                                          group=self.group, async_op=True))
        timed = False
        if self._tw_every:
            self._tw_step += 1
            timed = self._tw_step % self._tw_every == 0
        if not timed:
            # every collective of this process group runs in issue order on ONE internal stream, so the compute stream only has to
            # wait for the LAST one (the bias block): one cross-stream wait per step instead of one per bucket (~11 us of compute-
            # stream time each in the one-rank rehearsal: 0.12 ms per step with per-layer buckets)
            if self.dist.get_backend(self.group) == "nccl":
                works[-1].wait()
                self._keep_works = works      # (handles stay referenced until the next step replaces them)
            else:
                for w in works:               # (gloo, the CPU test backend: no stream semantics)
                    w.wait()
            return
        import torch
        rec = []
        for w in works:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            w.wait()
            e1.record()
            rec.append((e0, e1))
        self._tw.append(rec)

    def train_step(self, batch, hyper, B):
        """forward+loss -> bucketed backward with overlapped all-reduce -> clip+Adam.
        `hyper.loss_scale_rows` must hold the GLOBAL batch rows."""
        if self.native:
            self.engine.train_step_dp(batch, hyper, self.buckets)
            return
        self._refuse_sharded_tie()             # (tying switched on after this object was built)
        self._refuse_sharded_average()
        self._refuse_sharded_trust()
        self.engine.step_forward_loss(batch, hyper)
        if self.sharded and (self.world > 1 or self.always_reduce):
            self._backward_reduce_scatter(B)
            self._sharded_update(hyper)
            return
        self.backward_and_reduce(B)
        self.engine.step_update(hyper)

    # ---- sharded update ---------------------------------------------------------------------
    def _backward_reduce_scatter(self, B):
        """As backward_and_reduce, but every bucket is REDUCE-SCATTERED: afterwards this rank holds the summed gradient of
        its own shard of each bucket (in place, inside the flat gradient vector); the bias block is all-reduced."""
        eng = self.engine
        works = []
        side = eng.side_stream() if hasattr(eng, "side_stream") else None
        for lo, hi in self.buckets:
            if side is not None:
                eng.step_backward(B, lo, hi, join=False)
            else:
                eng.step_backward(B, lo, hi)
            span = self._weight_span(lo, hi)
            a, b = self._shard_bounds(lo, hi)
            shard = eng.grads[a:b]
            if side is not None:
                with torch.cuda.stream(side):
                    works.append(self.dist.reduce_scatter_tensor(shard, span, op=self.dist.ReduceOp.SUM, group=self.group, async_op=True))
            else:
                works.append(self.dist.reduce_scatter_tensor(shard, span, op=self.dist.ReduceOp.SUM, group=self.group, async_op=True))
        if side is not None:
            eng.join()
        works.append(self.dist.all_reduce(eng.grads[eng.b_off[0]:eng.n_param], op=self.dist.ReduceOp.SUM, group=self.group, async_op=True))
        if self.dist.get_backend(self.group) == "nccl":
            works[-1].wait()                  # (one in-order collective stream: see backward_and_reduce)
            self._keep_works = works
        else:
            for w in works:
                w.wait()

    def _sharded_update(self, hyper):
        eng = self.engine
        # clip_grad_norm_'s total norm: every rank's shards (+ the replicated bias block, counted once) -> one all-reduce
        acc = eng.new_accumulator()
        for lo, hi in self.buckets:
            a, b = self._shard_bounds(lo, hi)
            eng.span_sumsq(a, b, acc)
        if self.rank == 0:
            eng.span_sumsq(eng.b_off[0], eng.n_param, acc)
        self.dist.all_reduce(acc, op=self.dist.ReduceOp.SUM, group=self.group)
        self.last_grad_sq = acc
        if hasattr(eng, "record_grad_sq"):
            eng.record_grad_sq(acc)          # where read_scalars() / last_loss_and_grad_norm() look for the step's sum g^2
        for lo, hi in self.buckets:
            a, b = self._shard_bounds(lo, hi)
            eng.step_update_span(hyper, a, b, acc)
        eng.step_update_span(hyper, eng.b_off[0], eng.n_param, acc)
        # what the next step reads must be whole on every rank (RCCL gathers in place: a rank's input IS its slot of
        # the output; gloo, the CPU test backend, wants a separate input)
        in_place = self.dist.get_backend(self.group) == "nccl"
        works = []
        for t in eng.replica_tensors():
            for lo, hi in self.buckets:
                a, b = self._weight_span_bounds(lo, hi)
                sa, sb = self._shard_bounds(lo, hi)
                src = t[sa:sb] if in_place else t[sa:sb].clone()
                works.append(self.dist.all_gather_into_tensor(t[a:b], src, group=self.group, async_op=True))
        for w in works:
            w.wait()
        eng.after_replica_sync()
        eng.step_count += 1

    def gather_params(self):
        """Sharded mode: make the fp32 master parameters whole on every rank (each rank has only kept its own shards
        current).  Call before reading / saving parameters."""
        if not self.sharded or self.world == 1:
            return
        eng = self.engine
        p = eng.params if not hasattr(eng, "_params") else eng._params
        for lo, hi in self.buckets:
            a, b = self._weight_span_bounds(lo, hi)
            sa, sb = self._shard_bounds(lo, hi)
            self.dist.all_gather_into_tensor(p[a:b], p[sa:sb].clone(), group=self.group)

    def replicas_agree(self):
        """Collective: whether every rank holds rank 0's state, bit for bit - the per-tensor state digests (16 bytes each, computed
        on the device: include/codae_hip.h, "State digest") are all-gathered and compared; the same answer on every rank.  A check
        against silent divergence that moves no tensor to the host.  The scalars vector is left out: it holds each rank's own partial
        epoch sums and the loss of its own shard.  Refused with the sharded update, whose moments live in shards."""
        if self.sharded:
            raise HipError("replicas_agree(): the sharded update is not supported: the moments of a rank live in its shards")
        eng = self.engine
        with torch.cuda.device(eng.device):
            st = {n: t for n, t in eng.state_tensors().items() if n != "scalars"}
            mine = torch.empty((len(st), 2), dtype=torch.int64, device=eng.device)
            for i, t in enumerate(st.values()):
                eng.digest_into(t, mine[i])
        if self.world == 1:
            return True
        if self.dist.get_backend(self.group) != "nccl":
            mine = mine.cpu()                  # (gloo, the CPU test backend)
        every = [torch.empty_like(mine) for _ in range(self.world)]
        self.dist.all_gather(every, mine, group=self.group)
        return all(bool(torch.equal(every[0], e)) for e in every[1:])

    def broadcast_params(self, params_flat):
        if self.world > 1:
            self.dist.broadcast(params_flat, src=0, group=self.group)

    def reduce_scalars(self, t):
        if self.world > 1:
            self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, group=self.group)
        return t


class _ResidentInventory:
    """The slots of a resident [N, S*E] data matrix in the shape tool.ComplementRetriever reads (data_per_category views).
    The global scaling of dataset.data does not change cosines."""

    def __init__(self, data, S, E):
        self.nb_used_category, self.embedding_size = S, E
        self.data_per_category = {c: data[:, c * E:(c + 1) * E] for c in range(S)}


def _is_variable_loss(criterion):
    from .tool.variable_loss import VariableLoss
    return isinstance(criterion, VariableLoss)


class HipEmbeddingTrainer:
    """Owns a DaeEngine, the resident dataset and the mask tables; runs train / eval steps."""

    def __init__(self, schedule, data, mask_table_u8, mask_to_use_i32, lr, weight_decay, clip=1.0,
                 max_batch=8192, precision="bf16", device="cuda:0", distributed=False, n_buckets=None, use_graph=False,
                 sharded_update=False, native_dp=False, activation=None, n_slots=None, input_noise=None,
                 loss_emphasis=None, hidden_dropout=None, criterion=None, contrast=None, optimizer=None, presence=None,
                 tied_weights=None, dataset_image=True, weight_average=None, residual=None, norm=None, sparse_code=None):
        """use_graph: replay the fused step from a hipGraph (codae_train_step_graph): for launch-bound shapes
        (small batches); single process only - the bucketed data-parallel step is not captured.
        activation: what follows every hidden Linear, as the model classes take it (a factory called as activation(True),
        e.g. torch.nn.ELU); None = ReLU.  Every step form (fused, graph replay, data parallel) runs it.
        n_slots: categories per row (complete() only; default: read off the mask table).
        input_noise: a codae.tool.InputNoise (Gaussian / masking / salt-and-pepper, or swap: a slot replaced by another row's item
        of that slot, drawn from the noise's pool) applied to the gathered training input before the slot mask, in every step form (fused, graph replay, torch.distributed, sharded, native data parallel);
        keyed by the dataset row and the optimizer step, so N ranks noise their shards exactly as one process noises the
        global batch.  eval_batch and complete never apply it.  None = off.
        loss_emphasis: a codae.tool.LossEmphasis: the training loss weights corrupted elements (the blanked slot, elements the
        input noise replaced) by alpha, untouched ones by beta, and every column by its slot / column weight, in every step
        form; epoch_sums() stays unweighted, eval_batch and complete are never weighted.  None (or all defaults) = off.
        hidden_dropout: a codae.tool.HiddenDropout: the output of every hidden Linear (after its activation: none, ReLU or
        LeakyReLU) is multiplied by 0 with probability p or by 1 / (1 - p), in every step form, keyed by the dataset row, the
        optimizer step and the layer; the loss and epoch_sums() of a training step are those of the dropped network;
        eval_batch and complete never drop.  None (or p = 0) = off.
        criterion: a codae.tool.ReconstructionLoss: the training loss is L1, SmoothL1, Huber or the per-slot cosine (optionally
        with an MSE anchor) instead of the mean squared error, in every step form, weighted by loss_emphasis when that is on;
        epoch_sums() stays the unweighted squared-error sums, eval_batch and complete never see it.  None (or the default
        ReconstructionLoss()) = the mean squared error, exactly as before.  Or a codae.tool.VariableLoss: the mixed-variable
        criterion for rows made of variables (RMSE per numeric variable, NLL per one-hot variable; any io in fp32), in every
        step form of a single process - it composes with the element noises, dropout, skips, norms, the sparse code, every
        optimizer, tied weights, the weight average and checkpoints on plain steps (use_graph=True replays the criterion on its own
        only: with any of those options train_batch raises a HipError naming the option), and is refused (HipError naming the option) with loss
        emphasis, the slot contrast, a presence table, swap noise and distributed=True; last_output() then gives the step's
        reconstruction, and the embedding-slot features (complete*, score_outfits, the metrics, encode_items, code_index) raise.
        contrast: a codae.tool.SlotContrast: a sampled softmax over the true item of each slot and negatives drawn per step from
        the resident dataset, added to the criterion's loss in every step form (candidates keyed by the optimizer step and the
        slot, shared by all ranks); epoch_sums(), eval_batch and complete never see it.  None (or weight 0) = off, exactly as
        before.
        optimizer: a codae.tool.Optimizer: AdamW, SGD with (Nesterov) momentum or AMSGrad instead of Adam with L2 decay, and a
        warm-up + cosine / linear / step schedule on `lr`, in every step form (fused, graph replay - a schedule never re-captures
        -, torch.distributed, sharded, native data parallel); `lr` stays the base rate, current_lr() tells the scheduled one.
        None (or the default Optimizer()) = Adam at a constant rate, exactly as before.
        presence: a codae.tool.SlotPresence over the rows of `data`: rows that lack an item in some slots train, evaluate and
        complete - an absent slot is 0 in the input, has no term in the loss, the monitors or the contrast, and is never a
        candidate of complete(); what `data` holds there is never used.  Every step form and eval_batch.  None (or a table
        without an absent slot) = off, exactly as before.
        tied_weights: True ties the decoder to the encoder (include/codae_hip.h, "Tied weights"): Linear L-1-l uses the transpose of
        Linear l, the free parameters are the encoder matrices, the middle one of an odd stack and every bias, in every step form
        but the sharded update (refused, as is a stack that is not mirror-symmetric: HipError naming the layer pair).  params(),
        eval_batch and complete see whole decoder matrices, kept as mirrors.  None / False = off, exactly as before.
        dataset_image: bf16 precision only: keep a bf16 image of `data` beside it (half its bytes again), cast once here, and let
        every un-noised gather - training in every step form, eval_batch - read it instead of converting the fp32 rows every step
        (DaeEngine.set_dataset_image); the results are bit for bit the same.  The trainer never writes to `data`; a caller that
        rewrites self.data in place calls refresh_dataset_image().  False, or CODAE_NO_DATASET_IMAGE in the environment = no
        image, exactly as before.
        weight_average: a codae.tool.WeightAverage: every update also keeps an EMA or the equal-weight mean (SWA) of the parameters
        it produces, in the update's own launch and in every step form but the sharded update (refused); eval_batch and complete
        take weights="average" to run on it, params(average=True) / average_params() read it.  It starts as a copy of the
        parameters; load_params and init_params reset it.  Training itself is untouched: parameters, moments and shadows keep
        their bits.  None (or kind "off") = off, exactly as before.
        residual: a codae.tool.Residual: an identity skip around every chosen hidden layer of equal widths (after no activation,
        ReLU or LeakyReLU; never the last layer), h_{l+1} = act(W_l h_l + b_l) + h_l.  It is part of the model: every step form,
        eval_batch, complete, score_outfits and weights="average" run through the skips, and checkpoints record them.  A layer
        that cannot take a skip is refused (HipError naming the layer and the reason).  None (or no layer) = off, exactly as
        before.
        norm: a codae.tool.Norm: parameter-free layer or RMS normalisation of every chosen layer's output, per batch row, after the
        activation, dropout and the skip (never the last layer; after no activation, ReLU or LeakyReLU; any widths).  It is part
        of the model like the skips: every step form, eval_batch, complete, score_outfits and weights="average" run through it,
        and checkpoints record it.  A layer that cannot take it is refused (HipError naming the layer and the reason).  None (or
        no layer) = off, exactly as before.
        sparse_code: a codae.tool.SparseCode(keep, layer=None): the hard top-k code layer of a k-sparse autoencoder - per batch row
        the `keep` units of h_layer (default: code_layers) that rank first by magnitude keep their bits, every other unit is +0,
        and the backward selects the same units.  It is part of the model like the skips and the norm: every step form,
        eval_batch, complete, score_outfits, encode, code_index and weights="average" run through it, and checkpoints record it.
        The producing layer takes neither skip nor norm (name the other layers), has no activation, ReLU or LeakyReLU and is
        never the last (HipError naming the layer and the reason).  None, or keep == Z = off, exactly as before."""
        from .hip.engine import DaeEngine
        fit_host_threads()      # the loop that feeds this trainer must not get its container CPU-throttled (codae/hostcpu.py)
        self.device = torch.device(device)
        self.engine = DaeEngine(schedule, max_batch, precision, self.device, activation=activation)
        if input_noise is not None and getattr(input_noise, "kind", None) != "swap":
            self.engine.set_input_noise(input_noise)
        self.data = data.to(device=self.device, dtype=torch.float32).contiguous()
        self.dataset_image = bool(dataset_image) and not os.environ.get("CODAE_NO_DATASET_IMAGE")
        self.refresh_dataset_image()
        self.mask_table = None if mask_table_u8 is None else mask_table_u8.to(self.device).contiguous()
        self.mask_to_use = None if mask_to_use_i32 is None else mask_to_use_i32.to(self.device).contiguous()
        self.lr, self.weight_decay, self.clip = lr, weight_decay, clip
        self.n_slots = n_slots
        if input_noise is not None and getattr(input_noise, "kind", None) == "swap":
            self.set_input_noise(input_noise)      # (needs the slots and the dataset's rows)
        if loss_emphasis is not None:
            self.set_loss_emphasis(loss_emphasis)
        if hidden_dropout is not None:
            self.set_hidden_dropout(hidden_dropout)
        if residual is not None:
            self.set_residual(residual)
        if norm is not None:
            self.set_norm(norm)
        if sparse_code is not None:
            self.set_sparse_code(sparse_code)
        if criterion is not None:
            if distributed and _is_variable_loss(criterion):
                raise HipError("variable loss: data parallel (distributed=True) is not supported: a global-batch RMSE is not a sum over shards")
            self.set_criterion(criterion)
        if contrast is not None:
            self.set_contrast(contrast)
        self.dp = None                  # (built below, once the engine holds its settings: DataParallel refuses what a shard cannot do)
        if optimizer is not None:
            self.set_optimizer(optimizer)
        self.presence = None
        if presence is not None:
            self.set_presence(presence)
        if tied_weights:
            self.set_tied_weights(True)
        if weight_average is not None:
            self.set_weight_average(weight_average)
        self.dp = DataParallel(self.engine, n_buckets=n_buckets, sharded=sharded_update, native=native_dp) if distributed else None
        self.world = self.dp.world if self.dp else 1
        self.use_graph = bool(use_graph) and self.dp is None
        # graph replay freezes kernel arguments: the step's row indices / mask ids are copied into these
        self._idx_buf = torch.zeros(max_batch, dtype=torch.int32, device=self.device) if self.use_graph else None
        self._mid_buf = torch.zeros(max_batch, dtype=torch.int32, device=self.device) if self.use_graph else None
        # (the default stream cannot be captured: graph steps run on a stream of their own, ordered after / before
        # the caller's current stream)
        self._graph_stream = torch.cuda.Stream(device=self.device) if self.use_graph else None

    def refresh_dataset_image(self):
        """(Re)build and register the bf16 image of self.data - after the dataset was rewritten in place.  Nothing happens when the
        trainer keeps no image (dataset_image=False, fp32 precision, CODAE_NO_DATASET_IMAGE)."""
        from .hip import PREC_BF16
        if self.dataset_image and self.engine.precision == PREC_BF16:
            self.engine.set_dataset_image(self.data)

    def set_input_noise(self, noise):
        """DaeEngine.set_input_noise; swap noise gets the trainer's number of slots (n_slots, else read off the mask table) and the
        resident dataset's row count, against which its pool is checked.  The presence table it honours is the trainer's own."""
        if noise is not None and getattr(noise, "kind", None) == "swap":
            if not self.n_slots and self.mask_table is None:
                raise HipError("swap noise: the trainer has neither n_slots nor a mask table to read the slots from; "
                               "construct it with n_slots")
            self.engine.set_input_noise(noise, n_slots=self._slots()[0], n_rows=int(self.data.shape[0]))
        else:
            self.engine.set_input_noise(noise)

    def set_loss_emphasis(self, emphasis):
        """DaeEngine.set_loss_emphasis with the trainer's number of slots (n_slots, else read off the mask table) for a
        slot_weight."""
        S = None
        if emphasis is not None and getattr(emphasis, "slot_weight", None) is not None and (self.n_slots or self.mask_table is not None):
            S = self._slots()[0]
        self.engine.set_loss_emphasis(emphasis, n_slots=S)

    def set_criterion(self, criterion):
        """DaeEngine.set_recon_loss with the trainer's number of slots (n_slots, else read off the mask table) for slot_cosine; a
        codae.tool.VariableLoss goes to DaeEngine.set_variable_loss (and replaces a ReconstructionLoss kind only when that is the
        default: both at once are refused).  None switches both off."""
        if _is_variable_loss(criterion):
            if self.__dict__.get("dp") is not None:
                raise HipError("variable loss: data parallel is not supported: a global-batch RMSE is not a sum over shards")
            self.engine.set_variable_loss(criterion)
            self.__dict__.pop("_retrievers", None)
            return
        if getattr(self.engine, "variable_loss", None) is not None and (criterion is None or getattr(criterion, "is_default", False)):
            self.engine.set_variable_loss(None)
        S = None
        if criterion is not None and getattr(criterion, "kind", None) == "slot_cosine":
            if not self.n_slots and self.mask_table is None:
                raise HipError("criterion slot_cosine: the trainer has neither n_slots nor a mask table to read the slots from; "
                               "construct it with n_slots")
            S = self._slots()[0]
        self.engine.set_recon_loss(criterion, n_slots=S)

    def set_contrast(self, contrast):
        """DaeEngine.set_slot_contrast on the resident dataset with the trainer's number of slots (n_slots, else read off the mask
        table); None switches it off."""
        S = None
        if contrast is not None and not getattr(contrast, "is_default", True):
            if not self.n_slots and self.mask_table is None:
                raise HipError("slot contrast: the trainer has neither n_slots nor a mask table to read the slots from; "
                               "construct it with n_slots")
            S = self._slots()[0]
        self.engine.set_slot_contrast(contrast, self.data, n_slots=S)

    def set_presence(self, presence):
        """DaeEngine.set_slot_presence for the resident dataset: a codae.tool.SlotPresence with one row per dataset row, or None to
        switch it off.  complete() then ranks only rows that have the slot."""
        if presence is not None and not getattr(presence, "is_default", True) and presence.n_rows != int(self.data.shape[0]):
            raise HipError("slot presence: the table has %d rows, the dataset %d" % (presence.n_rows, int(self.data.shape[0])))
        self.engine.set_slot_presence(presence)
        self.presence = None if presence is None or presence.is_default else presence
        self.__dict__.pop("_retrievers", None)

    def set_tied_weights(self, on):
        """DaeEngine.set_tied_weights: True ties the decoder to the encoder (the decoder matrices become mirrors at once), None /
        False unties it (the matrices stay as they are and train freely from there)."""
        dp = self.__dict__.get("dp")
        if on and dp is not None and dp.sharded and self.engine.L >= 2:
            from .tool.tied import TiedWeights
            raise TiedWeights.sharded_refusal(self.engine.L)
        self.engine.set_tied_weights(bool(on))

    def set_weight_average(self, average):
        """DaeEngine.set_weight_average: a codae.tool.WeightAverage, or None to switch it off (the average kept so far stays
        readable).  Refused with the sharded update."""
        dp = self.__dict__.get("dp")
        if average is not None and not getattr(average, "is_default", True) and dp is not None and dp.sharded:
            raise HipError("weight average: the sharded update is not supported: the average of a shard would have to be "
                           "all-gathered too")
        self.engine.set_weight_average(average)

    def set_optimizer(self, optimizer):
        """DaeEngine.set_optimizer: a codae.tool.Optimizer, or None for Adam at a constant rate."""
        if self.dp is not None:
            self.dp._refuse_sharded_trust(optimizer)         # (before anything changes: the previous setting stays)
        self.engine.set_optimizer(optimizer)

    def trust_ratios(self):
        """DaeEngine.trust_ratios: the fp32 [n_matrices] layer-wise ratios of the last update under lamb / lars (a device tensor;
        nothing synchronises unless the caller reads it)."""
        return self.engine.trust_ratios()

    def current_lr(self):
        """The learning rate of the NEXT step as the update kernel forms it: the fp32 lr_t at step_count + 1 (the fp32 base lr
        without a schedule)."""
        opt = self.engine.optimizer
        if opt is None:
            from .tool.optimizer import Optimizer
            opt = Optimizer()
        return opt.lr_at(self.lr, self.engine.step_count + 1)

    def set_hidden_dropout(self, dropout):
        """DaeEngine.set_hidden_dropout: a codae.tool.HiddenDropout, or None to switch it off."""
        self.engine.set_hidden_dropout(dropout)

    def set_residual(self, residual):
        """DaeEngine.set_residual: a codae.tool.Residual, or None to switch the skips off."""
        self.engine.set_residual(residual)

    def set_norm(self, norm):
        """DaeEngine.set_norm: a codae.tool.Norm, or None to switch the normalisation off."""
        self.engine.set_norm(norm)

    def set_sparse_code(self, sparse_code):
        """DaeEngine.set_sparse_code: a codae.tool.SparseCode, or None to switch the sparse code off."""
        self.engine.set_sparse_code(sparse_code)

    # ---- parameters ---------------------------------------------------------------------
    def load_params(self, params):
        self.engine.load_params(params)
        if self.dp:
            self.dp.broadcast_params(self.engine.params)
            self.engine.sync_shadows()
            self.engine.reset_average()        # (behind the broadcast: every rank's average starts from rank 0's parameters)

    def init_params(self, seed=0):
        """Xavier-uniform weights / zero bias (embedding_...py:188-211), same on every rank.  Tied weights: the free tensors and
        the biases have the bits of the untied init for that seed; the decoder matrices are mirrors (load_params)."""
        g = torch.Generator(device="cpu")
        g.manual_seed(seed)
        ps = []
        for (k, n, _) in self.engine.schedule:
            a = (6.0 / (k + n)) ** 0.5
            ps.append(((torch.rand((n, k), generator=g) * 2 - 1) * a, torch.zeros(n)))
        self.load_params(ps)

    def params(self, average=False):
        """[(W, b)] views of the parameters; average=True: of the weight average, synchronised first (with tied weights its
        decoder matrices are then mirrors of its encoder's)."""
        if average:
            return self.average_params()
        return [(self.engine.weight(l), self.engine.bias(l)) for l in range(self.engine.L)]

    def average_params(self):
        return [(self.engine.average_weight(l), self.engine.average_bias(l)) for l in range(self.engine.L)]

    def load_average(self, params):
        """params: [(W, b)] as load_params takes them, into the weight average (a restored run)."""
        self.engine.load_average(params)

    def reset_average(self):
        """weight average <- the current parameters."""
        self.engine.reset_average()

    # ---- steps ---------------------------------------------------------------------------
    def _batch(self, row_idx, run):
        if self.mask_to_use is not None and run is not None:
            # id = mask_to_use[row][run] is looked up inside the kernels
            return self.engine.make_batch(self.data, row_idx, None, self.mask_table, mask_to_use=self.mask_to_use, run=run)
        return self.engine.make_batch(self.data, row_idx, None, None)

    def train_batch(self, row_idx, run=0, mask_id=None, global_rows=None):
        """One optimizer step on rows `row_idx` (int32 device tensor) of the resident dataset.
        global_rows: rows of the whole minibatch over all ranks (default: B * world)."""
        eng = self.engine
        if self.use_graph:
            caller = torch.cuda.current_stream(self.device)
            self._graph_stream.wait_stream(caller)
            with torch.cuda.stream(self._graph_stream):
                n = int(row_idx.numel())
                self._idx_buf[:n].copy_(row_idx)
                if mask_id is not None:
                    self._mid_buf[:n].copy_(mask_id)
                    batch = eng.make_batch(self.data, self._idx_buf[:n], self._mid_buf[:n], self.mask_table)
                else:
                    batch = self._batch(self._idx_buf[:n], run)
                B = batch.B
                hyper = eng.hyper(self.lr, self.weight_decay, self.clip,
                                  global_rows=B * self.world if global_rows is None else global_rows)
                eng.train_step(batch, hyper, graph=True)
            caller.wait_stream(self._graph_stream)
            self._keep = batch
            self._note_train_step(B)
            return B
        if mask_id is None:
            batch = self._batch(row_idx, run)
        else:
            batch = eng.make_batch(self.data, row_idx, mask_id, self.mask_table)
        B = batch.B
        hyper = eng.hyper(self.lr, self.weight_decay, self.clip,
                          global_rows=B * self.world if global_rows is None else global_rows)
        if self.dp is None:
            eng.train_step(batch, hyper)
        else:
            self.dp.train_step(batch, hyper, B)
        self._keep = batch  # keep the ctypes struct (and its tensors) alive until the next call
        self._note_train_step(B)
        return B

    def last_output(self):
        """The [B, io] fp32 reconstruction of the last train_batch, a view of the engine's work space: valid until the next call
        that runs a forward.  HipError when that step did not store y (a bf16 step whose loss rode in the last GEMM's epilogue
        or in the chain kernel), or before the first step."""
        B = self.__dict__.get("_last_train_B")
        if not B:
            raise HipError("last_output(): no train_batch has run")
        if not self._last_train_stored_y:
            raise HipError("last_output(): the last training step did not store its reconstruction (the bf16 step with the plain "
                           "mean squared error folds the loss into the last GEMM); set a criterion, or use eval_batch(want_y=True)")
        return self.engine.output_view(B)

    def _note_train_step(self, B):
        """What last_output() needs of the step just issued: its rows, and whether it stored y - the engine's answer, read off the
        step plan the step followed (the data-parallel forms never take the fused-loss epilogue's carried finish, but store y
        under the same rule)."""
        self._last_train_B = int(B)
        ask = getattr(self.engine, "step_stores_output", None)         # (an engine stand-in without the query: nothing to read back)
        self._last_train_stored_y = bool(ask(B)) if ask is not None else False

    def _refuse_slot_feature(self, who):
        if getattr(self.engine, "variable_loss", None) is not None:
            raise HipError("%s is an embedding-slot feature: it is not supported while a VariableLoss is set (rows made of "
                           "variables have no equal-width slots)" % who)

    def eval_batch(self, row_idx, run=0, want_y=False, weights="live"):
        """weights: "live" = the parameters the last step left, "average" = the weight average (HipError when none is kept)."""
        batch = self._batch(row_idx, run)
        y = (torch.empty((batch.B, self.data.shape[1]), dtype=torch.float32, device=self.device)
             if want_y else None)
        self.engine.eval_step(batch, y, weights=weights)
        self._keep = batch
        return y

    def _slots(self):
        """(S, E): from `n_slots`, else from the Corrupter table (row 0 = the 1-subset {slot 0}: its zeros are one slot)."""
        io = int(self.data.shape[1])
        if self.n_slots:
            S = int(self.n_slots)
        elif self.mask_table is not None:
            S = io // int((self.mask_table[0] == 0).sum())
        else:
            raise HipError("complete(): the trainer has no mask table; construct it with n_slots")
        if S < 1 or io % S:
            raise HipError("complete(): %d slots do not divide io %d" % (S, io))
        return S, io // S

    def complete(self, row_idx, slot, k, exclude_self=False, distinct=True, candidates=None, chunk=8192, weights="live"):
        """Complementarity inference: blank slot `slot` of dataset rows `row_idx`, run the eval forward, and return the k
        resident-dataset rows whose slot is closest (cosine) to the reconstruction: (idx LongTensor [B, k], score FloatTensor
        [B, k]), ordered as tool.ComplementRetriever.topk.  Mask id c is the 1-subset {c} of the Corrupter's table order
        (the trainer's own S x io table when it has none), so the result does not depend on the mask run.  exclude_self:
        never return a row's own item.  The metric sums of the engine are left as they were.
        With a presence table only rows that HAVE the slot are candidates (intersected with `candidates`); a query row that
        lacks the slot is the normal case; a slot no candidate row has gives (-1, -inf) everywhere.
        weights: "live", or "average" to reconstruct with the weight average."""
        self._refuse_slot_feature("complete()")
        from .tool.criteria import ComplementRetriever
        S, E = self._slots()
        if isinstance(slot, bool) or not isinstance(slot, int) or not 0 <= slot < S:
            raise HipError("complete(): slot must be an int in [0, %d), got %r" % (S, slot))
        idx = torch.as_tensor(row_idx, dtype=torch.int32).to(self.device).contiguous().reshape(-1)
        table = self.mask_table
        if table is None:
            if getattr(self, "_own_table", None) is None:
                t = torch.ones((S, S * E), dtype=torch.uint8)
                for c in range(S):
                    t[c, c * E:(c + 1) * E] = 0
                self._own_table = t.to(self.device)
            table = self._own_table
        cand = None if candidates is None else tuple(sorted(set(int(i) for i in candidates)))
        B = int(idx.numel())
        pslot = None
        if self.presence is not None:
            # the slot's inventory is the rows that have it: one retriever per (slot, subset)
            pslot = slot
            has = self.presence.table[:, slot] != 0
            cand = tuple(int(i) for i in (has.nonzero()[0] if cand is None else [i for i in cand if 0 <= i < has.shape[0] and has[i]]))
            if not cand:
                return (torch.full((B, int(k)), -1, dtype=torch.long, device=self.device),
                        torch.full((B, int(k)), float("-inf"), dtype=torch.float32, device=self.device))
        key = (bool(distinct), cand, pslot)
        cache = self.__dict__.setdefault("_retrievers", {})
        if key not in cache:
            inv = _ResidentInventory(self.data, S, E)
            cache[key] = ComplementRetriever(inv, self.device, candidates=key[1], distinct=key[0])
        ret = cache[key]
        mask_id = torch.full((B,), slot, dtype=torch.int32, device=self.device)
        batch = self.engine.make_batch(self.data, idx, mask_id, table)
        y = torch.empty((B, self.data.shape[1]), dtype=torch.float32, device=self.device)
        sums = self.engine.scalars.clone()
        self.engine.eval_step(batch, y, weights=weights)
        self.engine.scalars.copy_(sums)                     # (the eval step adds into the epoch's metric sums)
        self._keep = batch
        ret._check_args(y, slot, k, idx if exclude_self else None, chunk)
        # the blanked slot reaches the kernels through the same mask table as the forward (codae_complete_topk's mask route)
        return ret._device_topk(y, int(k), idx if exclude_self else None, int(chunk), mask_id=mask_id, mask_table=table)

    def retrieval_metrics(self, validation_indices, ks=(1, 5, 10, 50), distinct=True):
        """A tool.RetrievalMetrics over the resident data, bound to this trainer's presence table, mask table and mask_to_use:
        its add(y, row_idx, run=0) takes the output of eval_batch(row_idx, run, want_y=True) and needs nothing else.  hit@k, MRR
        and the position histogram of every blanked slot a validation row has, incomplete rows included."""
        self._refuse_slot_feature("retrieval_metrics()")
        from .tool.criteria import RetrievalMetrics
        if self.mask_table is None or self.mask_to_use is None:
            raise HipError("retrieval_metrics(): the trainer has no mask tables")
        S, E = self._slots()
        rm = RetrievalMetrics(_ResidentInventory(self.data, S, E), validation_indices, self.device, ks=ks,
                              presence=self.presence, distinct=distinct)
        rm.mask_table, rm.mask_to_use = self.mask_table, self.mask_to_use
        return rm

    # ---- assembled outfits (include/codae_hip.h, "Assembled outfits and compatibility") ------------------------------------
    def _outfit_items(self, items, who):
        """items -> a contiguous int32 [Q, S] device tensor; a host tensor / list is checked against the dataset's rows first (on the
        device an entry past the last row counts as absent: the kernels never read through an unchecked index)."""
        S, _ = self._slots()
        t = items if torch.is_tensor(items) else torch.as_tensor(items)
        if t.dim() != 2 or t.shape[1] != S or t.shape[0] < 1 or t.dtype.is_floating_point or t.dtype == torch.bool:
            raise HipError("%s: items must be an integer [Q, %d] tensor with Q >= 1, got %s %s" % (who, S, t.dtype, tuple(t.shape)))
        if t.device.type == "cpu" and int(t.max()) >= int(self.data.shape[0]):
            raise HipError("%s: items name row %d, the dataset has %d" % (who, int(t.max()), int(self.data.shape[0])))
        return t.to(device=self.device, dtype=torch.int32).contiguous()

    def score_outfits(self, items, weights="live"):
        """Score assembled outfits: items integer [Q, S], items[q][s] = the dataset row whose slot-s item outfit q holds, negative =
        none (with a presence table a slot the row lacks is absent too).  Every present item is left out in turn, reconstructed by
        the evaluation forward from the others (weights: "live" or "average") and compared with itself -> {"score": [Q] the mean
        cosine (NaN with fewer than two items), "cos": [Q, S], "sq": [Q, S] the squared error, "n_present": [Q] int32}, device
        tensors.  Runs in chunks of max_batch // S outfits without a host synchronisation; epoch_sums(), the parameters and the
        optimizer state stay exactly as they were."""
        self._refuse_slot_feature("score_outfits()")
        S, _ = self._slots()
        it = self._outfit_items(items, "score_outfits()")
        per = self.engine.max_batch // S
        if per < 1:
            raise HipError("score_outfits(): max_batch %d holds no outfit of %d slots" % (self.engine.max_batch, S))
        parts = [self.engine.score_outfits(self.data, it[o:o + per], weights=weights) for o in range(0, int(it.shape[0]), per)]
        if len(parts) == 1:
            return parts[0]
        return {k: torch.cat([p[k] for p in parts]) for k in parts[0]}

    def complete_items(self, items, slot, k, exclude_items=True, distinct=True, candidates=None, chunk=8192, weights="live"):
        """complete() for assembled outfits: slot `slot` of every outfit is blanked - whatever items[:, slot] holds -, the rest runs
        through the evaluation forward and the reconstruction is ranked against the resident rows' items of that slot, with
        complete()'s contract: (idx LongTensor [Q, k], score FloatTensor [Q, k]), ordering, (-1, -inf) padding, presence-restricted
        candidates.  exclude_items: never return the item the query itself names in items[:, slot] (with `distinct`, the item that
        row belongs to)."""
        self._refuse_slot_feature("complete_items()")
        from .tool.compat import Compatibility
        from .tool.criteria import ComplementRetriever
        S, E = self._slots()
        if isinstance(slot, bool) or not isinstance(slot, int) or not 0 <= slot < S:
            raise HipError("complete_items(): slot must be an int in [0, %d), got %r" % (S, slot))
        it = self._outfit_items(items, "complete_items()")
        Q = int(it.shape[0])
        if Q > self.engine.max_batch:
            raise HipError("complete_items(): %d outfits exceed max_batch %d" % (Q, self.engine.max_batch))
        cand = None if candidates is None else tuple(sorted(set(int(i) for i in candidates)))
        pslot = None
        if self.presence is not None:
            pslot = slot
            has = self.presence.table[:, slot] != 0
            cand = tuple(int(i) for i in (has.nonzero()[0] if cand is None else [i for i in cand if 0 <= i < has.shape[0] and has[i]]))
            if not cand:
                return (torch.full((Q, int(k)), -1, dtype=torch.long, device=self.device),
                        torch.full((Q, int(k)), float("-inf"), dtype=torch.float32, device=self.device))
        key = (bool(distinct), cand, pslot)
        cache = self.__dict__.setdefault("_retrievers", {})
        if key not in cache:
            cache[key] = ComplementRetriever(_ResidentInventory(self.data, S, E), self.device, candidates=key[1], distinct=key[0])
        ret = cache[key]
        blank = torch.full((Q,), slot, dtype=torch.int32, device=self.device)
        x = Compatibility.assemble(self.data, it, blank=blank, presence=self.presence)
        y = self.engine.forward(x, weights=weights)          # the evaluation's forward launches; no loss kernel, no metric sums
        exclude = it[:, slot].contiguous() if exclude_items else None
        ret._check_args(y, slot, k, exclude, chunk)
        return ret._device_topk(y, int(k), exclude, int(chunk), slot=slot)

    def compatibility_metrics(self, validation_indices, negatives=1, seed=0, distinct=True):
        """A tool.CompatibilityMetrics over the resident data, bound to this trainer and its presence table: add_batch(row_idx,
        weights=...) scores the outfits of those validation rows and their swapped negatives; total() gives the AUC and the paired
        accuracy."""
        self._refuse_slot_feature("compatibility_metrics()")
        from .tool.compat import CompatibilityMetrics
        S, E = self._slots()
        cm = CompatibilityMetrics(_ResidentInventory(self.data, S, E), validation_indices, self.device, negatives=negatives, seed=seed,
                                  presence=self.presence, distinct=distinct)
        cm.trainer = self
        return cm

    # ---- outfit codes (include/codae_hip.h, "Outfit codes"; codae/tool/codes.py) ------------------------------------------------
    @property
    def code_layers(self):
        """k of the code h_k: the index, plus one, of the lowest hidden Linear without an activation - the z layer of every stack
        linear_stack builds.  HipError when the stack has no such layer (encode(..., layer=k) then names it)."""
        from .tool.codes import code_layers
        return code_layers([(s[0], s[1], a) for s, a in zip(self.engine.schedule, self.engine.layer_activations())])

    def _code_layer(self, who, layer):
        from .tool.codes import check_layer
        return self.code_layers if layer is None else check_layer(who, layer, self.engine.L)

    def code_width(self, layer=None):
        """Z: the width of h_k, k = layer or code_layers."""
        return int(self.engine.schedule[self._code_layer("code_width()", layer) - 1][1])

    def _blank_vector(self, who, blank, Q):
        """blank -> None or an int32 [Q] device tensor (negative: none); a device tensor is not read back"""
        if blank is None:
            return None
        S, _ = self._slots()
        if torch.is_tensor(blank):
            if blank.dim() != 1 or blank.shape[0] != Q or blank.dtype.is_floating_point or blank.dtype == torch.bool:
                raise HipError("%s: blank must be None, an int slot or an integer [%d] tensor" % (who, Q))
            return blank.to(device=self.device, dtype=torch.int32).contiguous()
        if isinstance(blank, bool) or not isinstance(blank, int) or not -1 <= blank < S:
            raise HipError("%s: blank must be None, an int slot in [0, %d) or an integer [Q] tensor, got %r" % (who, S, blank))
        return torch.full((Q,), blank, dtype=torch.int32, device=self.device)

    def _encode_into(self, it, bl, k, weights, code, norm):
        """codes of the assembled outfits it [Q, S] (slot bl[q] blanked) into code [Q, Z] and norm [Q] (or None), in chunks of
        max_batch, every chunk written at its offset; no host synchronisation"""
        from .tool.compat import Compatibility
        per = self.engine.max_batch
        for o in range(0, int(it.shape[0]), per):
            x = Compatibility.assemble(self.data, it[o:o + per], blank=None if bl is None else bl[o:o + per], presence=self.presence)
            self.engine.encode(x, k, want_norm=norm is not None, weights=weights, out=code[o:o + per],
                               norm_out=None if norm is None else norm[o:o + per])

    def encode_items(self, items, blank=None, layer=None, weights="live", want_norm=False):
        """The codes of assembled outfits: items integer [Q, S] in score_outfits' convention (negative = no item; with a presence
        table a slot the row lacks is absent), assembled as complete_items assembles them - absent and blanked slots are zeros -
        and run through the first k Linears of the evaluation forward with their skips and norms (k = layer, default
        code_layers; weights: "live" or "average") -> [Q, Z] fp32 on the device, (codes, norms [Q]) with want_norm.  bf16 engine:
        bf16 values widened to fp32.  blank: None (the whole outfit), an int slot, or an integer [Q] tensor with -1 for none - a
        partial outfit ("this top and these shoes, any bottom").  Chunks of max_batch, no host synchronisation; epoch_sums(), the
        parameters and the optimizer state stay exactly as they were."""
        self._refuse_slot_feature("encode_items()")
        k = self._code_layer("encode()", layer)
        it = self._outfit_items(items, "encode()")
        Q = int(it.shape[0])
        bl = self._blank_vector("encode()", blank, Q)
        code = torch.empty((Q, self.code_width(k)), dtype=torch.float32, device=self.device)
        norm = torch.empty(Q, dtype=torch.float32, device=self.device) if want_norm else None
        self._encode_into(it, bl, k, weights, code, norm)
        return (code, norm) if want_norm else code

    def encode(self, row_idx, blank=None, layer=None, weights="live", want_norm=False):
        """encode_items for resident rows: row r is the outfit [r, r, .., r]."""
        S, _ = self._slots()
        idx = torch.as_tensor(row_idx).reshape(-1)
        if idx.dtype.is_floating_point or idx.dtype == torch.bool:
            raise HipError("encode(): row_idx must be integer dataset rows, got %s" % idx.dtype)
        return self.encode_items(idx[:, None].expand(-1, S), blank=blank, layer=layer, weights=weights, want_norm=want_norm)

    def decode(self, z, layer=None, weights="live"):
        """The reconstruction of codes: Linears k .. L - 1 on z [Q, Z] (k = layer, default code_layers) with their skips and norms
        -> [Q, io] fp32 on the device.  decode(encode(rows, blank=c)) has the bits of eval_batch(rows, want_y=True) under the
        one-slot mask {c} at the same batch size.  Chunked as encode."""
        k = self._code_layer("decode()", layer)
        Z = int(self.engine.schedule[k][0])
        if not torch.is_tensor(z) or z.dim() != 2 or z.shape[1] != Z or z.shape[0] < 1:
            raise HipError("decode(): codes must be a [Q, %d] tensor with Q >= 1, got %s" % (Z, tuple(z.shape) if torch.is_tensor(z) else type(z).__name__))
        z = z.to(self.device)
        per = self.engine.max_batch
        parts = [self.engine.decode(z[o:o + per], k, weights=weights) for o in range(0, int(z.shape[0]), per)]
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def code_index(self, rows=None, blank=None, layer=None, weights="live", distinct=True):
        """A tool.OutfitCodes over the codes of dataset rows `rows` (None = every resident row): the bank [M, Z], encoded chunk by
        chunk into one preallocated tensor, its norms from the export kernel's same pass, and the rows the entries stand for.
        similar(query, k, exclude) then ranks it against query codes from encode / encode_items."""
        self._refuse_slot_feature("code_index()")
        from .hip import PREC_BF16
        from .tool.codes import OutfitCodes
        k = self._code_layer("code_index()", layer)
        S, _ = self._slots()
        if rows is None:
            idx = torch.arange(int(self.data.shape[0]), dtype=torch.int32, device=self.device)
        else:
            idx = torch.as_tensor(rows).reshape(-1)
            if idx.dtype.is_floating_point or idx.dtype == torch.bool:
                raise HipError("code_index(): rows must be integer dataset rows, got %s" % idx.dtype)
        it = self._outfit_items(idx[:, None].expand(-1, S), "code_index()")
        M = int(it.shape[0])
        bl = self._blank_vector("code_index()", blank, M)
        bank = torch.empty((M, self.code_width(k)), dtype=torch.float32, device=self.device)
        norm = torch.empty(M, dtype=torch.float32, device=self.device)
        self._encode_into(it, bl, k, weights, bank, norm)
        index = OutfitCodes(bank, rows=None if rows is None else idx, norm=norm, layer=k, distinct=distinct)
        index.precision = "bf16" if self.engine.precision == PREC_BF16 else "f32"      # (cluster()'s default operand type)
        return index

    def epoch_sums(self, reset=True, reduce=True):
        """(sum (x-y)^2, sum (1-fmask)(x-y)^2) accumulated since the last reset (summed over the
        ranks when `reduce`)."""
        s = self.engine.scalars[:2].clone()
        if self.dp and reduce:
            self.dp.reduce_scalars(s)
        if reset:
            self.engine.zero_metric_sums()
        s = s.cpu()
        return float(s[0]), float(s[1])

    def last_loss_and_grad_norm(self):
        _, _, gsq, loss = self.engine.read_scalars()
        return loss, gsq ** 0.5

    # ---- checkpoint and resume (include/codae_hip.h, "State digest"; codae/tool/checkpoint.py) --------------------------------------
    def _refuse_sharded(self, who):
        if self.dp is not None and self.dp.sharded:
            raise HipError("%s: the sharded update is not supported: the moments of a rank live in its shards" % who)

    def _state_meta(self):
        """What the file records beside the tensors: the structure load() checks, and the training options for information."""
        eng = self.engine
        opt, avg = eng.optimizer, eng.weight_average
        from .tool.norm import meta_record
        norm = meta_record(getattr(eng, "norm", None), getattr(eng, "norm_layers", None))
        meta = {
            "step_count": int(eng.step_count),
            "schedule": [[k, n, bool(r)] for k, n, r in eng.schedule],
            "n_param": int(eng.n_param),
            "precision": "bf16" if eng.precision == 1 else "f32",
            "activation": None if eng.activation is None else [list(a) for a in eng.activation],
            "tied_weights": bool(eng.tied_weights),
            "residual": list(eng.residual_layers) or None,       # the skipped layers: part of the model, load() checks them
            "optimizer": "adam" if opt is None else opt.kind,
            "amsgrad": bool(opt is not None and opt.amsgrad),
            "weight_average": None if avg is None or avg.is_default else
            {"kind": avg.kind, "decay": avg.decay, "debias": avg.debias, "start": avg.start, "every": avg.every},
            "optional": [n for n in ("adam_vmax", "weight_avg") if getattr(eng, n) is not None],
            "lr": float(self.lr), "weight_decay": float(self.weight_decay), "clip": float(self.clip or 0.0),
            # construction options of the trainer that wrote the file: load() does not read them
            "options": {n: (None if getattr(eng, n) is None else repr(getattr(eng, n)))
                        for n in ("input_noise", "loss_emphasis", "hidden_dropout", "recon_loss", "slot_contrast", "optimizer",
                                  "slot_presence")},
        }
        variable_loss = getattr(eng, "variable_loss", None)
        if variable_loss is not None:          # (informational, and only when it is on: the files of other runs keep their bytes)
            meta["options"]["variable_loss"] = variable_loss.describe()
        if norm is not None:          # (written only when a norm is on: the files of runs without one keep their bytes)
            meta["norm"] = norm       # {kind, eps, layers}: part of the model, load() checks it
        from .tool.sparse import meta_record as sparse_record
        sparse = sparse_record(getattr(eng, "sparse_code", None), getattr(eng, "sparse_resolved", None))
        if sparse is not None:        # (written only when it is on, as the norm's)
            meta["sparse_code"] = sparse      # {keep, layer}: part of the model, load() checks it
        return meta

    def snapshot(self):
        """Freeze the state as it is behind the steps enqueued so far, without blocking the host: on the current stream, behind
        engine.join(), one codae_state_digest(src, staging) per state tensor - one pass that fingerprints it and copies it to a device
        staging buffer -, then on a side stream the copies into pinned host buffers and an event.  Steps enqueued afterwards overlap
        the device-to-host copy.  -> a Snapshot: write(path) waits for the event and writes the file, release() drops it.  The staging
        set is allocated on first use and kept; there is one, so a second snapshot() while one is neither written nor released is
        refused (HipError).  Data parallel: every rank may take one; save() writes on rank 0 only."""
        self._refuse_sharded("snapshot()")
        if getattr(self, "_snap_live", None) is not None:
            raise HipError("snapshot(): the previous snapshot is neither written nor released (there is one staging set)")
        eng = self.engine
        with torch.cuda.device(self.device):
            st = eng.state_tensors()                     # (joins the engine's side stream into the current one)
            sig = tuple((n, t.dtype, t.numel()) for n, t in st.items())
            if getattr(self, "_snap_sig", None) != sig:
                self._snap_dev = {n: torch.empty_like(t) for n, t in st.items()}
                self._snap_host = {n: torch.empty(t.numel(), dtype=t.dtype).pin_memory() for n, t in st.items()}
                self._snap_dig = torch.zeros((len(st), 2), dtype=torch.int64, device=self.device)
                self._snap_dig_host = torch.zeros((len(st), 2), dtype=torch.int64).pin_memory()
                self._snap_stream = torch.cuda.Stream(device=self.device)
                self._snap_event = torch.cuda.Event()
                self._snap_sig = sig
            else:
                # a released snapshot's copies may still be reading the staging buffers
                torch.cuda.current_stream(self.device).wait_event(self._snap_event)
            for i, (n, t) in enumerate(st.items()):
                eng.digest_into(t, self._snap_dig[i], dst=self._snap_dev[n])
            self._snap_stream.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(self._snap_stream):
                for n in st:
                    self._snap_host[n].copy_(self._snap_dev[n], non_blocking=True)
                self._snap_dig_host.copy_(self._snap_dig, non_blocking=True)
                self._snap_event.record(self._snap_stream)
        self._snap_live = Snapshot(self, list(st), self._state_meta())
        return self._snap_live

    def save(self, path, extra=None):
        """snapshot().write(path): the file of codae/tool/checkpoint.py.  Data parallel: a collective every rank calls; rank 0 writes,
        every other rank returns None (the replicas hold the same state: DataParallel.replicas_agree()).  The two running epoch sums
        of the scalars are each rank's own partial sums: the file gets their sum over the ranks, and load() gives it to rank 0 alone,
        so epoch_sums() goes on as in the run that was not interrupted.  -> bytes written."""
        self._refuse_sharded("save()")
        sums = None
        if self.dp is not None and self.dp.world > 1:
            sums = self.dp.reduce_scalars(self.engine.scalars[:2].clone()).cpu()
            if self.dp.rank != 0:
                return None
        return self.snapshot().write(path, extra=extra, metric_sums=sums)

    def state_digest(self):
        """{name: (out0, out1)} of every state tensor, computed on the device, and "all": the digest of the concatenated little-endian
        per-tensor digests in that order.  Synchronises."""
        from .tool.checkpoint import StateDigest
        with torch.cuda.device(self.device):
            d = self.engine.digests()
        d["all"] = StateDigest.combine(d.values())
        return d

    def _check_structure(self, path, tensors, meta, strict, need=("params", "adam_m", "adam_v", "scalars")):
        eng = self.engine

        def refuse(piece, what):
            raise HipError("load(%s): %s: %s" % (path, piece, what))
        if [list(x) for x in meta.get("schedule", [])] != [[k, n, bool(r)] for k, n, r in eng.schedule]:
            refuse("schedule", "the file was written for %r, this trainer runs %r" % (meta.get("schedule"), eng.schedule))
        if bool(meta.get("tied_weights")) != bool(eng.tied_weights):
            refuse("tied_weights", "the file was written with tied weights %s, this trainer has them %s"
                   % ("on" if meta.get("tied_weights") else "off", "on" if eng.tied_weights else "off"))
        from .tool.residual import meta_mismatch
        why = meta_mismatch(meta, eng.residual_layers)
        if why is not None:
            refuse("residual", why)
        from .tool.norm import meta_mismatch as norm_mismatch
        why = norm_mismatch(meta, getattr(eng, "norm", None), getattr(eng, "norm_layers", None))
        if why is not None:
            refuse("norm", why)
        from .tool.sparse import meta_mismatch as sparse_mismatch
        why = sparse_mismatch(meta, getattr(eng, "sparse_code", None), getattr(eng, "sparse_resolved", None))
        if why is not None:
            refuse("sparse_code", why)
        live = eng.state_tensors()
        for n in need:
            if n not in tensors:
                refuse(n, "the file does not hold it")
        for n, t in tensors.items():
            if n in live and (t.size != live[n].numel() or "torch." + t.dtype.name != str(live[n].dtype)):
                refuse(n, "the file holds %d x %s, this trainer %d x %s" % (t.size, t.dtype, live[n].numel(), live[n].dtype))
            if n not in meta.get("digests", {}):
                refuse(n, "'meta' records no digest for it")
        if "adam_vmax" in need or (eng.optimizer is not None and eng.optimizer.amsgrad and "adam_m" in need):
            if "adam_vmax" not in tensors:
                refuse("adam_vmax", "AMSGrad is on and the file does not hold its running maximum")
        # lamb / lars keep other moments than the kinds before them (lars: a momentum buffer of ratio-scaled steps, no v): a file and
        # a trainer that differ in kind are refused wherever one of the two is a trust kind; the other kinds keep loading each other
        mine, theirs = "adam" if eng.optimizer is None else eng.optimizer.kind, meta.get("optimizer", "adam")
        if "adam_m" in need and mine != theirs and ({mine, theirs} & {"lamb", "lars"}):
            refuse("optimizer", "the file was written under %r, this trainer runs %r" % (theirs, mine))
        if strict and eng.averaging() and "adam_m" in need and "weight_avg" not in tensors:
            refuse("weight_avg", "weight averaging is on and the file holds no average (strict=False starts it from the parameters)")
        if strict and "adam_m" in need:
            prec = "bf16" if eng.precision == 1 else "f32"
            if meta.get("precision") != prec:
                refuse("precision", "the file was written by a %s engine, this one is %s" % (meta.get("precision"), prec))
            act = None if eng.activation is None else [list(a) for a in eng.activation]
            if meta.get("activation") != act:
                refuse("activation", "the file was written with %r, this trainer runs %r" % (meta.get("activation"), act))

    def _upload_verified(self, path, tensors, meta, names):
        """Upload the named tensors into temporaries, digest each ON THE DEVICE and compare with `meta`: -> {name: device tensor}, or
        HipError naming the first tensor that differs (nothing is kept)."""
        from .tool.checkpoint import StateDigest
        eng = self.engine
        with torch.cuda.device(self.device):
            tmp = {n: torch.from_numpy(tensors[n].reshape(-1)).to(self.device) for n in names}
            out = torch.empty((len(names), 2), dtype=torch.int64, device=self.device)
            for i, n in enumerate(names):
                eng.digest_into(tmp[n], out[i])
            got = eng._digest_pairs(out.cpu())
        for n, d in zip(names, got):
            if StateDigest.hex(d) != meta["digests"][n]:
                raise HipError("load(%s): tensor '%s' has digest %s on the device, the file recorded %s"
                               % (path, n, StateDigest.hex(d), meta["digests"][n]))
        return tmp

    def load(self, path, strict=True):
        """Restore the state save() wrote, so that the next step is bit for bit the step the writing run took next.  Structure first
        (HipError naming the piece; the trainer stays as it was): the schedule and parameter count, tied weights on in one and off in
        the other, residual connections around other layers, another norm or another sparse code (a file without the record has none), adam_vmax missing while AMSGrad is on; under `strict` also an average missing while averaging is on, another
        precision or activation, and optional tensors this trainer does not keep.  Then every tensor is uploaded into a temporary,
        digested on the device and compared with the file's record (HipError naming the tensor; nothing is kept), and only then
        copied over the live state.  On success: step_count is set, the scalars are the file's, the bf16 shadows are rebuilt
        (sync_shadows) and the average's images marked stale; the average is NOT reset.  Training options (noise, emphasis, criterion,
        contrast, dropout, presence, optimizer) belong to this trainer's construction, not to the file.  Data parallel: every rank
        reads the file.  -> the file's `meta`."""
        from .tool.checkpoint import CheckpointError, read_checkpoint
        self._refuse_sharded("load()")
        try:
            tensors, meta = read_checkpoint(path, verify=False)
        except CheckpointError as e:
            raise HipError(str(e))
        eng = self.engine
        self._check_structure(path, tensors, meta, strict)
        live = eng.state_tensors()
        if strict:
            for n in tensors:
                if n not in live:
                    raise HipError("load(%s): %s: the file holds it and this trainer does not keep it (strict=False ignores it)" % (path, n))
        names = [n for n in live if n in tensors]
        tmp = self._upload_verified(path, tensors, meta, names)
        with torch.no_grad():
            for n in names:
                live[n].copy_(tmp[n])
            if "weight_avg" in live and "weight_avg" not in tensors:
                live["weight_avg"].copy_(live["params"])
            if self.dp is not None and self.dp.world > 1 and self.dp.rank != 0:
                eng.scalars[:2].zero_()                    # (the file's epoch sums are the sum over the ranks: rank 0 carries them)
        eng.set_step_count(int(meta["step_count"]))
        eng.sync_shadows()
        eng._avg_stale = True
        return meta

    @classmethod
    def load_for_inference(cls, path, data, mask_table_u8=None, mask_to_use_i32=None, n_slots=None, max_batch=8192, device="cuda:0",
                           presence=None):
        """A trainer built from the file's own record (schedule, precision, activation, tied weights, skips, norm, sparse code, the kind of average) over
        `data`, holding the file's parameters and - when it has one - weight average, each verified on the device as load() does:
        eval_batch, complete*, score_outfits and the metrics give what the writing process gave.  The moments are neither read nor
        required (a file stripped of them loads)."""
        from .tool.average import WeightAverage
        from .tool.checkpoint import CheckpointError, read_checkpoint
        from .tool.residual import Residual
        from .tool.norm import norm_from_meta
        from .tool.sparse import sparse_from_meta
        try:
            tensors, meta = read_checkpoint(path, verify=False)
        except CheckpointError as e:
            raise HipError(str(e))
        act = meta.get("activation")
        tr = cls([tuple(x) for x in meta["schedule"]], data, mask_table_u8, mask_to_use_i32, meta.get("lr", 0.0), meta.get("weight_decay", 0.0),
                 clip=meta.get("clip", 0.0), max_batch=max_batch, precision=meta.get("precision", "bf16"), device=device,
                 activation=None if act is None else [tuple(a) for a in act], n_slots=n_slots, presence=presence,
                 tied_weights=bool(meta.get("tied_weights")), residual=Residual(meta["residual"]) if meta.get("residual") else None,
                 norm=norm_from_meta(meta), sparse_code=sparse_from_meta(meta))
        eng = tr.engine
        names = ["params"]
        wa = meta.get("weight_average")
        if "weight_avg" in tensors:
            eng.set_weight_average(WeightAverage(**wa) if wa else WeightAverage())
            names.append("weight_avg")
        tr._check_structure(path, tensors, meta, False, need=("params",))
        tmp = tr._upload_verified(path, tensors, meta, names)
        live = eng.state_tensors()
        with torch.no_grad():
            for n in names:
                live[n].copy_(tmp[n])
        eng.set_step_count(int(meta["step_count"]))
        eng.sync_shadows()
        eng._avg_stale = True
        return tr


class Snapshot:
    """The state of a HipEmbeddingTrainer at one point of its stream, on its way to pinned host memory (HipEmbeddingTrainer.snapshot).
    write(path) waits for the copies and writes the checkpoint file; release() drops it.  Either frees the trainer's staging set."""

    def __init__(self, trainer, names, meta):
        self._trainer, self._names, self.meta = trainer, names, meta

    def _live(self):
        if self._trainer is None or self._trainer._snap_live is not self:
            raise HipError("Snapshot: already written or released")

    def wait(self):
        """Block until the copies have landed (write() does)."""
        self._live()
        self._trainer._snap_event.synchronize()

    def digests(self):
        """{name: (out0, out1)} as the device computed them while copying; waits for the copies."""
        self.wait()
        from .hip.engine import DaeEngine
        return dict(zip(self._names, DaeEngine._digest_pairs(self._trainer._snap_dig_host)))

    def write(self, path, extra=None, metric_sums=None):
        """-> bytes written.  extra: a JSON-serialisable dict of the caller's, kept in meta["extra"].  metric_sums: two float64 that
        replace the running epoch sums in the file's scalars (save() on data-parallel replicas: the sum over the ranks)."""
        from .tool.checkpoint import StateDigest, write_checkpoint
        dig = self.digests()
        tr = self._trainer
        if metric_sums is not None:
            tr._snap_host["scalars"][:2] = torch.as_tensor(metric_sums, dtype=torch.float64)
            dig["scalars"] = StateDigest.get(tr._snap_host["scalars"].numpy())
        meta = dict(self.meta)
        meta["digests"] = {n: StateDigest.hex(d) for n, d in dig.items()}
        meta["all"] = StateDigest.hex(StateDigest.combine(dig.values()))
        meta["extra"] = {} if extra is None else extra
        try:
            return write_checkpoint(path, {n: tr._snap_host[n].numpy() for n in self._names}, meta)
        finally:
            self.release()

    def release(self):
        tr, self._trainer = self._trainer, None
        if tr is not None and tr._snap_live is self:
            tr._snap_live = None
