"""Sampled-softmax slot contrast: an additional term of the training loss on top of the criterion - the counterpart of
codae_slot_contrast in include/codae_hip.h ("Slot contrast").

The stack fills a blanked slot with an embedding that is then RANKED by cosine against the inventory (RankingLoss,
ComplementRetriever.topk, HipEmbeddingTrainer.complete).  slot_cosine pulls a reconstruction towards its own item; a rank is a
relative quantity, so this term also pushes it away from the other items of the slot: per (row, slot) pair a softmax over the
true item and K negatives sampled from the same inventory (sampled softmax / InfoNCE), all as unit vectors,

    z_0 = cos(x, y) / tau,  z_k = cos(c_k, y) / tau,   l = logsumexp(z_0, z_kept) - z_0,
    L   = L_criterion + weight * sum_{b,s} W l / (rows S)

with the candidates c_k of step t and slot s drawn with replacement by Philox (counter (k / 4, s, t, 256)) and shared by every row
and rank, and a candidate left out for a pair when it IS the pair's item (`distinct`: the same embedding; else the same row).

SlotContrast carries the parameters (as fp32, the type of the C struct), hands them to the HIP engine
(DaeEngine.set_slot_contrast, HipEmbeddingTrainer(contrast=...)) and states the same term in plain torch ops with autograd for the
drop-in loops (loss).
"""
import math

import numpy as np

from ..hip import HipError
from .noise import philox4x32_10

COS_EPS = 1e-8          # CODAE_COS_EPS
MAX_NEG = 4096
MAX_SLOTS = 128
MAX_E = 1024
MIN_TAU = 0.01
COUNTER_WORD = 256      # fourth Philox counter word: input noise uses 0, dropout 1 + layer <= 255


def _number(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise HipError("slot contrast: %s must be a number, got %r" % (name, v))
    v = float(v)
    if not math.isfinite(v) or abs(v) > 3.4e38:
        raise HipError("slot contrast: %s = %r is not finite" % (name, v))
    return float(np.float32(v))


def item_ids(data, n_slots):
    """int64 tensor [S, N]: per slot, the index of every dataset row's item among the slot's distinct embeddings
    (torch.unique(dim=0, return_inverse=True), as RankingLoss and ComplementRetriever group an inventory)."""
    import torch
    N, io = data.shape
    E = io // n_slots
    return torch.stack([torch.unique(data[:, s * E:(s + 1) * E], dim=0, return_inverse=True)[1] for s in range(n_slots)])


class SlotContrast:
    """SlotContrast(negatives=256, temperature=0.1, weight=1.0, seed=0, candidates=None, distinct=True).
    negatives: K in [1, 4096]; temperature: tau >= 0.01; weight >= 0 (0 = off: `is_default`); seed: 64-bit stream id;
    candidates: dataset rows to draw from (default: all); distinct: leave a candidate out of a pair when its slot holds the same
    embedding as the pair's target (False: only when it is the same dataset row)."""

    def __init__(self, negatives=256, temperature=0.1, weight=1.0, seed=0, candidates=None, distinct=True):
        if isinstance(negatives, bool) or not isinstance(negatives, (int, np.integer)) or not 1 <= int(negatives) <= MAX_NEG:
            raise HipError("slot contrast: negatives must be an integer in [1, %d], got %r" % (MAX_NEG, negatives))
        self.negatives = int(negatives)
        self.temperature = _number("temperature", temperature)
        if self.temperature < float(np.float32(MIN_TAU)):
            raise HipError("slot contrast: temperature %r must be >= %g" % (self.temperature, MIN_TAU))
        self.weight = _number("weight", weight)
        if self.weight < 0.0:
            raise HipError("slot contrast: weight %r must be >= 0" % self.weight)
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
            raise HipError("slot contrast: seed must be an integer in [0, 2^64), got %r" % (seed,))
        self.seed = int(seed)
        if not isinstance(distinct, (bool, np.bool_)):
            raise HipError("slot contrast: distinct must be a bool, got %r" % (distinct,))
        self.distinct = bool(distinct)
        self.candidates = None
        if candidates is not None:
            c = np.asarray(candidates.cpu() if hasattr(candidates, "cpu") else candidates)
            if c.ndim != 1 or c.size < 1 or not np.issubdtype(c.dtype, np.integer):
                raise HipError("slot contrast: candidates must be a non-empty 1-d integer array of dataset rows")
            if c.min() < 0 or c.max() >= 2 ** 31:
                raise HipError("slot contrast: candidates must be rows in [0, 2^31)")
            self.candidates = c.astype(np.int32)
        self._ids = None    # (data pointer, shape, S) -> item ids, for loss()

    def __repr__(self):
        return "SlotContrast(negatives=%d, temperature=%r, weight=%r, seed=%d, candidates=%s, distinct=%r)" % (
            self.negatives, self.temperature, self.weight, self.seed,
            None if self.candidates is None else "<%d rows>" % self.candidates.size, self.distinct)

    @property
    def is_default(self):
        return self.weight == 0.0

    def check_rows(self, n_rows):
        if self.candidates is not None and int(self.candidates.max()) >= int(n_rows):
            raise HipError("slot contrast: candidate row %d outside the dataset's [0, %d)" % (int(self.candidates.max()), int(n_rows)))

    @staticmethod
    def _check_slots(n_slots, io=None):
        if n_slots is None or isinstance(n_slots, bool) or not isinstance(n_slots, (int, np.integer)) or not 1 <= int(n_slots) <= MAX_SLOTS:
            raise HipError("slot contrast: n_slots must be in [1, %d], got %r" % (MAX_SLOTS, n_slots))
        if io is not None:
            if int(io) % int(n_slots):
                raise HipError("slot contrast: n_slots %d does not divide io %d" % (int(n_slots), int(io)))
            if int(io) // int(n_slots) > MAX_E:
                raise HipError("slot contrast: E = %d columns per slot, at most %d are supported" % (int(io) // int(n_slots), MAX_E))
        return int(n_slots)

    def candidate_rows(self, step, slot, n_rows):
        """int64 [K]: the dataset rows of the candidates of optimizer step `step` (1-based) and slot `slot`."""
        self.check_rows(n_rows)
        k = np.arange(self.negatives, dtype=np.int64)
        words = philox4x32_10((k // 4, np.int64(slot), np.int64(step) & 0xFFFFFFFF, COUNTER_WORD), (self.seed & 0xFFFFFFFF, self.seed >> 32))
        r = np.stack(words, axis=-1)[np.arange(self.negatives), k % 4].astype(np.uint64)
        P = np.uint64(int(n_rows) if self.candidates is None else self.candidates.size)
        j = ((r * P) >> np.uint64(32)).astype(np.int64)
        return j if self.candidates is None else self.candidates[j].astype(np.int64)

    def as_struct(self, n_slots, n_rows, pool=None, item_id=None, ws=None):
        """The codae_slot_contrast of this setting.  pool / item_id / ws: the device tensors it borrows (int32 [n_pool], int32
        [S, n_rows], uint8 work space) - the caller keeps them alive."""
        from ..hip import SlotContrast as Struct, ptr
        S = self._check_slots(n_slots)
        self.check_rows(n_rows)
        return Struct(S, self.negatives, self.temperature, self.weight, self.seed, int(n_rows), 0 if pool is None else int(pool.numel()),
                      0 if ws is None else int(ws.numel() * ws.element_size()), ptr(pool), ptr(item_id), ptr(ws))

    # ---- a dense batch (drop-in loops) ---------------------------------------------------------------
    def loss(self, input, output, rows, step, data, weight=None, n_slots=None, global_rows=None):
        """weight * sum W l / (rows S) of the dense batch in plain torch ops (differentiable in `output`), on host or HIP tensors:
        the term alone, to be added to the criterion's loss.  input: the clean rows [B, io]; rows [B]: their dataset rows; step:
        the 1-based optimizer step; data [N, io]: the dataset the candidates are drawn from; weight [B, io]: the element weights
        (LossEmphasis.weights(corrupted)), default 1; global_rows: rows of the whole minibatch over all ranks."""
        import torch
        if input.dim() != 2 or input.shape != output.shape:
            raise HipError("SlotContrast.loss: input %s and output %s must be equal [B, io] shapes" % (tuple(input.shape), tuple(output.shape)))
        B, io = input.shape
        S = self._check_slots(n_slots, io)
        E = io // S
        data = torch.as_tensor(data)
        if data.dim() != 2 or data.shape[1] != io:
            raise HipError("SlotContrast.loss: data %s does not have the batch's %d columns" % (tuple(data.shape), io))
        N = int(data.shape[0])
        dev, dt = output.device, output.dtype
        rows_t = torch.as_tensor(np.asarray(rows.cpu() if hasattr(rows, "cpu") else rows, dtype=np.int64), device=dev)
        if rows_t.numel() != B:
            raise HipError("SlotContrast.loss: %d dataset rows for %d batch rows" % (rows_t.numel(), B))
        ids = None
        if self.distinct:
            key = (data.data_ptr(), tuple(data.shape), S)
            if self._ids is None or self._ids[0] != key:
                self._ids = (key, item_ids(data, S))
            ids = self._ids[1].to(dev)
        n_glob = float(B if global_rows is None else global_rows)
        x3 = input.to(device=dev, dtype=dt).reshape(B, S, E)
        y3 = output.reshape(B, S, E)
        nx = x3.norm(dim=-1, keepdim=True)
        ny = y3.norm(dim=-1, keepdim=True)
        y3 = torch.where(ny > COS_EPS, y3, y3.detach())            # [|y| > eps]: no gradient through a zero output slot
        xh = x3 / nx.clamp_min(COS_EPS)
        yh = y3 / y3.norm(dim=-1, keepdim=True).clamp_min(COS_EPS)
        W = None if weight is None else weight.to(device=dev, dtype=dt).reshape(B, S, E).mean(dim=-1)
        total = output.new_zeros(())
        for s in range(S):
            ck = torch.as_tensor(self.candidate_rows(step, s, N), device=dev)
            c = data[ck.to(data.device), s * E:(s + 1) * E].to(device=dev, dtype=dt)
            ch = c / c.norm(dim=-1, keepdim=True).clamp_min(COS_EPS)
            z = (yh[:, s] @ ch.t()) / self.temperature                                         # [B, K]
            hit = (ids[s][ck][None, :] == ids[s][rows_t][:, None]) if ids is not None else (ck[None, :] == rows_t[:, None])
            z = z.masked_fill(hit, float("-inf"))
            z0 = (xh[:, s] * yh[:, s]).sum(dim=-1, keepdim=True) / self.temperature
            l = torch.logsumexp(torch.cat([z0, z], dim=1), dim=1) - z0[:, 0]
            l = torch.where(nx[:, s, 0] > COS_EPS, l, torch.zeros_like(l))                   # no positive: nothing
            total = total + (l if W is None else W[:, s] * l).sum()
        return self.weight * total / (n_glob * S)


def contrast_from_config(block):
    """The `HIP: CONTRAST:` block of the embedding script's config: {NEGATIVES: 256, TEMPERATURE: 0.1, WEIGHT: 1.0, SEED: 0,
    DISTINCT: true}, every key optional.  None / empty -> None."""
    if not block:
        return None
    if not isinstance(block, dict):
        raise HipError("CONTRAST must be a mapping, got %r" % (block,))
    known = {"NEGATIVES", "TEMPERATURE", "WEIGHT", "SEED", "DISTINCT"}
    extra = sorted(set(block) - known, key=str)
    if extra:
        raise HipError("CONTRAST: unknown key(s) %s (known: %s)" % (", ".join(map(str, extra)), ", ".join(sorted(known))))
    return SlotContrast(negatives=block.get("NEGATIVES", 256), temperature=block.get("TEMPERATURE", 0.1), weight=block.get("WEIGHT", 1.0),
                        seed=block.get("SEED", 0), distinct=block.get("DISTINCT", True))
