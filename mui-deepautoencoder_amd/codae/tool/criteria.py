"""Criteria and metrics of `codae.tool` (codae/tool/metering.py:24-204 of the reference).

CombinedCriterion (the abalone loss) and RankingLoss (the validation-only rank metric) keep the
reference's call signatures and numerics.  ComplementRetriever answers the question the rank metric scores: the k
inventory items closest to a reconstructed slot (codae_complete_topk); RetrievalMetrics scores that answer over a validation
set: hit@k, MRR and a position histogram per slot, incomplete rows included (codae_retrieval_metrics_batched).  With tensors on a HIP device they run as kernels of
libcodae_hip.so (criteria.hip: codae_combined_loss_fwd_bwd / _full, codae_ranking_loss); with host
tensors (which upstream also accepts) they are whole-tensor torch expressions, no per-sample loops.
"""
import ctypes as C

import numpy as np
import torch

from ..hip import HipError, check as _check, current_stream as _stream, lib as _hip_lib, ptr as _ptr
from ..hip import RM_HIST, RM_HIT, RM_MAX_KS, RM_PAIRS, RM_RR, RM_RRE, RM_STRIDE
from .batching import get_mask_transformation


class _CombinedMeanFn(torch.autograd.Function):
    """loss = CombinedCriterion mean loss; d loss / d y from the same kernel pass."""

    @staticmethod
    def forward(ctx, y, x, crit):
        loss, dy = crit._hip_mean(x, y.detach())
        ctx.save_for_backward(dy)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dy,) = ctx.saved_tensors
        return g * dy, None, None


def get_rmse(x, y):
    return np.sqrt(np.mean((x - y) ** 2))


class RankingLoss:
    """Cosine-rank of the reconstructed slot among the validation inventory (metering.py:29-79)."""

    def __init__(self, dataset, validation_indices, device):
        self.dataset = dataset
        self.device = device
        self.category_getter = torch.zeros((self.dataset.nb_predictor), device=self.device)
        for i in range(self.dataset.nb_used_category):
            self.category_getter[i * self.dataset.embedding_size] = i
        self.validation_indices = validation_indices
        self._val = None

    def _get_inventory(self, dev):
        ds = self.dataset
        S, E = ds.nb_used_category, ds.embedding_size
        if getattr(self, "_inv", None) is None or self._inv.device != dev:
            self._inv = torch.stack([ds.data_per_category[c].to(dev, torch.float32) for c in range(S)]).contiguous()
            self._inv_norm = torch.empty(self._inv.shape[:2], dtype=torch.float32, device=dev)
            with torch.cuda.device(dev):
                _check(_hip_lib().codae_row_norms(_ptr(self._inv), S * self._inv.shape[1], E, _ptr(self._inv_norm), _stream()))
            self._val_i32 = torch.as_tensor(list(self.validation_indices), dtype=torch.int32, device=dev)
            self._out = torch.zeros(1, dtype=torch.float64, device=dev)

    def _get_hip(self, prediction, fmask, indices):
        ds = self.dataset
        dev = prediction.device
        S, E = ds.nb_used_category, ds.embedding_size
        self._get_inventory(dev)
        idx = torch.as_tensor(list(indices), dtype=torch.int32, device=dev)
        pred = prediction.detach().to(torch.float32).contiguous()
        fm = fmask.to(device=dev, dtype=torch.float32).contiguous()
        self._out.zero_()
        with torch.cuda.device(dev):
            _check(_hip_lib().codae_ranking_loss(_ptr(pred), _ptr(fm), _ptr(idx), pred.shape[0], pred.shape[1], S, E,
                                                 _ptr(self._inv), _ptr(self._inv_norm), self._inv.shape[1],
                                                 _ptr(self._val_i32), len(self.validation_indices), _ptr(self._out),
                                                 _stream()))
        return float(self._out.item())

    # ---- device-resident form: one batched call per validation batch, one read-back per epoch ---------
    def _device_tables(self, dev):
        self._get_inventory(dev)
        if getattr(self, "_inv_val", None) is None or self._inv_val.device != dev:
            S, E = self.dataset.nb_used_category, self.dataset.embedding_size
            V = len(self.validation_indices)
            self._inv_val = torch.empty((S, V, E), dtype=torch.float32, device=dev)
            self._inv_val_norm = torch.empty((S, V), dtype=torch.float32, device=dev)
            with torch.cuda.device(dev):
                _check(_hip_lib().codae_gather_inventory_rows(_ptr(self._inv), self._inv.shape[1], E, S, _ptr(self._val_i32), V,
                                                              _ptr(self._inv_val), _stream()))
                _check(_hip_lib().codae_row_norms(_ptr(self._inv_val), S * V, E, _ptr(self._inv_val_norm), _stream()))
            pos = torch.full((self._inv.shape[1],), -1, dtype=torch.int32)
            pos[torch.as_tensor(list(self.validation_indices), dtype=torch.long)] = torch.arange(V, dtype=torch.int32)
            self._val_pos = pos.to(dev)
            # rows of a slot's validation inventory that hold the same bytes share a group id: the reference never counts an exact
            # copy of the sample's own row (equal similarities out of one cosine_similarity call), so neither may we (codae_hip.h)
            groups = [torch.unique(self._inv_val[c], dim=0, return_inverse=True)[1] for c in range(S)]
            grp = torch.stack(groups).to(torch.int32).contiguous()
            # (kept as soon as ANY slot holds duplicates: a slot without any has V groups, and its maximum says nothing about the others)
            self._val_group = grp if any(int(g.max()) + 1 < V for g in groups) else None     # (no duplicates: nothing to skip)
            self._acc = torch.zeros(1, dtype=torch.float64, device=dev)
            self._work = None

    def add(self, prediction, row_idx, corrupter, run=0, chunk=4096):
        """Accumulate RankingLoss.get(prediction, fmask, indices) of one validation batch ON THE DEVICE: `row_idx` int32
        dataset rows (device), masks taken from `corrupter`'s device tables for `run`.  No host synchronisation; read the
        epoch's sum with total()."""
        dev = prediction.device
        self._device_tables(dev)
        S, E = self.dataset.nb_used_category, self.dataset.embedding_size
        V = len(self.validation_indices)
        pred = prediction.detach()
        if pred.dtype != torch.float32 or not pred.is_contiguous():
            pred = pred.to(torch.float32).contiguous()
        B = pred.shape[0]
        chunk = min(int(chunk), V)
        if self._work is None or self._work.numel() < B * chunk or self._rows.numel() < 8 * B:
            self._work = torch.empty(B * chunk, dtype=torch.float32, device=dev)
            self._rows = torch.empty(8 * B, dtype=torch.int32, device=dev)
            self._perm = torch.empty(S * B + S, dtype=torch.int32, device=dev)
            self._q = torch.empty(B * E, dtype=torch.float32, device=dev)
        m2u = corrupter.mask_to_use_i32
        with torch.cuda.device(dev):
            _check(_hip_lib().codae_ranking_loss_batched(
                _ptr(pred), B, pred.shape[1], S, E, _ptr(row_idx), None, _ptr(m2u), m2u.shape[1], int(run),
                _ptr(corrupter.mask_table_u8), _ptr(self._inv), _ptr(self._inv_norm), self._inv.shape[1],
                _ptr(self._inv_val), _ptr(self._inv_val_norm), _ptr(self._val_pos),
                _ptr(self._val_group) if self._val_group is not None else None, V, _ptr(self._work), chunk, _ptr(self._rows),
                _ptr(self._perm), _ptr(self._q), _ptr(self._acc), _stream()))
        self._keep = (pred, row_idx)             # (alive until the stream has consumed them)

    def total(self, reset=True):
        """Sum of the batches add()ed since the last reset (one device-to-host read)."""
        v = float(self._acc.item())
        if reset:
            self._acc.zero_()
        return v

    def get(self, prediction, fmask, indices):
        if prediction.device.type == "cuda":
            return self._get_hip(prediction, fmask, indices)
        E = self.dataset.embedding_size
        dev = prediction.device
        if self._val is None or self._val.device != dev:
            self._val = torch.as_tensor(list(self.validation_indices), dtype=torch.long, device=dev)
        idx = torch.as_tensor(list(indices), dtype=torch.long, device=dev)
        # blanked slot of every sample: dot(1 - fmask, category_getter) (metering.py:56), k = 1 only
        slot = torch.matmul(1 - fmask, self.category_getter.to(dev)).long()
        pred = prediction.detach()
        total = 0.0
        for c in torch.unique(slot).tolist():
            rows = (slot == c).nonzero(as_tuple=True)[0]
            inv = self.dataset.data_per_category[c].to(dev)                      # [N, E] unscaled
            q = pred[rows, c * E:(c + 1) * E]                                    # [b, E]
            inv_n = inv / inv.norm(dim=1, keepdim=True).clamp_min(1e-8)
            q_n = q / q.norm(dim=1, keepdim=True).clamp_min(1e-8)
            s = q_n @ inv_n.t()                                                  # [b, N] cosine
            own = s.gather(1, idx[rows].unsqueeze(1))                            # s[idx]
            rank = (own > s[:, self._val]).sum(dim=1)                            # strict > over validation ids
            total += float((1 - rank.double() / (len(self.validation_indices) - 1)).sum())
        return total


TOPK_MAX = 256


class ComplementRetriever:
    """Complementarity inference (README step IV of the reference): the k inventory items closest to the model's
    reconstruction of a blanked slot.

    For query b with slot c the score of candidate v is <q, v> / (max(|q|, 1e-8) max(|v|, 1e-8)), q = prediction[b][cE:(c+1)E];
    candidates are the rows of data_per_category[c] (all dataset rows, or the `candidates` subset).  Results are ordered by
    score descending, equal scores by ascending dataset row id (-0 == +0); NaN scores are never returned; missing results
    are (-1, -inf).  With `distinct`, rows of a slot's inventory that hold the same bytes are one item, represented by its
    lowest dataset row.  Device tensors run codae_complete_topk (fp32 GEMM per candidate chunk + the HIP top-k selection
    kernel, no host synchronisation); host tensors a whole-tensor torch form of the same contract."""

    def __init__(self, dataset, device, candidates=None, distinct=True, row_norms=None):
        """row_norms: one-slot inventories only - an fp32 [n_obs] device tensor of the rows' norms that is already at hand (the
        export kernel's, for a bank of codes): the device tables take the candidates' norms from it instead of sweeping them."""
        self.dataset = dataset
        self.device = device
        self.distinct = bool(distinct)
        self.row_norms = row_norms
        self.S, self.E = int(dataset.nb_used_category), int(dataset.embedding_size)
        self.n_obs = int(dataset.data_per_category[0].shape[0])
        if candidates is None:
            self.candidates = None
        else:
            rows = torch.as_tensor(list(candidates) if not torch.is_tensor(candidates) else candidates, dtype=torch.long).reshape(-1)
            if rows.numel() == 0 or int(rows.min()) < 0 or int(rows.max()) >= self.n_obs:
                raise ValueError("candidates must be a non-empty list of dataset rows in [0, %d)" % self.n_obs)
            self.candidates = torch.unique(rows)                  # sorted: candidate positions follow dataset row order
        self._tables = {}

    # ---- tables: built once per device ------------------------------------------------------------------------------
    def _host_tables(self):
        """(cand [S, n_cand, E] f32, count [S], row_id [S, n_cand] i32 (pad -1), pos [S, n_obs] i32: row -> candidate
        position or -1), built on the host."""
        t = self._tables.get("host")
        if t is not None:
            return t
        S, E, n_obs = self.S, self.E, self.n_obs
        rows = self.candidates if self.candidates is not None else torch.arange(n_obs)
        per = []
        for c in range(S):
            X = self.dataset.data_per_category[c].detach().to("cpu", torch.float32)[rows].contiguous()
            if self.distinct:
                # identical bytes = one item (compared as int32 words, so -0 and +0 or two NaN payloads stay apart);
                # the item is its lowest dataset row, items in ascending order of that row
                _, inv = torch.unique(X.view(torch.int32), dim=0, return_inverse=True)
                local = torch.arange(rows.numel())
                first = torch.full((int(inv.max()) + 1,), rows.numel(), dtype=torch.long).scatter_reduce(0, inv, local, "amin")
                first = first.sort()[0]                               # (rows ascend: lowest local index = lowest row id)
                item = torch.empty_like(first)
                item[inv[first]] = torch.arange(first.numel())        # group id -> item position
                ids, item_of_row, Xc = rows[first], item[inv], X[first]
            else:
                ids, item_of_row, Xc = rows, torch.arange(rows.numel()), X
            pos = torch.full((n_obs,), -1, dtype=torch.int32)
            pos[rows] = item_of_row.to(torch.int32)
            per.append((Xc, ids, pos))
        n_cand = max(p[0].shape[0] for p in per)
        cand = torch.zeros((S, n_cand, E), dtype=torch.float32)
        row_id = torch.full((S, n_cand), -1, dtype=torch.int32)
        for c, (Xc, ids, _) in enumerate(per):
            cand[c, :Xc.shape[0]] = Xc
            row_id[c, :ids.numel()] = ids.to(torch.int32)
        t = (cand, [p[0].shape[0] for p in per], row_id, torch.stack([p[2] for p in per]).contiguous())
        self._tables["host"] = t
        return t

    def _device_tables(self, dev):
        t = self._tables.get(dev)
        if t is None:
            cand, count, row_id, pos = self._host_tables()
            S, n_cand = cand.shape[0], cand.shape[1]
            cand_d = cand.to(dev).contiguous()
            row_id = row_id.to(dev).contiguous()
            if self.row_norms is not None and S == 1:
                norm = self.row_norms.to(dev)[row_id.clamp_min(0).long()].contiguous()      # candidate j is dataset row row_id[j]
            else:
                norm = torch.empty((S, n_cand), dtype=torch.float32, device=dev)
                with torch.cuda.device(dev):
                    _check(_hip_lib().codae_row_norms(_ptr(cand_d), S * n_cand, self.E, _ptr(norm), _stream()))
            t = (cand_d, norm, (C.c_int32 * S)(*count), row_id, pos.to(dev).contiguous())
            self._tables[dev] = t
        return t

    # ---- arguments ----------------------------------------------------------------------------------------------------
    def _check_args(self, prediction, slot, k, exclude, chunk):
        if not torch.is_tensor(prediction) or prediction.dim() != 2 or prediction.shape[1] != self.S * self.E or prediction.shape[0] < 1:
            raise HipError("topk: prediction must be a [B, %d] tensor" % (self.S * self.E))
        B = prediction.shape[0]
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= TOPK_MAX:
            raise HipError("topk: k must be an int in [1, %d], got %r" % (TOPK_MAX, k))
        if isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or int(chunk) < 1:
            raise HipError("topk: chunk must be a positive int, got %r" % (chunk,))
        if torch.is_tensor(slot):
            if slot.dim() != 1 or slot.shape[0] != B or slot.dtype.is_floating_point or slot.dtype == torch.bool:
                raise HipError("topk: slot tensor must be an integer [B] tensor")
            if slot.device.type == "cpu" and slot.numel() and (int(slot.min()) < 0 or int(slot.max()) >= self.S):
                raise HipError("topk: slot outside [0, %d)" % self.S)
        elif isinstance(slot, bool) or not isinstance(slot, (int, np.integer)) or not 0 <= int(slot) < self.S:
            raise HipError("topk: slot must be an int in [0, %d) or a [B] tensor, got %r" % (self.S, slot))
        if exclude is not None:
            if not torch.is_tensor(exclude) or exclude.dim() != 1 or exclude.shape[0] != B or exclude.dtype.is_floating_point:
                raise HipError("topk: exclude must be an integer [B] tensor of dataset rows")

    def topk(self, prediction, slot, k, exclude=None, chunk=8192):
        """(idx LongTensor [B, k] dataset rows, score FloatTensor [B, k]) of the k best candidates for every query row.
        slot: int or integer [B] tensor (on the device it is not read back: a row whose slot lies outside [0, S) returns
        only (-1, -inf)); exclude: optional integer [B] dataset rows, each skipped (with the item it belongs to) for its
        query; chunk: candidates per GEMM + selection pass on the device."""
        self._check_args(prediction, slot, k, exclude, chunk)
        if prediction.device.type == "cuda":
            return self._device_topk(prediction, int(k), exclude, int(chunk), slot=slot)
        return self._host_topk(prediction, slot, int(k), exclude)

    def _device_topk(self, prediction, k, exclude, chunk, slot=None, mask_id=None, mask_table=None):
        dev = prediction.device
        cand, norm, count, row_id, pos = self._device_tables(dev)
        S, E, n_cand = self.S, self.E, cand.shape[1]
        pred = prediction.detach()
        if pred.dtype != torch.float32 or not pred.is_contiguous():
            pred = pred.to(torch.float32).contiguous()
        B = pred.shape[0]
        i32 = dict(dtype=torch.int32, device=dev)
        slot_t = None
        if slot is not None:
            slot_t = (torch.full((B,), int(slot), **i32) if not torch.is_tensor(slot) else slot.to(**i32).contiguous())
        ex = None if exclude is None else exclude.to(**i32).contiguous()
        chunk = min(chunk, n_cand)
        work = torch.empty(B * chunk, dtype=torch.float32, device=dev)
        rows = torch.empty(3 * B, **i32)
        perm = torch.empty(S * B + S, **i32)
        q = torch.empty(B * E, dtype=torch.float32, device=dev)
        state = torch.empty(B * k, dtype=torch.int64, device=dev)
        out_idx = torch.empty((B, k), **i32)
        out_score = torch.empty((B, k), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _check(_hip_lib().codae_complete_topk(
                _ptr(pred), B, S * E, S, E, _ptr(slot_t), None, _ptr(mask_id), None, 0, 0, _ptr(mask_table),
                _ptr(cand), _ptr(norm), _ptr(row_id), n_cand, count, _ptr(ex), _ptr(pos) if ex is not None else None, self.n_obs,
                k, _ptr(work), chunk, _ptr(rows), _ptr(perm), _ptr(q), _ptr(state), _ptr(out_idx), _ptr(out_score), _stream()))
        self._keep = (pred, slot_t, ex, mask_id, work, rows, perm, q, state)     # (alive until the stream has consumed them)
        return out_idx.long(), out_score

    def _host_topk(self, prediction, slot, k, exclude):
        cand, count, row_id, pos = self._host_tables()
        E = self.E
        pred = prediction.detach().to("cpu")
        B = pred.shape[0]
        slots = torch.full((B,), int(slot), dtype=torch.long) if not torch.is_tensor(slot) else slot.to("cpu", torch.long)
        ex = None if exclude is None else exclude.to("cpu", torch.long)
        out_idx = torch.full((B, k), -1, dtype=torch.long)
        out_score = torch.full((B, k), float("-inf"), dtype=torch.float32)
        for c in torch.unique(slots).tolist():
            n = count[c]
            rows = (slots == c).nonzero(as_tuple=True)[0]
            if n == 0:
                continue
            V = cand[c, :n].double()
            q = pred[rows, c * E:(c + 1) * E].double()
            s = (q @ V.t()) / (q.norm(dim=1, keepdim=True).clamp_min(1e-8) * V.norm(dim=1).clamp_min(1e-8)[None, :])
            s = s.float() + 0.0                                           # fp32 scores; -0 -> +0
            bad = torch.isnan(s)
            if ex is not None:
                e = ex[rows]
                ok = (e >= 0) & (e < self.n_obs)
                p = torch.full_like(e, -1)
                p[ok] = pos[c, e[ok]].long()
                hit = (p >= 0).nonzero(as_tuple=True)[0]
                bad[hit, p[hit]] = True
            s = s.masked_fill(bad, float("-inf"))
            # score descending with ties in candidate (= dataset row) order, then the invalid ones to the back
            order = torch.sort(s, dim=1, descending=True, stable=True)[1]
            order = order.gather(1, torch.sort(bad.gather(1, order).to(torch.int8), dim=1, stable=True)[1])
            kk = min(k, n)
            sel = order[:, :kk]
            valid = ~bad.gather(1, sel)
            out_idx[rows, :kk] = torch.where(valid, row_id[c].long()[sel], torch.full_like(sel, -1))
            out_score[rows, :kk] = torch.where(valid, s.gather(1, sel), torch.full_like(s[:, :kk], float("-inf")))
        return out_idx, out_score


class _OneSlot:
    """Slot c of a dataset as a one-slot dataset: what ComplementRetriever builds one slot's candidate table from."""

    def __init__(self, dataset, c):
        self.nb_used_category, self.embedding_size = 1, int(dataset.embedding_size)
        self.data_per_category = {0: dataset.data_per_category[c]}


def _check_ks(ks):
    try:
        ks = tuple(ks)
    except TypeError:
        raise HipError("retrieval metrics: ks must be a sequence of ints, got %r" % (ks,))
    if len(ks) > RM_MAX_KS:
        raise HipError("retrieval metrics: at most %d thresholds, got %d" % (RM_MAX_KS, len(ks)))
    for i, k in enumerate(ks):
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or int(k) < 1 or int(k) >= 2 ** 31 or (i and int(k) <= int(ks[i - 1])):
            raise HipError("retrieval metrics: thresholds must be ascending positive ints, got %r" % (ks,))
    return tuple(int(k) for k in ks)


class RetrievalMetrics:
    """hit@k, MRR, rank error and a position histogram of the reconstructed slots of a validation batch, per slot
    (include/codae_hip.h, "Retrieval metrics": the one definition the kernels, get() and the tests' reference share).

    Candidates of slot c are the validation rows that have the slot (`presence`: a SlotPresence or a uint8 [n_obs, S] table; None =
    all of them); with `distinct` candidates holding the same bytes are one item, as ComplementRetriever folds them.  Every slot a
    row's mask blanks and the row has is a query pair; its competitors are the slot's items without the row's own; position
    p = 1 + competitors - #{own > s_j}, so ties and NaN count against the model.  add() runs on device tensors without a host
    synchronisation (codae_retrieval_metrics_batched) and accumulates; total() reads the sums; get() is the whole-tensor torch form
    for host tensors."""

    def __init__(self, dataset, validation_indices, device, ks=(1, 5, 10, 50), presence=None, distinct=True):
        self.dataset = dataset
        self.device = device
        self.ks = _check_ks(ks)
        self.distinct = bool(distinct)
        self.S, self.E = int(dataset.nb_used_category), int(dataset.embedding_size)
        self.n_obs = int(dataset.data_per_category[0].shape[0])
        table = getattr(presence, "table", presence)
        if table is not None:
            table = np.asarray(table.detach().cpu().numpy() if hasattr(table, "detach") else table)
            if table.shape != (self.n_obs, self.S):
                raise HipError("retrieval metrics: the presence table must be [%d, %d], got shape %r" % (self.n_obs, self.S, tuple(table.shape)))
            table = np.ascontiguousarray(table != 0).astype(np.uint8)
        self.presence = table
        rows = torch.as_tensor(list(validation_indices) if not torch.is_tensor(validation_indices) else validation_indices, dtype=torch.long).reshape(-1)
        if rows.numel() == 0 or int(rows.min()) < 0 or int(rows.max()) >= self.n_obs:
            raise HipError("retrieval metrics: validation_indices must be a non-empty list of dataset rows in [0, %d)" % self.n_obs)
        self.validation_indices = torch.unique(rows)
        self.mask_table = None                 # bound by HipEmbeddingTrainer.retrieval_metrics: add() then needs no corrupter
        self.mask_to_use = None
        self._tables = {}

    # ---- tables ---------------------------------------------------------------------------------------------------------
    def _host_tables(self):
        """(cand [S, n_cand, E] f32 (n_cand a multiple of 4), count [S], pos [S, n_obs] i32): per slot the table
        ComplementRetriever._host_tables builds over the validation rows that have the slot."""
        t = self._tables.get("host")
        if t is not None:
            return t
        S, E = self.S, self.E
        per = []
        for c in range(S):
            rows = self.validation_indices
            if self.presence is not None:
                rows = rows[torch.from_numpy(self.presence[rows.numpy(), c] != 0)]
            if rows.numel() == 0:
                per.append((torch.zeros((0, E), dtype=torch.float32), 0, torch.full((self.n_obs,), -1, dtype=torch.int32)))
                continue
            cand, count, _, pos = ComplementRetriever(_OneSlot(self.dataset, c), "cpu", candidates=rows, distinct=self.distinct)._host_tables()
            per.append((cand[0, :count[0]], count[0], pos[0]))
        n_cand = max(4, -(-max(p[1] for p in per) // 4) * 4)
        cand = torch.zeros((S, n_cand, E), dtype=torch.float32)
        for c, (Xc, n, _) in enumerate(per):
            cand[c, :n] = Xc
        t = (cand, [p[1] for p in per], torch.stack([p[2] for p in per]).contiguous())
        self._tables["host"] = t
        return t

    def _device_tables(self, dev):
        t = self._tables.get(dev)
        if t is None:
            cand, count, pos = self._host_tables()
            S, E, n_cand = self.S, self.E, cand.shape[1]
            cand_d = cand.to(dev).contiguous()
            inv = torch.stack([self.dataset.data_per_category[c].to(dev, torch.float32) for c in range(S)]).contiguous()
            norm = torch.empty((S, n_cand), dtype=torch.float32, device=dev)
            inv_norm = torch.empty((S, self.n_obs), dtype=torch.float32, device=dev)
            with torch.cuda.device(dev):
                _check(_hip_lib().codae_row_norms(_ptr(cand_d), S * n_cand, E, _ptr(norm), _stream()))
                _check(_hip_lib().codae_row_norms(_ptr(inv), S * self.n_obs, E, _ptr(inv_norm), _stream()))
            t = dict(cand=cand_d, norm=norm, count=(C.c_int32 * S)(*count), pos=pos.to(dev).contiguous(), inv=inv, inv_norm=inv_norm,
                     presence=None if self.presence is None else torch.from_numpy(self.presence).to(dev).contiguous(),
                     ks=(C.c_int32 * max(1, len(self.ks)))(*self.ks), acc=torch.zeros((S, RM_STRIDE), dtype=torch.float64, device=dev),
                     work=None)
            self._tables[dev] = t
            self._dev = dev
        return t

    # ---- device ---------------------------------------------------------------------------------------------------------
    def add(self, prediction, row_idx, corrupter=None, run=0, chunk=4096, mask_to_use=None):
        """Accumulate one validation batch ON THE DEVICE: `prediction` [B, S*E], `row_idx` int32 dataset rows (device), masks from
        `corrupter`'s device tables for `run` (`mask_to_use`: an int32 [n_obs, nb_run] device table instead of
        corrupter.mask_to_use_i32, e.g. what SlotPresence.assign_masks returns).  chunk: items per GEMM + count pass.  No host
        synchronisation; read the sums with total()."""
        dev = prediction.device
        t = self._device_tables(dev)
        S, E, n_cand = self.S, self.E, t["cand"].shape[1]
        table = corrupter.mask_table_u8 if corrupter is not None else self.mask_table
        m2u = mask_to_use if mask_to_use is not None else (corrupter.mask_to_use_i32 if corrupter is not None else self.mask_to_use)
        if table is None or m2u is None:
            raise HipError("retrieval metrics: add() needs a corrupter (or a metric bound to a trainer's mask tables)")
        if prediction.dim() != 2 or prediction.shape[1] != S * E or prediction.shape[0] < 1 or row_idx.numel() != prediction.shape[0]:
            raise HipError("retrieval metrics: prediction must be [B, %d] with one dataset row per batch row" % (S * E))
        if isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or int(chunk) < 1:
            raise HipError("retrieval metrics: chunk must be a positive int, got %r" % (chunk,))
        pred = prediction.detach()
        if pred.dtype != torch.float32 or not pred.is_contiguous():
            pred = pred.to(torch.float32).contiguous()
        B = pred.shape[0]
        chunk = min(-(-int(chunk) // 4) * 4, n_cand)             # (whole groups of four columns: the count pass loads 16 bytes)
        if t["work"] is None or t["work"].numel() < B * chunk or t["perm"].numel() < S * B + S:
            t["work"] = torch.empty(B * chunk, dtype=torch.float32, device=dev)
            t["state"] = torch.empty(4 * S * B, dtype=torch.int32, device=dev)
            t["perm"] = torch.empty(S * B + S, dtype=torch.int32, device=dev)
            t["q"] = torch.empty(B * E, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _check(_hip_lib().codae_retrieval_metrics_batched(
                _ptr(pred), B, S * E, S, E, _ptr(row_idx), None, _ptr(m2u), m2u.shape[1], int(run), _ptr(table), _ptr(t["presence"]),
                _ptr(t["inv"]), _ptr(t["inv_norm"]), self.n_obs, _ptr(t["cand"]), _ptr(t["norm"]), n_cand, t["count"], _ptr(t["pos"]),
                t["ks"], len(self.ks), _ptr(t["work"]), chunk, _ptr(t["state"]), _ptr(t["perm"]), _ptr(t["q"]), _ptr(t["acc"]), _stream()))
        self._keep = (pred, row_idx, m2u, table)             # (alive until the stream has consumed them)

    def total(self, reset=True):
        """The metrics of the batches add()ed since the last reset (one device-to-host read): see summary()."""
        dev = getattr(self, "_dev", None)
        if dev is None:
            return self.summary(np.zeros((self.S, RM_STRIDE)))
        acc = self._tables[dev]["acc"]
        sums = acc.cpu().numpy().copy()
        if reset:
            acc.zero_()
        return self.summary(sums)

    def last_positions(self):
        """int64 [S, B] on the host: the position p of every query pair of the LAST add() (0 where (b, c) is no pair), read from
        the kernels' pair state.  Synchronises: for analysis ("which rows missed") and tests, not for the sweep."""
        dev = getattr(self, "_dev", None)
        if dev is None or getattr(self, "_keep", None) is None:
            raise HipError("retrieval metrics: last_positions() needs an add() first")
        t, S, B = self._tables[dev], self.S, self._keep[0].shape[0]
        st = t["state"][:4 * S * B].cpu().view(S, B, 4).long()
        self_col, beaten = st[..., 2], st[..., 3]
        n = torch.tensor(list(t["count"]), dtype=torch.long)[:, None] - (self_col >= 0).long()
        p = 1 + n - beaten
        p[(self_col == -2) | (n < 1)] = 0
        return p

    # ---- the sums as metrics --------------------------------------------------------------------------------------------
    def _one(self, s):
        pairs = float(s[RM_PAIRS])
        mean = (lambda v: float(v) / pairs) if pairs > 0 else (lambda v: float("nan"))
        out = {"pairs": int(round(pairs)), "rre": mean(s[RM_RRE]), "mrr": mean(s[RM_RR])}
        for i, k in enumerate(self.ks):
            out["hit@%d" % k] = mean(s[RM_HIT + i])
        # the bucket [2^i, 2^(i+1)) of positions that holds the median pair (None without pairs)
        cum = np.cumsum(s[RM_HIST:RM_HIST + 32])
        out["median_position_bucket"] = int(np.searchsorted(cum, pairs / 2.0)) if pairs > 0 else None
        return out

    def summary(self, sums):
        """{pairs, rre, mrr, hit@<k>.. (means over the pairs), median_position_bucket, per_slot: [the same per slot], sums: the raw
        float64 [S, RM_STRIDE] block} of a block of sums."""
        sums = np.asarray(sums, dtype=np.float64).reshape(self.S, RM_STRIDE)
        out = self._one(sums.sum(axis=0))
        out["per_slot"] = [self._one(sums[c]) for c in range(self.S)]
        out["sums"] = sums
        return out

    # ---- host -----------------------------------------------------------------------------------------------------------
    def get(self, prediction, fmask_or_mask_ids, indices, mask_table=None):
        """The same definition for HOST tensors, in whole-tensor torch ops (float64 cosines rounded to fp32, then compared):
        `fmask_or_mask_ids` is the float mask [B, S*E] of the batch (0 = blanked) or integer mask ids [B] into `mask_table`
        ([n_masks, S*E], 0 = blanked; default: the table the metric is bound to); `indices` the dataset rows.  Returns summary()
        of this batch alone; nothing is accumulated."""
        S, E = self.S, self.E
        cand, count, pos = self._host_tables()
        pred = prediction.detach().to("cpu")
        idx = torch.as_tensor(list(indices) if not torch.is_tensor(indices) else indices).to("cpu", torch.long).reshape(-1)
        m = fmask_or_mask_ids if torch.is_tensor(fmask_or_mask_ids) else torch.as_tensor(np.asarray(fmask_or_mask_ids))
        m = m.detach().to("cpu")
        if m.dim() == 1:
            table = mask_table if mask_table is not None else self.mask_table
            if table is None:
                raise HipError("retrieval metrics: mask ids need a mask table")
            m = torch.as_tensor(table).detach().to("cpu")[m.long()]
        if pred.dim() != 2 or pred.shape[1] != S * E or m.shape != pred.shape or idx.numel() != pred.shape[0]:
            raise HipError("retrieval metrics: prediction and mask must be [B, %d] with one dataset row per batch row" % (S * E))
        blank = m[:, ::E] == 0                                            # [B, S]
        if self.presence is not None:
            blank = blank & torch.from_numpy(self.presence[idx.numpy()] != 0)
        sums = np.zeros((S, RM_STRIDE), dtype=np.float64)
        for c in range(S):
            nc = count[c]
            rows = blank[:, c].nonzero(as_tuple=True)[0]
            if nc == 0 or rows.numel() == 0:
                continue
            V = cand[c, :nc].double()
            q = pred[rows, c * E:(c + 1) * E].double()
            own_v = self.dataset.data_per_category[c].detach().to("cpu")[idx[rows]].double()
            qn = q.norm(dim=1).clamp_min(1e-8)
            s = ((q @ V.t()) / (qn[:, None] * V.norm(dim=1).clamp_min(1e-8)[None, :])).float()
            own = ((q * own_v).sum(dim=1) / (qn * own_v.norm(dim=1).clamp_min(1e-8))).float()
            beats = own[:, None] > s                                      # (a NaN on either side: False)
            self_col = pos[c, idx[rows]].long()
            mine = (self_col >= 0).nonzero(as_tuple=True)[0]
            beats[mine, self_col[mine]] = False                           # the own item is skipped by position
            n = nc - (self_col >= 0).long()
            keep = n >= 1
            n, p = n[keep].double(), (1 + n - beats.sum(dim=1))[keep]
            sums[c, RM_PAIRS] = p.numel()
            sums[c, RM_RRE] = float(((p.double() - 1) / n).sum())
            sums[c, RM_RR] = float((1.0 / p.double()).sum())
            for i, k in enumerate(self.ks):
                sums[c, RM_HIT + i] = int((p <= k).sum())
            if p.numel():
                sums[c, RM_HIST:RM_HIST + 32] = np.bincount(np.floor(np.log2(p.numpy().astype(np.float64))).astype(np.int64), minlength=32)[:32]
        return self.summary(sums)


def retrieval_metrics_from_config(block):
    """The `HIP: RETRIEVAL_METRICS:` block of the embedding script's config: {K: [1, 10, 50], DISTINCT: true}.  None -> None (the
    script then runs, logs and writes exactly what it does without the key); else the keyword arguments of RetrievalMetrics /
    HipEmbeddingTrainer.retrieval_metrics: {"ks": (..), "distinct": bool}."""
    if block is None:
        return None
    if not isinstance(block, dict):
        raise HipError("RETRIEVAL_METRICS must be a mapping, got %r" % (block,))
    known = {"K", "DISTINCT"}
    extra = sorted(set(map(str, block)) - known)
    if extra:
        raise HipError("RETRIEVAL_METRICS: unknown key(s) %s (known: %s)" % (", ".join(extra), ", ".join(sorted(known))))
    distinct = block.get("DISTINCT", True)
    if not isinstance(distinct, bool):
        raise HipError("RETRIEVAL_METRICS: DISTINCT must be true or false, got %r" % (distinct,))
    return {"ks": _check_ks(block.get("K", (1, 10, 50))), "distinct": distinct}


class CombinedCriterion:
    """Per-variable RMSE / NLL loss following dataset.arch (metering.py:82-204)."""

    def __init__(self, arch, k_max, device, observation_mask, weight=None, reduction="none"):
        if k_max < 0 | k_max >= len(arch):      # chained comparison kept as upstream (never fires)
            raise Exception("Error: maximum number of corrupted index [k_max] must be (> 0) && (< len(arch)).")
        self.arch = arch
        self.k_max = k_max
        self.device = device
        self.reduction = reduction
        self.weight = torch.ones((1, len(self.arch))) if weight is None else torch.Tensor(weight)
        self.observation_mask = observation_mask
        self.io_size = len(self.observation_mask)
        # upstream tests type == "continuous", which no dataset emits: only the length is used
        self.loss_mask = [1 if v["type"] == "continuous" else 0 for v in arch]
        self.mask_transformation = get_mask_transformation(
            observation_mask=self.observation_mask, loss_mask=self.loss_mask).cpu().numpy()
        self.MSE_criterion = torch.nn.MSELoss(reduction=self.reduction)
        self.CE_criterion = torch.nn.NLLLoss(reduction=self.reduction)

    def __call__(self, x, y, as_numpy=False):
        if self.reduction == "mean":
            return self._mean_loss(x, y, as_numpy)
        if self.reduction == "none":
            return self._full_loss(x, y, as_numpy)
        raise Exception("Unknown reduction type.")

    # ---- HIP path (tensors on a HIP device) -------------------------------------------------
    def _tables(self, dev):
        t = getattr(self, "_dev_tables", None)
        if t is None or t[0].device != dev:
            i32 = dict(dtype=torch.int32, device=dev)
            w = self.weight.reshape(-1).to(torch.float32)
            if w.numel() != len(self.arch):
                raise Exception("CombinedCriterion: one weight per variable is required on the HIP path")
            t = (torch.tensor([v["position"] for v in self.arch], **i32),
                 torch.tensor([v["size"] for v in self.arch], **i32),
                 torch.tensor([0 if v["type"] == "regression" else 1 for v in self.arch], **i32),
                 w.to(dev).contiguous(),
                 torch.zeros(len(self.arch), dtype=torch.float64, device=dev))
            self._dev_tables = t
        return t

    def _hip_mean(self, x, y):
        dev = y.device
        pos, size, typ, w, acc = self._tables(dev)
        x = x.detach().to(torch.float32).contiguous()
        y = y.to(torch.float32).contiguous()
        dy = torch.empty_like(y)
        loss = torch.zeros(1, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            _check(_hip_lib().codae_combined_loss_fwd_bwd(_ptr(x), _ptr(y), y.shape[0], y.shape[1], len(self.arch), _ptr(pos),
                                                          _ptr(size), _ptr(typ), _ptr(w), _ptr(acc), _ptr(dy), _ptr(loss),
                                                          _stream()))
        return loss[0].to(torch.float32), dy

    def _hip_full(self, x, y):
        dev = y.device
        pos, size, typ, _, _ = self._tables(dev)
        x = x.detach().to(torch.float32).contiguous()
        y = y.detach().to(torch.float32).contiguous()
        out = torch.empty((y.shape[0], len(self.arch)), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _check(_hip_lib().codae_combined_loss_full(_ptr(x), _ptr(y), y.shape[0], y.shape[1], len(self.arch), _ptr(pos),
                                                       _ptr(size), _ptr(typ), _ptr(out), _stream()))
        return out

    # ---- device-resident per-step accounting of the abalone sweep -----------------------------------
    def accumulate(self, x, y, mask_ids, corrupter, normalizer=None, first_scaled_column=0):
        """What script/train_dae_on_abalone.py:227-236 of the reference does on the host after every step - the monitor
        criterion of the de-normalised batch, `get_partial`, two `get_per_k`s and four running sums - as ONE launch that
        adds into fp64 tables on the device (codae_monitor_accumulate).  `mask_ids`: int32 device tensor = the Corrupter's
        mask-table row per sample (`corrupter.mask_ids(batch_indices, run)`); `normalizer`: a tool.Normalizer whose `undo` the
        script applies to columns >= first_scaled_column of x and y (None: none).  Nothing is copied to the host; read the
        epoch's tables with `accumulated()`."""
        dev = y.device
        pos, size, typ, _, _ = self._tables(dev)
        nv, k_max = len(self.arch), self.k_max
        if getattr(self, "_mon_acc", None) is None or self._mon_acc.device != dev:
            self._mon_acc = torch.zeros(2 + 2 * k_max * nv, dtype=torch.float64, device=dev)
            self._mon_undo = None
        if normalizer is not None and self._mon_undo is None:
            io = x.shape[1]
            sc = torch.ones(io, dtype=torch.float32, device=dev)
            mn = torch.zeros(io, dtype=torch.float32, device=dev)
            sc[first_scaled_column:] = normalizer.scale.to(dev, torch.float32)
            mn[first_scaled_column:] = normalizer.min.to(dev, torch.float32)
            self._mon_undo = (sc.contiguous(), mn.contiguous())
        x = x.detach().to(torch.float32).contiguous()
        y = y.detach().to(torch.float32).contiguous()
        us, um = self._mon_undo if normalizer is not None else (None, None)
        with torch.cuda.device(dev):
            _check(_hip_lib().codae_monitor_accumulate(_ptr(x), _ptr(y), y.shape[0], y.shape[1], nv, _ptr(pos), _ptr(size), _ptr(typ),
                                                       _ptr(us) if us is not None else None, _ptr(um) if um is not None else None,
                                                       _ptr(mask_ids), _ptr(corrupter.mask_table_u8), _ptr(corrupter.k_of_mask_i32),
                                                       k_max, _ptr(self._mon_acc), _stream()))
        self._mon_keep = (x, y, mask_ids)          # (alive until the stream has consumed them)

    def accumulated(self, reset=True):
        """(f, p, f_k [k_max, n_var], p_k [k_max, n_var]) summed over the accumulate() calls since the last reset: float64
        numpy, one device-to-host copy."""
        nv, k_max = len(self.arch), self.k_max
        a = self._mon_acc.cpu().numpy().copy()
        if reset:
            self._mon_acc.zero_()
        return float(a[0]), float(a[1]), a[2:2 + k_max * nv].reshape(k_max, nv), a[2 + k_max * nv:].reshape(k_max, nv)

    def _per_variable(self, x, y, v):
        p, s = v["position"], v["size"]
        xs, ys = x[:, p:p + s], y[:, p:p + s]
        if v["type"] == "regression":
            return self.MSE_criterion(input=xs, target=ys)
        return self.CE_criterion(input=torch.log_softmax(ys, dim=1), target=xs.max(dim=1)[1])

    def _full_loss(self, x, y, as_numpy=False):
        if y.device.type == "cuda":
            loss = self._hip_full(x, y).cpu()                   # upstream returns a host tensor (:133)
            return loss.numpy() if as_numpy else loss
        loss = torch.zeros((x.size()[0], len(self.arch)))       # on the host, as upstream (:133)
        for i, v in enumerate(self.arch):
            li = self._per_variable(x, y, v)
            if v["type"] == "regression":
                loss[:, i:i + 1] = li
            else:
                loss[:, i] = li
        if as_numpy:
            return loss.clone().cpu().detach().numpy()
        return loss

    def _mean_loss(self, x, y, as_numpy=False):
        if y.device.type == "cuda" and not as_numpy:
            return _CombinedMeanFn.apply(y, x, self)
        loss = []
        for v in self.arch:
            li = self._per_variable(x, y, v)
            loss.append(torch.sqrt(li) if v["type"] == "regression" else li)
        if as_numpy:
            out = sum(loss) / len(self.arch)
            return out.clone().cpu().detach().numpy()
        loss = [loss[i] * self.weight[i] for i in range(len(loss))]
        return sum(loss) / len(self.arch)

    def get_per_k(self, loss, masks):
        """Per-k column sums of `loss` over the rows whose mask blanks k variables
        (metering.py:187-197: matmul(mask, ones) clipped to 1 is a row indicator; times T it is
        that indicator spread over the variables)."""
        out = np.zeros((self.k_max, len(self.arch)))
        spread = self.mask_transformation.sum(axis=0).astype(np.float64)      # 1 per variable
        for i, mask in enumerate(masks):
            hit = (mask.sum(dim=1) > 0).cpu().numpy().astype(np.float64)
            out[i, :] = np.sum(hit[:, None] * spread[None, :] * loss, axis=0)
        return out

    def get_partial(self, loss, mask):
        return (1 - np.matmul(mask.cpu().numpy(), self.mask_transformation)) * loss
