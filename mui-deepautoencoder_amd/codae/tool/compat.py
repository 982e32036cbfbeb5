"""Assembled outfits and compatibility (include/codae_hip.h, "Assembled outfits and compatibility": the one definition the kernels, the
torch forms here and the tests' reference share).

An assembled outfit names its items per slot: items[q][s] = r says slot s of outfit q holds the slot-s item of dataset row r, a
negative value that the outfit has no item there - so a query can mix the items of different rows, which a batch of row indices
cannot.  Compatibility holds the definitions as static methods: `assemble` builds the model's input (one slot blanked, or the S
leave-one-out rows of every outfit), `slot_scores` compares each left-out item with its reconstruction and averages the cosines
into one score per outfit, `auc` counts how often real outfits score above outfits with one item swapped, `negatives` draws those
swapped outfits.  Device tensors run the kernels of csrc/compat.hip without a host synchronisation; host tensors (and drop-in
loops) the same definitions in whole-tensor torch ops.  CompatibilityMetrics is the validation metric built from them.

Not covered: training on the negatives, the mixed-variable (abalone) path, data-parallel reduction of the counts (each rank scores
what it is given).
"""
import numpy as np
import torch

from ..hip import AUC_PAIRED, AUC_PAIRS, AUC_STRIDE, AUC_TIES, AUC_WINS, HipError
from ..hip import check as _check, current_stream as _stream, lib as _hip_lib, ptr as _ptr

COS_EPS = 1e-8          # CODAE_COS_EPS
MAX_SLOTS = 128


def _presence_table(presence, n_rows, S):
    """uint8 numpy [n_rows, S] or None from a SlotPresence, an array or a tensor."""
    table = getattr(presence, "table", presence)
    if table is None:
        return None
    table = np.asarray(table.detach().cpu().numpy() if hasattr(table, "detach") else table)
    if table.shape != (n_rows, S):
        raise HipError("compatibility: the presence table must be [%d, %d], got shape %r" % (n_rows, S, tuple(table.shape)))
    return np.ascontiguousarray(table != 0).astype(np.uint8)


def _presence_on(presence, n_rows, S, device):
    t = _presence_table(presence, n_rows, S)
    if t is None or bool(t.all()):
        return None
    if hasattr(presence, "to") and hasattr(presence, "assign_masks"):
        return presence.to(device)                    # (SlotPresence caches its device copies)
    return torch.from_numpy(t).to(device).contiguous()


def _check_items(items, S=None):
    if not torch.is_tensor(items):
        items = torch.as_tensor(np.asarray(items))
    if items.dim() != 2 or items.dtype.is_floating_point or items.dtype == torch.bool or items.shape[0] < 1:
        raise HipError("compatibility: items must be an integer [Q, S] tensor with Q >= 1, got %s %s" % (items.dtype, tuple(items.shape)))
    if S is not None and items.shape[1] != S:
        raise HipError("compatibility: items has %d slots, expected %d" % (items.shape[1], S))
    if not 1 <= items.shape[1] <= MAX_SLOTS:
        raise HipError("compatibility: 1 .. %d slots, got %d" % (MAX_SLOTS, items.shape[1]))
    return items


def _check_data(data, S):
    if not torch.is_tensor(data) or data.dim() != 2 or data.shape[0] < 1 or data.shape[1] % S != 0:
        raise HipError("compatibility: data must be [N, io] with %d slots dividing io" % S)
    return int(data.shape[0]), int(data.shape[1]), int(data.shape[1]) // S


class Compatibility:
    """The definitions, each for device tensors (kernels) and host tensors (torch ops)."""

    # ---- assemble --------------------------------------------------------------------------------------------------------
    @staticmethod
    def assemble(data, items, blank=None, leave_one_out=False, presence=None, out_dtype=None, out=None):
        """X[row][s E + e] = data[items[q][s]][s E + e], +0 where the pair (q, s) is absent or slot s is blanked for the row.
        data: [N, io] fp32, or the bf16 image of it (then the result is bf16).  blank: integer [Q] (negative: none) or None - one
        row per outfit; leave_one_out: S rows per outfit, row q S + v has slot v blanked.  presence: a SlotPresence / uint8 [N, S]
        table - a pair it marks absent is absent whatever data holds there.  out_dtype: torch.float32 (default for fp32 data) or
        torch.bfloat16.  out (device only): a [rows, ld >= io] tensor to assemble into."""
        items = _check_items(items)
        Q, S = int(items.shape[0]), int(items.shape[1])
        N, io, E = _check_data(data, S)
        if data.dtype not in (torch.float32, torch.bfloat16):
            raise HipError("compatibility: data must be fp32 or its bf16 image, got %s" % data.dtype)
        if leave_one_out and blank is not None:
            raise HipError("compatibility: the leave-one-out form takes no blank vector")
        if out_dtype is None:
            out_dtype = data.dtype if out is None else out.dtype
        if out_dtype not in (torch.float32, torch.bfloat16) or (data.dtype == torch.bfloat16 and out_dtype != torch.bfloat16):
            raise HipError("compatibility: cannot assemble %s rows into %s" % (data.dtype, out_dtype))
        if blank is not None:
            blank = torch.as_tensor(blank)
            if blank.dim() != 1 or blank.shape[0] != Q or blank.dtype.is_floating_point:
                raise HipError("compatibility: blank must be an integer [Q] tensor")
        rows = Q * S if leave_one_out else Q
        if data.device.type == "cuda":
            dev = data.device
            if not data.is_contiguous():
                raise HipError("compatibility: data must be contiguous")
            it = items.to(device=dev, dtype=torch.int32).contiguous()
            bl = None if blank is None else blank.to(device=dev, dtype=torch.int32).contiguous()
            pres = _presence_on(presence, N, S, dev)
            if out is None:
                out = torch.empty((rows, io), dtype=out_dtype, device=dev)
            elif out.dim() != 2 or out.shape[0] != rows or out.shape[1] < io or out.stride(1) != 1 or out.dtype != out_dtype or out.device != dev:
                raise HipError("compatibility: out must be a [%d, >= %d] %s tensor on %s" % (rows, io, out_dtype, dev))
            with torch.cuda.device(dev):
                _check(_hip_lib().codae_assemble_outfits(_ptr(data), int(data.dtype == torch.bfloat16), N, io, S, _ptr(it), Q, _ptr(bl),
                                                         int(bool(leave_one_out)), _ptr(pres), _ptr(out), int(out_dtype == torch.bfloat16),
                                                         int(out.stride(0)), _stream()))
            Compatibility._keep = (data, it, bl, pres)          # (alive until the stream has consumed them)
            return out[:, :io]
        it = items.to("cpu", torch.long)
        on = (it >= 0) & (it < N)
        r = it.clamp(0, N - 1)
        table = _presence_table(presence, N, S)
        cols = torch.arange(S)
        if table is not None:
            on &= torch.from_numpy(table)[r, cols[None, :]] != 0
        X = data.detach().to("cpu").reshape(N, S, E)[r, cols[None, :]]          # [Q, S, E]
        if leave_one_out:
            on = on[:, None, :] & (cols[None, :, None] != cols[None, None, :])      # [Q, v, s]
            X = X[:, None].expand(Q, S, S, E)
        elif blank is not None:
            on = on & (cols[None, :] != blank.to("cpu", torch.long)[:, None])
        X = torch.where(on[..., None], X, torch.zeros((), dtype=X.dtype))
        return X.reshape(rows, io).to(out_dtype)

    # ---- slot scores -----------------------------------------------------------------------------------------------------
    @staticmethod
    def slot_scores(data, items, Y, presence=None):
        """data [N, io] fp32, items [Q, S], Y [Q S, io] fp32 = the model's output for assemble(..., leave_one_out=True) ->
        {"cos": [Q, S], "sq": [Q, S], "score": [Q], "n_present": [Q] int32}: for a present pair cos = dot / (max(|x|, eps)
        max(|y|, eps)) and sq = sum (x - y)^2 between x = data[items[q][s]][slot s] and y = Y[q S + s][slot s], 0 for an absent one;
        score = the mean of the present cosines (added in ascending slot order), NaN with fewer than two."""
        items = _check_items(items)
        Q, S = int(items.shape[0]), int(items.shape[1])
        N, io, E = _check_data(data, S)
        if data.dtype != torch.float32 or not torch.is_tensor(Y) or Y.dtype != torch.float32 or Y.dim() != 2 or tuple(Y.shape) != (Q * S, io):
            raise HipError("compatibility: slot_scores takes fp32 data and an fp32 Y of shape [%d, %d]" % (Q * S, io))
        if data.device.type == "cuda":
            dev = data.device
            if Y.device != dev or not data.is_contiguous() or Y.stride(1) != 1:
                raise HipError("compatibility: data and Y must be contiguous on %s" % dev)
            it = items.to(device=dev, dtype=torch.int32).contiguous()
            pres = _presence_on(presence, N, S, dev)
            f32 = dict(dtype=torch.float32, device=dev)
            res = {"cos": torch.empty((Q, S), **f32), "sq": torch.empty((Q, S), **f32), "score": torch.empty(Q, **f32),
                   "n_present": torch.empty(Q, dtype=torch.int32, device=dev)}
            with torch.cuda.device(dev):
                _check(_hip_lib().codae_outfit_scores(_ptr(data), N, io, S, _ptr(it), Q, _ptr(pres), _ptr(Y), int(Y.stride(0)), _ptr(res["cos"]),
                                                      _ptr(res["sq"]), _ptr(res["score"]), _ptr(res["n_present"]), _stream()))
            Compatibility._keep = (data, it, pres, Y)
            return res
        it = items.to("cpu", torch.long)
        on = (it >= 0) & (it < N)
        r = it.clamp(0, N - 1)
        cols = torch.arange(S)
        table = _presence_table(presence, N, S)
        if table is not None:
            on &= torch.from_numpy(table)[r, cols[None, :]] != 0
        zero = torch.zeros((), dtype=torch.float32)
        x = torch.where(on[..., None], data.detach().to("cpu").reshape(N, S, E)[r, cols[None, :]], zero)
        y = Y.detach().to("cpu").reshape(Q, S, S, E)[:, cols, cols]                  # [Q, S, E]: row q S + s, slot s
        eps = torch.tensor(COS_EPS, dtype=torch.float32)
        nx, ny = (x * x).sum(-1).sqrt(), (y * y).sum(-1).sqrt()
        nx, ny = torch.where(nx < eps, eps, nx), torch.where(ny < eps, eps, ny)      # max(., eps) that keeps a NaN norm a NaN
        cos = torch.where(on, (x * y).sum(-1) / (nx * ny), zero)
        sq = torch.where(on, ((x - y) ** 2).sum(-1), zero)
        acc = torch.zeros(Q, dtype=torch.float32)
        for s in range(S):                                                           # ascending slots, fp32
            acc = torch.where(on[:, s], acc + cos[:, s], acc)
        n = on.sum(1).to(torch.int32)
        score = torch.where(n >= 2, acc / n.clamp_min(1).to(torch.float32), torch.full((), float("nan")))
        return {"cos": cos, "sq": sq, "score": score, "n_present": n}

    # ---- AUC -------------------------------------------------------------------------------------------------------------
    @staticmethod
    def auc(scores_pos, scores_neg, neg_slot, n_slots, neg_parent=None, pos_on=None):
        """int64 [n_slots + 1, AUC_STRIDE] counts (CODAE_AUC_*): row s = {wins, ties, pairs, paired wins} of the negatives whose swapped
        slot is s against every positive, row n_slots = {live positives, live negatives, 0, 0}.  A win is pos > neg, a tie pos ==
        neg, everything else - NaN on either side included - a loss.  neg_parent [M]: the positive each negative was made from
        (paired wins count pos[parent] > neg); pos_on [P] uint8: positives that are off take part in nothing, nor do negatives
        whose slot lies outside [0, n_slots) or whose parent is off.  The counts stay on the device of the scores; summary()
        turns them into the metrics."""
        S = int(n_slots)
        if not 1 <= S <= MAX_SLOTS:
            raise HipError("compatibility: 1 .. %d slots, got %d" % (MAX_SLOTS, S))
        for name, t in (("scores_pos", scores_pos), ("scores_neg", scores_neg)):
            if not torch.is_tensor(t) or t.dim() != 1 or t.dtype != torch.float32 or t.numel() < 1:
                raise HipError("compatibility: %s must be a non-empty fp32 vector" % name)
        P, M = int(scores_pos.numel()), int(scores_neg.numel())
        dev = scores_pos.device
        for name, t, n in (("neg_slot", neg_slot, M), ("neg_parent", neg_parent, M), ("pos_on", pos_on, P)):
            if t is not None and (not torch.is_tensor(t) or t.dim() != 1 or t.numel() != n or t.dtype.is_floating_point):
                raise HipError("compatibility: %s must be an integer vector of %d entries" % (name, n))
        if neg_slot is None:
            raise HipError("compatibility: auc needs neg_slot")
        if dev.type == "cuda":
            pos, neg = scores_pos.contiguous(), scores_neg.to(dev).contiguous()
            sl = neg_slot.to(device=dev, dtype=torch.int32).contiguous()
            par = None if neg_parent is None else neg_parent.to(device=dev, dtype=torch.int32).contiguous()
            on = None if pos_on is None else pos_on.to(device=dev, dtype=torch.uint8).contiguous()
            ws = torch.empty(int(_hip_lib().codae_auc_blocks(M)) * S * 3, dtype=torch.int64, device=dev)
            counts = torch.empty((S + 1, AUC_STRIDE), dtype=torch.int64, device=dev)
            with torch.cuda.device(dev):
                _check(_hip_lib().codae_auc_counts(_ptr(pos), _ptr(on), P, _ptr(neg), _ptr(sl), _ptr(par), M, S, _ptr(ws), _ptr(counts), _stream()))
            Compatibility._keep = (pos, neg, sl, par, on, ws)
            return counts
        pos, neg = scores_pos.detach(), scores_neg.detach().to("cpu")
        sl = neg_slot.to("cpu", torch.long)
        live_p = torch.ones(P, dtype=torch.bool) if pos_on is None else pos_on.to("cpu") != 0
        live_n = (sl >= 0) & (sl < S)
        par = None
        if neg_parent is not None:
            par = neg_parent.to("cpu", torch.long)
            if pos_on is not None:
                ok = (par >= 0) & (par < P)
                live_n &= ok & live_p[par.clamp(0, P - 1)]
        counts = torch.zeros((S + 1, AUC_STRIDE), dtype=torch.int64)
        slc = sl.clamp(0, S - 1)
        for j0 in range(0, M, 4096):                                                # a [P, chunk] comparison at a time
            j1 = min(M, j0 + 4096)
            v, keep = neg[j0:j1], (live_p[:, None] & live_n[None, j0:j1])
            counts[:S, AUC_WINS].index_add_(0, slc[j0:j1], ((pos[:, None] > v[None, :]) & keep).sum(0))
            counts[:S, AUC_TIES].index_add_(0, slc[j0:j1], ((pos[:, None] == v[None, :]) & keep).sum(0))
        n_neg = torch.zeros(S, dtype=torch.int64).index_add_(0, slc, live_n.to(torch.int64))
        counts[:S, AUC_PAIRS] = int(live_p.sum()) * n_neg
        if par is not None:
            ok = live_n & (par >= 0) & (par < P)
            pw = ok & live_p[par.clamp(0, P - 1)] & (pos[par.clamp(0, P - 1)] > neg)
            counts[:S, AUC_PAIRED].index_add_(0, slc, pw.to(torch.int64))
        counts[S, 0], counts[S, 1] = int(live_p.sum()), int(n_neg.sum())
        return counts

    @staticmethod
    def summary(counts, skipped=0):
        """{auc, paired_acc, pairs, outfits, skipped, per_slot: [{auc, pairs, wins, ties, paired_acc, negatives}], counts} from the
        counts of auc() (a host copy is made: one device-to-host read).  auc = (wins + ties / 2) / pairs; NaN where there is no pair."""
        c = np.asarray(counts.detach().cpu().numpy() if hasattr(counts, "detach") else counts).astype(np.int64)
        S = c.shape[0] - 1
        n_pos, n_neg = int(c[S, 0]), int(c[S, 1])

        def ratio(a, b):
            return float(a) / float(b) if b else float("nan")

        per = []
        for s in range(S):
            w, t, p, pw = (int(v) for v in c[s, :4])
            negs = p // n_pos if n_pos else 0
            per.append({"auc": ratio(w + 0.5 * t, p), "pairs": p, "wins": w, "ties": t, "paired_acc": ratio(pw, negs), "negatives": negs})
        w, t, p, pw = (int(c[:S, f].sum()) for f in (AUC_WINS, AUC_TIES, AUC_PAIRS, AUC_PAIRED))
        return {"auc": ratio(w + 0.5 * t, p), "paired_acc": ratio(pw, n_neg), "pairs": p, "outfits": n_pos, "skipped": int(skipped),
                "per_slot": per, "counts": c}

    # ---- negatives -------------------------------------------------------------------------------------------------------
    @staticmethod
    def negatives(dataset, validation_indices, negatives=1, seed=0, presence=None, distinct=True):
        """The swapped outfits of a validation set, drawn on the host from a CPU torch.Generator seeded with `seed`.  dataset: an
        object with nb_used_category, embedding_size and data_per_category (as ComplementRetriever takes).  For every validation row
        r (ascending) with at least two present slots and every draw j < negatives: a slot s uniform among r's present slots, a donor
        uniform among the validation rows that have slot s and hold a different item there (`distinct`: different bytes, by the
        grouping of ComplementRetriever._host_tables; else a different row); the negative is r's items with entry s replaced by the
        donor.  ->
          rows [P] int64 the scored rows; pos_items [P, S] int32 (r where present, else -1); neg_items [P, J, S] int32 (all -1: a
          skipped draw); neg_slot [P, J] int32 (-1: skipped); neg_parent [P, J] int32 (= the index into rows); skipped: rows with
          fewer than two present slots plus draws without any donor."""
        from .criteria import ComplementRetriever, _OneSlot
        S = int(dataset.nb_used_category)
        n_obs = int(dataset.data_per_category[0].shape[0])
        if isinstance(negatives, bool) or not isinstance(negatives, (int, np.integer)) or int(negatives) < 1:
            raise HipError("compatibility: negatives must be an int >= 1, got %r" % (negatives,))
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
            raise HipError("compatibility: seed must be an int, got %r" % (seed,))
        J = int(negatives)
        rows = torch.as_tensor(list(validation_indices) if not torch.is_tensor(validation_indices) else validation_indices, dtype=torch.long).reshape(-1)
        if rows.numel() == 0 or int(rows.min()) < 0 or int(rows.max()) >= n_obs:
            raise HipError("compatibility: validation_indices must be a non-empty list of dataset rows in [0, %d)" % n_obs)
        rows = torch.unique(rows)
        table = _presence_table(presence, n_obs, S)
        pres = torch.ones((rows.numel(), S), dtype=torch.bool) if table is None else torch.from_numpy(table)[rows] != 0
        n_r = pres.sum(1)
        scored = n_r >= 2
        skipped = int((~scored).sum())
        prow, ppres, pn = rows[scored], pres[scored], n_r[scored]
        P = int(prow.numel())
        pos_items = torch.where(ppres, prow[:, None].expand(P, S), torch.full((), -1, dtype=torch.long))
        g = torch.Generator(device="cpu")
        g.manual_seed(int(seed))
        u = torch.rand((P, J, 2), generator=g, dtype=torch.float64)
        # the slot: the floor(u n_r)-th present slot of the row
        k1 = torch.minimum((u[:, :, 0] * pn[:, None]).floor().long(), pn[:, None] - 1)
        slot = ((ppres.long().cumsum(1)[:, None, :] == (k1 + 1)[:, :, None]) & ppres[:, None, :]).long().argmax(2) if P else k1
        donor = torch.full((P, J), -1, dtype=torch.long)
        parent_row = prow[:, None].expand(P, J)
        for s in range(S):
            rs = rows[pres[:, s]]                              # the validation rows that have the slot, ascending
            sel = slot == s
            if rs.numel() == 0 or not bool(sel.any()):
                continue
            item = ComplementRetriever(_OneSlot(dataset, s), "cpu", candidates=rs, distinct=distinct)._host_tables()[3][0].long()
            order = torch.sort(item[rs], stable=True)[1]
            by_item, sorted_item = rs[order], item[rs][order]
            it = item[parent_row[sel]]
            g0 = torch.searchsorted(sorted_item, it, right=False)
            gs = torch.searchsorted(sorted_item, it, right=True) - g0
            count = rs.numel() - gs                            # rows that hold another item
            k2 = torch.minimum((u[:, :, 1][sel] * count).floor().long(), (count - 1).clamp_min(0))
            k2 = k2 + (k2 >= g0).long() * gs                   # skip the parent's own group
            donor[sel] = torch.where(count > 0, by_item[k2.clamp(0, rs.numel() - 1)], torch.full((), -1, dtype=torch.long))
        drawn = donor >= 0
        skipped += int((~drawn).sum())
        neg_items = pos_items[:, None, :].expand(P, J, S).clone()
        if P:
            neg_items.scatter_(2, slot[:, :, None], donor[:, :, None])
        neg_items = torch.where(drawn[:, :, None], neg_items, torch.full((), -1, dtype=torch.long))
        neg_slot = torch.where(drawn, slot, torch.full((), -1, dtype=torch.long))
        return {"rows": prow, "pos_items": pos_items.to(torch.int32), "neg_items": neg_items.to(torch.int32),
                "neg_slot": neg_slot.to(torch.int32), "neg_parent": torch.arange(P, dtype=torch.int32)[:, None].expand(P, J).contiguous(),
                "skipped": skipped}


class CompatibilityMetrics:
    """Compatibility prediction over a validation set: the AUC of the real outfits' scores against the scores of outfits with one
    item swapped (Compatibility.negatives, drawn once here), per swapped slot and in total, and the paired accuracy - the share of
    negatives that score below the outfit they were made from.

    dataset: as ComplementRetriever takes it (nb_used_category, embedding_size, data_per_category).  A validation row is an outfit of
    the items it has (`presence`); rows with fewer than two are skipped.  add() stores the scores of a batch in their places on
    `device` (no host synchronisation: a row added twice is stored once), total() runs one count of every stored positive against
    every stored negative (codae_auc_counts) and reads the counts: one device-to-host read.  get() is the same in torch ops on host
    copies."""

    def __init__(self, dataset, validation_indices, device, negatives=1, seed=0, presence=None, distinct=True):
        self.device = torch.device(device)
        self.S = int(dataset.nb_used_category)
        self.n_obs = int(dataset.data_per_category[0].shape[0])
        self.negatives, self.seed, self.distinct = int(negatives) if not isinstance(negatives, bool) else negatives, seed, bool(distinct)
        self.table = Compatibility.negatives(dataset, validation_indices, negatives=negatives, seed=seed, presence=presence, distinct=distinct)
        self.skipped = int(self.table["skipped"])
        self.trainer = None                    # bound by HipEmbeddingTrainer.compatibility_metrics: add_batch(row_idx) then suffices
        t, dev, S, J = self.table, self.device, self.S, int(negatives)
        P = self.P = int(t["rows"].numel())
        # one trash place behind the P real ones: where the rows that are no outfit (fewer than two items) go, never counted
        pos_of_row = torch.full((self.n_obs,), P, dtype=torch.long)
        pos_of_row[t["rows"]] = torch.arange(P)
        trash = torch.full((1, S), -1, dtype=torch.int32)
        self.pos_of_row = pos_of_row.to(dev)
        self.pos_items = torch.cat([t["pos_items"], trash]).to(dev).contiguous()
        self.neg_items = torch.cat([t["neg_items"], trash[None].expand(1, J, S)]).to(dev).contiguous()
        self.neg_slot = t["neg_slot"].reshape(-1).to(dev).contiguous()
        self.neg_parent = t["neg_parent"].reshape(-1).to(dev).contiguous()
        nan = float("nan")
        self.pos_score = torch.full((P + 1,), nan, dtype=torch.float32, device=dev)
        self.neg_score = torch.full((P + 1, J), nan, dtype=torch.float32, device=dev)
        self.pos_on = torch.zeros(P + 1, dtype=torch.uint8, device=dev)

    def places(self, row_idx):
        """The place of every dataset row of `row_idx` among the scored outfits (P: the row is none), on the metric's device."""
        return self.pos_of_row[torch.as_tensor(row_idx).to(self.device).long()]

    def add(self, scores_pos, scores_neg, places):
        """scores_pos [B], scores_neg [B, negatives] fp32 and places [B] (places(row_idx)) of one batch: stored, not yet counted."""
        J = self.neg_score.shape[1]
        if scores_pos.dim() != 1 or tuple(scores_neg.shape) != (scores_pos.shape[0], J) or places.shape != scores_pos.shape:
            raise HipError("compatibility metrics: add takes scores [B], [B, %d] and places [B]" % J)
        places = places.to(self.device).long()
        self.pos_score[places] = scores_pos.to(self.device, torch.float32)
        self.neg_score[places] = scores_neg.to(self.device, torch.float32)
        self.pos_on[places] = 1

    def add_batch(self, *args, weights="live"):
        """add_batch(row_idx) on a metric bound to a trainer, or add_batch(trainer, row_idx): scores the outfits of dataset rows
        `row_idx` and their negatives with trainer.score_outfits (weights: "live" or "average") and stores them."""
        if len(args) == 2:
            trainer, row_idx = args
        elif len(args) == 1 and self.trainer is not None:
            trainer, row_idx = self.trainer, args[0]
        else:
            raise HipError("compatibility metrics: add_batch(row_idx) needs a metric bound to a trainer; else add_batch(trainer, row_idx)")
        places = self.places(row_idx)
        B, J = int(places.numel()), self.neg_score.shape[1]
        if B == 0:
            return
        items = torch.cat([self.pos_items[places], self.neg_items[places].reshape(B * J, self.S)]).contiguous()
        score = trainer.score_outfits(items, weights=weights)["score"]
        self.add(score[:B], score[B:].reshape(B, J), places)

    def _count(self, host):
        P, J = self.P, self.neg_score.shape[1]
        if P == 0:
            return torch.zeros((self.S + 1, AUC_STRIDE), dtype=torch.int64)
        to = (lambda t: t.cpu()) if host else (lambda t: t)
        return Compatibility.auc(to(self.pos_score[:P]), to(self.neg_score[:P].reshape(P * J)), to(self.neg_slot), self.S,
                                 neg_parent=to(self.neg_parent), pos_on=to(self.pos_on[:P]))

    def total(self, reset=True):
        """{auc, paired_acc, pairs, outfits, skipped, per_slot: [...], counts} of the outfits add()ed since the last reset: one count
        on the metric's device, one device-to-host read."""
        out = Compatibility.summary(self._count(host=False), self.skipped)
        if reset:
            self.pos_on.zero_()
        return out

    def get(self, reset=False):
        """total() in whole-tensor torch ops on host copies of the stored scores."""
        out = Compatibility.summary(self._count(host=True), self.skipped)
        if reset:
            self.pos_on.zero_()
        return out


def compatibility_from_config(block):
    """The `HIP: COMPATIBILITY:` block of the embedding script's config: {NEGATIVES: 1, SEED: 0, DISTINCT: true}.  None -> None (the
    script then runs, logs and writes exactly what it does without the key); else the keyword arguments of CompatibilityMetrics /
    HipEmbeddingTrainer.compatibility_metrics: {"negatives": int, "seed": int, "distinct": bool}."""
    if block is None:
        return None
    if not isinstance(block, dict):
        raise HipError("COMPATIBILITY must be a mapping, got %r" % (block,))
    known = {"NEGATIVES", "SEED", "DISTINCT"}
    extra = sorted(set(map(str, block)) - known)
    if extra:
        raise HipError("COMPATIBILITY: unknown key(s) %s (known: %s)" % (", ".join(extra), ", ".join(sorted(known))))
    negatives, seed, distinct = block.get("NEGATIVES", 1), block.get("SEED", 0), block.get("DISTINCT", True)
    if isinstance(negatives, bool) or not isinstance(negatives, int) or negatives < 1:
        raise HipError("COMPATIBILITY: NEGATIVES must be an int >= 1, got %r" % (negatives,))
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise HipError("COMPATIBILITY: SEED must be an int, got %r" % (seed,))
    if not isinstance(distinct, bool):
        raise HipError("COMPATIBILITY: DISTINCT must be true or false, got %r" % (distinct,))
    return {"negatives": negatives, "seed": seed, "distinct": distinct}
