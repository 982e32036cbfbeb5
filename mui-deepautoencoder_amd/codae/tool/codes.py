"""Outfit codes - the counterpart of "Outfit codes" in include/codae_hip.h: the latent vector of an outfit, and nearest
neighbours in code space ("which outfits look like this one?").

Layers are l = 0 .. L-1, h_0 is the input, h_{l+1} as codae.tool.norm defines it (activation, skip, norm; an evaluation forward:
no noise, no dropout).  A forward over the first k Linears, 1 <= k <= L-1, yields h_k - exactly what Linear k reads.  The code
is h_k for k = code_layers(schedule): the index, plus one, of the lowest hidden Linear whose schedule entry has no activation -
the z layer of every stack model.schedule.linear_stack builds.  A schedule without such a layer has no default: the caller
names k.

OutfitCodes holds a bank of codes [M, Z], its row norms and the dataset rows the entries stand for, and ranks it against query
codes by cosine (both norms clamped at 1e-8, fp32) under tool.ComplementRetriever.topk's contract - the bank is a one-slot
inventory with S = 1, E = Z, so the selection, the distinct-item folding and the ordering are the retriever's own.
HipEmbeddingTrainer.encode / encode_items / decode / code_index are the device route; forward_to states h_k in whole-tensor
torch ops with autograd for host tensors and drop-in loops.
"""
import numpy as np
import torch

from ..hip import HipError
from .residual import _act_tuple, _apply_act


def code_layers(schedule):
    """k of the definition above for a schedule of (in, out, activation) triples (the activation entry a bool as linear_stack
    writes it, a CODAE_ACT_* kind or the engine's 4-tuple); HipError when no hidden layer lacks an activation."""
    L = len(schedule)
    for l in range(L - 1):
        if _act_tuple(schedule[l][2])[0] == 0:
            return l + 1
    raise HipError("outfit codes: no hidden layer of the %d-layer schedule lacks an activation, so there is no default code layer; "
                   "pass layer=k with 1 <= k <= %d" % (L, L - 1))


def check_layer(who, k, L):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= L - 1:
        raise HipError("%s: layer must be an int in [1, %d], got %r" % (who, L - 1, k))
    return int(k)


class OutfitCodes:
    """OutfitCodes(bank [M, Z] fp32, rows=None, norm=None, layer=None, distinct=True).  rows: the dataset row each entry stands
    for (integers [M], distinct; None = 0 .. M-1); norm: the fp32 row norms of a device bank as codae_export_rows left them (None
    = the retriever computes them); layer: the k the codes were taken at (kept for the record).  distinct: bank rows that hold
    identical bytes are one entry, represented by their lowest row."""

    def __init__(self, bank, rows=None, norm=None, layer=None, distinct=True):
        if not torch.is_tensor(bank) or bank.dim() != 2 or bank.shape[0] < 1 or bank.shape[1] < 1 or bank.dtype != torch.float32:
            raise HipError("outfit codes: the bank must be an fp32 [M, Z] tensor with M, Z >= 1")
        self.bank = bank.detach().contiguous()
        M = int(bank.shape[0])
        self.layer, self.distinct = layer, bool(distinct)
        self.norm = norm
        if norm is not None and (not torch.is_tensor(norm) or tuple(norm.shape) != (M,) or norm.dtype != torch.float32 or norm.device != bank.device):
            raise HipError("outfit codes: norm must be an fp32 [%d] tensor on the bank's device" % M)
        if rows is None:
            self.rows = None
        else:
            r = torch.as_tensor(rows).detach().to("cpu", torch.long).reshape(-1)
            if r.numel() != M or (M and int(r.min()) < 0) or torch.unique(r).numel() != M:
                raise HipError("outfit codes: rows must name %d distinct dataset rows >= 0" % M)
            if M > 1 and not bool((r[1:] > r[:-1]).all()):
                # entries in ascending dataset row: "ties by ascending row" and "the lowest row represents identical entries" are
                # then the retriever's own candidate order
                r, order = torch.sort(r)
                order = order.to(self.bank.device)
                self.bank = self.bank[order].contiguous()
                if self.norm is not None:
                    self.norm = self.norm[order].contiguous()
            self.rows = r
        self._ret = None
        self._dev = {}
        # the precision of the engine that wrote the bank ("bf16": every value is a bf16 number), as code_index records it; None = unknown
        self.precision = None

    def cluster(self, k, iters=25, seed=0, init="rows", precision=None):
        """Spherical k-means over the bank: a tool.CodeClusters fitted on self.bank with self.norm and self.rows.  precision: the
        operand type of the scores, "f32" or "bf16"; None = "bf16" for a bank the bf16 engine wrote (its values are bf16 numbers
        already: only the centroids are rounded), "f32" otherwise - decided from the record code_index left, the bank is not
        scanned.  Every entry counts once: `distinct` plays no part."""
        from .clusters import CodeClusters
        if precision is None:
            precision = "bf16" if self.precision == "bf16" else "f32"
        return CodeClusters.fit(self.bank, k, norm=self.norm, rows=self.rows, iters=iters, seed=seed, init=init, precision=precision)

    @property
    def width(self):
        return int(self.bank.shape[1])

    def __len__(self):
        return int(self.bank.shape[0])

    def _retriever(self):
        from ..train import _ResidentInventory
        from .criteria import ComplementRetriever
        if self._ret is None:
            # the bank is a one-slot inventory: S = 1, E = Z; cand_norm comes from the export kernel's pass over it, not a second one
            self._ret = ComplementRetriever(_ResidentInventory(self.bank, 1, self.width), self.bank.device, distinct=self.distinct,
                                            row_norms=self.norm)
        return self._ret

    def _maps(self, dev):
        """(rows [M] on dev: bank position -> dataset row, pos on dev: dataset row -> bank position or -1), or None when they are
        the identity"""
        if self.rows is None:
            return None
        m = self._dev.get(dev)
        if m is None:
            pos = torch.full((int(self.rows.max()) + 1,), -1, dtype=torch.long)
            pos[self.rows] = torch.arange(self.rows.numel())
            m = self._dev[dev] = (self.rows.to(dev), pos.to(dev))
        return m

    def similar(self, query, k, exclude=None, chunk=8192):
        """The k bank entries closest (cosine) to every query code: (idx LongTensor [Q, k] dataset rows, score FloatTensor [Q, k]),
        ordered by score descending and then by ascending row, NaN never returned, a short list ending in (-1, -inf).  query:
        [Q, Z] on the bank's device - the output of encode / encode_items with any blank.  exclude: integer [Q] or None, one
        dataset row per query that is never returned (with `distinct`, the entry it belongs to); the usual case is the query's
        own row.  chunk: bank entries per GEMM + selection pass on the device."""
        if not torch.is_tensor(query) or query.dim() != 2 or query.shape[0] < 1 or query.shape[1] != self.width:
            raise HipError("similar(): query must be a [Q, %d] tensor with Q >= 1, got %s" % (
                self.width, tuple(query.shape) if torch.is_tensor(query) else type(query).__name__))
        if query.device != self.bank.device:
            raise HipError("similar(): the query is on %s, the bank on %s" % (query.device, self.bank.device))
        ret = self._retriever()
        dev = self.bank.device
        maps = self._maps(dev)
        ex = exclude
        if ex is not None:
            if not torch.is_tensor(ex):
                ex = torch.as_tensor(ex)
            if ex.dim() != 1 or ex.shape[0] != query.shape[0] or ex.dtype.is_floating_point or ex.dtype == torch.bool:
                raise HipError("similar(): exclude must be an integer [Q] tensor of dataset rows")
            ex = ex.to(dev).long()
            if maps is not None:
                ok = (ex >= 0) & (ex < maps[1].numel())
                ex = torch.where(ok, maps[1][ex.clamp(0, maps[1].numel() - 1)], torch.full_like(ex, -1))
        idx, score = ret.topk(query, 0, k, exclude=ex, chunk=chunk)
        if maps is not None:
            idx = torch.where(idx >= 0, maps[0][idx.clamp_min(0)], idx)
        return idx, score

    @staticmethod
    def forward_to(x, weights, biases, activation, layers, residual=None, norm=None, sparse=None):
        """h_layers of the definition in whole-tensor torch ops (autograd works through it): weights[l] [out, in], biases[l]
        [out]; activation per layer as Norm.resolve takes it; residual / norm / sparse: None or the codae.tool.Residual / Norm /
        SparseCode of the stack.  The counterpart of Norm.forward and Residual.forward, stopped behind Linear layers - 1."""
        L = len(weights)
        k = check_layer("forward_to", layers, L)
        if sparse is not None:
            return sparse.forward(x, weights, biases, activation, residual=residual, norm=norm, layers=k)
        acts = [_act_tuple(a) for a in activation]
        ins, outs = [int(w.shape[1]) for w in weights], [int(w.shape[0]) for w in weights]
        skips = residual.resolve(ins, outs, acts) if residual is not None else [0] * L
        flags = norm.resolve(ins, outs, acts) if norm is not None else [0] * L
        h = x
        for l in range(k):
            a = _apply_act(acts[l], h @ weights[l].t() + biases[l])
            s = a + h if skips[l] else a
            h = norm.normalise(s) if flags[l] else s
        return h


_KEYS = {"SAVE": True, "LAYER": None, "NEIGHBOURS": 0, "DISTINCT": True}


def codes_from_config(block):
    """The `HIP: CODES:` block of the embedding script's config: {SAVE: true, LAYER: null, NEIGHBOURS: 0, DISTINCT: true} ->
    {"save", "layer", "neighbours", "distinct"}; None / empty -> None (nothing is encoded, logged or written)."""
    if not block:
        return None
    if not isinstance(block, dict):
        raise HipError("CODES must be a mapping with SAVE, LAYER, NEIGHBOURS and DISTINCT, got %r" % (block,))
    extra = sorted(set(block) - set(_KEYS), key=str)
    if extra:
        raise HipError("CODES: unknown key(s) %s (known: %s)" % (", ".join(map(str, extra)), ", ".join(sorted(_KEYS))))
    layer = block.get("LAYER", None)
    if layer is not None and (isinstance(layer, bool) or not isinstance(layer, int) or layer < 1):
        raise HipError("CODES: LAYER must be null or an int >= 1, got %r" % (layer,))
    nb = block.get("NEIGHBOURS", 0)
    if isinstance(nb, bool) or not isinstance(nb, int) or not 0 <= nb <= 256:
        raise HipError("CODES: NEIGHBOURS must be an int in [0, 256], got %r" % (nb,))
    for key in ("SAVE", "DISTINCT"):
        if not isinstance(block.get(key, True), bool):
            raise HipError("CODES: %s must be true or false, got %r" % (key, block.get(key)))
    if not block.get("SAVE", True):
        return None
    return {"save": True, "layer": layer, "neighbours": int(nb), "distinct": bool(block.get("DISTINCT", True))}
