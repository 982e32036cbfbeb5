"""Code clusters - the counterpart of "Code clusters" in include/codae_hip.h: spherical k-means over a bank of outfit codes ("which
kinds of outfit are there, and to which does this one belong?").

The metric is the cosine, as in OutfitCodes.similar.  x [M, Z] is the bank, n_r its fp32 row norms, c [K, Z] fp32 centroids,
eps = 1e-8, op(v) = v in the "f32" form and v rounded to bf16 in the "bf16" form:
  nearest   d[r][j] = sum_z op(x[r][z]) op(c[j][z]) in fp32; assign[r] = the lowest j that reaches the maximum over the non-NaN
            d[r][.] (-0 == +0), -1 when all are NaN; best[r] = d[r][assign[r]] / max(n_r, eps), NaN when assign[r] = -1
  update    sum_j = sum over the members of j of x[r] / max(n_r, eps); c'[j] = sum_j / max(|sum_j|, eps), c[j] bit for bit when j has
            no member; rows with assign = -1 belong to nobody
  fit       for i < iters: a_i = nearest(c_i), changed[i] = #{a_i != a_{i-1}} (changed[0] = M), objective[i] = the float64 mean of
            best over the assigned rows, c_{i+1} = update(a_i, c_i); then assign = nearest(c_iters) with its best, mean and counts
Device tensors take the two kernels (codae_nearest_centroid, codae_centroid_update), host tensors the same definitions in
whole-tensor torch ops.  No step of a fit waits for the device; converged_at reads `changed` when it is asked for.
"""
import numpy as np
import torch

from .. import hip
from ..hip import HipError

EPS = 1e-8
MAX_K = 4096


def _nearest_host(x, c, norm, bf16):
    xo, co = (x.bfloat16().float(), c.bfloat16().float()) if bf16 else (x, c)
    d = xo @ co.t()
    nan = torch.isnan(d)
    dm = torch.where(nan, torch.full_like(d, float("-inf")), d)
    top = dm.max(dim=1, keepdim=True).values
    K = int(c.shape[0])
    j = torch.arange(K, device=d.device).expand_as(d)
    assign = torch.where((dm == top) & ~nan, j, torch.full_like(j, K)).min(dim=1).values
    none = assign == K
    assign = torch.where(none, torch.full_like(assign, -1), assign)
    best = d.gather(1, assign.clamp_min(0)[:, None])[:, 0]
    if norm is not None:
        best = best / norm.clamp_min(EPS)
    return assign, torch.where(none, torch.full_like(best, float("nan")), best)


def _update_host(x, norm, assign, c):
    K = int(c.shape[0])
    live = assign >= 0
    a = assign[live]
    sums = torch.zeros_like(c).index_add_(0, a, x[live] / norm[live].clamp_min(EPS)[:, None])
    counts = torch.zeros(K, dtype=torch.long, device=c.device).index_add_(0, a, torch.ones_like(a))
    unit = sums / torch.linalg.vector_norm(sums, dim=1).clamp_min(EPS)[:, None]
    return torch.where((counts > 0)[:, None], unit, c), counts


class _DeviceRoute:
    """the two kernels over one bank: the work spaces are allocated once per fit / predict"""

    def __init__(self, Z, K, bf16, device):
        self.lib, self.Z, self.K, self.bf16, self.device = hip.lib(), Z, K, int(bf16), device
        n = int(self.lib.codae_nearest_centroid_ws_bytes(Z, K, self.bf16))
        if n < 0:
            raise HipError("code clusters: no work space for Z %d, K %d" % (Z, K))
        self.ws_near = torch.empty(n, dtype=torch.uint8, device=device)
        self.ws_upd = None

    def nearest(self, x, c, norm):
        M = int(x.shape[0])
        assign = torch.empty(M, dtype=torch.long, device=self.device)
        best = torch.empty(M, dtype=torch.float32, device=self.device)
        hip.check(self.lib.codae_nearest_centroid(hip.ptr(x), x.stride(0), M, self.Z, hip.ptr(c), c.stride(0), self.K, self.bf16,
                                                  hip.ptr(norm), hip.ptr(assign), hip.ptr(best), hip.ptr(self.ws_near),
                                                  hip.current_stream()))
        return assign, best

    def update(self, x, norm, assign, c):
        M = int(x.shape[0])
        if self.ws_upd is None:
            self.ws_upd = torch.empty(int(self.lib.codae_centroid_update_ws_bytes(M, self.Z, self.K)), dtype=torch.uint8, device=self.device)
        out = torch.empty_like(c)
        counts = torch.empty(self.K, dtype=torch.long, device=self.device)
        hip.check(self.lib.codae_centroid_update(hip.ptr(x), x.stride(0), M, self.Z, hip.ptr(norm), hip.ptr(assign), hip.ptr(c), hip.ptr(out),
                                                 out.stride(0), self.K, hip.ptr(counts), hip.ptr(self.ws_upd), hip.current_stream()))
        return out, counts


class _HostRoute:
    def __init__(self, bf16):
        self.bf16 = bf16

    def nearest(self, x, c, norm):
        return _nearest_host(x, c, norm, self.bf16)

    def update(self, x, norm, assign, c):
        return _update_host(x, norm, assign, c)


def _check_k(who, k, M=None):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= MAX_K:
        raise HipError("%s: k must be an int in [1, %d], got %r" % (who, MAX_K, k))
    if M is not None and int(k) > M:
        raise HipError("%s: k %d exceeds the bank's %d entries" % (who, int(k), M))
    return int(k)


def _route(Z, K, precision, device):
    if precision not in ("f32", "bf16"):
        raise HipError("code clusters: precision must be \"f32\" or \"bf16\", got %r" % (precision,))
    bf16 = precision == "bf16"
    return _DeviceRoute(Z, K, bf16, device) if device.type == "cuda" else _HostRoute(bf16)


class CodeClusters:
    """The result of CodeClusters.fit: centroids [K, Z] fp32, assign int64 [M] in bank order (-1: a row whose scores are all NaN),
    score [M] (the cosine to the own centroid), counts int64 [K], objective float64 [iters + 1], changed int64 [iters], rows (the
    dataset row of every bank entry, or None = 0 .. M-1), precision; converged_at: the first i with changed[i] == 0, or None."""

    def __init__(self, centroids, assign, score, counts, objective, changed, rows, precision):
        self.centroids, self.assign, self.score, self.counts = centroids, assign, score, counts
        self.objective, self.changed, self.rows, self.precision = objective, changed, rows, precision
        self._predict = None

    @property
    def k(self):
        return int(self.centroids.shape[0])

    @property
    def width(self):
        return int(self.centroids.shape[1])

    @property
    def converged_at(self):
        still = np.flatnonzero(self.changed.cpu().numpy() == 0)
        return int(still[0]) if still.size else None

    @classmethod
    def fit(cls, bank, k, norm=None, rows=None, iters=25, seed=0, init="rows", precision="f32"):
        """bank [M, Z] fp32; norm: its fp32 row norms [M] on the bank's device (None = computed here); rows: the dataset row of every
        entry (integers [M]; None = 0 .. M-1); iters >= 0 Lloyd iterations; init: "rows" = k distinct bank positions
        torch.randperm(M, generator = a CPU generator seeded with seed)[:k], normalised as the update normalises, or an fp32 [k, Z]
        tensor taken as given; precision: the operand type of the scores."""
        if not torch.is_tensor(bank) or bank.dim() != 2 or bank.shape[0] < 1 or bank.shape[1] < 1 or bank.dtype != torch.float32:
            raise HipError("code clusters: the bank must be an fp32 [M, Z] tensor with M, Z >= 1")
        x = bank.detach()
        if x.stride(1) != 1:
            x = x.contiguous()
        M, Z, dev = int(x.shape[0]), int(x.shape[1]), x.device
        K = _check_k("code clusters", k, M)
        if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or iters < 0:
            raise HipError("code clusters: iters must be an int >= 0, got %r" % (iters,))
        if norm is None:
            norm = torch.linalg.vector_norm(x, dim=1)
        elif not torch.is_tensor(norm) or tuple(norm.shape) != (M,) or norm.dtype != torch.float32 or norm.device != dev:
            raise HipError("code clusters: norm must be an fp32 [%d] tensor on the bank's device" % M)
        norm = norm.contiguous()
        if rows is not None:
            rows = torch.as_tensor(rows).detach().to("cpu", torch.long).reshape(-1)
            if rows.numel() != M:
                raise HipError("code clusters: rows must name %d dataset rows, got %d" % (M, rows.numel()))
        if torch.is_tensor(init):
            if tuple(init.shape) != (K, Z) or init.dtype != torch.float32:
                raise HipError("code clusters: init must be \"rows\" or an fp32 [%d, %d] tensor, got %s %s" % (K, Z, init.dtype, tuple(init.shape)))
            c = init.detach().to(dev).contiguous().clone()
        elif isinstance(init, str) and init == "rows":
            if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
                raise HipError("code clusters: seed must be an int, got %r" % (seed,))
            pick = torch.randperm(M, generator=torch.Generator().manual_seed(int(seed)))[:K].to(dev)
            v = x[pick] / norm[pick].clamp_min(EPS)[:, None]
            c = (v / torch.linalg.vector_norm(v, dim=1).clamp_min(EPS)[:, None]).contiguous()
        else:
            raise HipError("code clusters: init must be \"rows\" or an fp32 [%d, %d] tensor, got %r" % (K, Z, init))
        route = _route(Z, K, precision, dev)

        def mean(assign, best):
            live = assign >= 0
            return torch.where(live, best.double(), torch.zeros((), dtype=torch.float64, device=dev)).sum() / live.sum()

        objective, changed, prev = [], [], None
        for i in range(int(iters)):
            a, best = route.nearest(x, c, norm)
            changed.append(torch.full((), M, dtype=torch.long, device=dev) if prev is None else (a != prev).sum())
            objective.append(mean(a, best))
            c, _ = route.update(x, norm, a, c)
            prev = a
        assign, score = route.nearest(x, c, norm)
        objective.append(mean(assign, score))
        live = assign >= 0
        counts = torch.zeros(K, dtype=torch.long, device=dev).index_add_(0, assign.clamp_min(0), live.long())
        return cls(c, assign, score, counts, torch.stack(objective),
                   torch.stack(changed) if changed else torch.zeros(0, dtype=torch.long, device=dev), rows, precision)

    def predict(self, query):
        """The cluster of every query code [Q, Z] on the centroids' device - for instance the code of a partial outfit from
        encode_items(blank=...) - and its cosine to that centroid: (cluster int64 [Q], score fp32 [Q]); -1 and NaN for a query whose
        scores are all NaN."""
        if not torch.is_tensor(query) or query.dim() != 2 or query.shape[0] < 1 or query.shape[1] != self.width or query.dtype != torch.float32:
            raise HipError("predict(): query must be an fp32 [Q, %d] tensor with Q >= 1, got %s" % (
                self.width, ("%s %s" % (query.dtype, tuple(query.shape))) if torch.is_tensor(query) else type(query).__name__))
        if query.device != self.centroids.device:
            raise HipError("predict(): the query is on %s, the centroids on %s" % (query.device, self.centroids.device))
        q = query.detach()
        if q.stride(1) != 1:
            q = q.contiguous()
        if self._predict is None:
            self._predict = _route(self.width, self.k, self.precision, self.centroids.device)
        return self._predict.nearest(q, self.centroids, torch.linalg.vector_norm(q, dim=1))

    def _dataset_rows(self, pos):
        return pos if self.rows is None else self.rows.to(pos.device)[pos]

    def members(self, j):
        """the dataset rows of cluster j, ascending"""
        if isinstance(j, bool) or not isinstance(j, (int, np.integer)) or not 0 <= int(j) < self.k:
            raise HipError("members(): cluster must be an int in [0, %d), got %r" % (self.k, j))
        return torch.sort(self._dataset_rows(torch.nonzero(self.assign == int(j))[:, 0])).values

    def representatives(self):
        """per cluster the dataset row with the highest score, the lowest row of equal scores, -1 for an empty cluster: int64 [K]"""
        assign, score = self.assign.cpu(), self.score.cpu()                   # (a read-out of K numbers: whole-tensor ops on the host)
        row = self._dataset_rows(torch.arange(int(assign.shape[0])))
        live = assign >= 0
        a, s, row = assign[live], score[live], row[live]
        top = torch.full((self.k,), float("-inf")).scatter_reduce(0, a, s, "amax", include_self=True)
        first = torch.full((self.k,), torch.iinfo(torch.long).max, dtype=torch.long)
        hit = s == top[a]
        first = first.scatter_reduce(0, a[hit], row[hit], "amin", include_self=True)
        return torch.where(self.counts.cpu() > 0, first, torch.full_like(first, -1)).to(self.assign.device)


_KEYS = {"K": 64, "ITERS": 25, "SEED": 0, "LAYER": None}


def clusters_from_config(block):
    """The `HIP: CODE_CLUSTERS:` block of the embedding script's config: {K: 64, ITERS: 25, SEED: 0, LAYER: null} ->
    {"k", "iters", "seed", "layer"}; None / empty -> None (nothing is encoded, logged or written)."""
    if not block:
        return None
    if not isinstance(block, dict):
        raise HipError("CODE_CLUSTERS must be a mapping with K, ITERS, SEED and LAYER, got %r" % (block,))
    extra = sorted(set(block) - set(_KEYS), key=str)
    if extra:
        raise HipError("CODE_CLUSTERS: unknown key(s) %s (known: %s)" % (", ".join(map(str, extra)), ", ".join(sorted(_KEYS))))
    k = block.get("K", _KEYS["K"])
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_K:
        raise HipError("CODE_CLUSTERS: K must be an int in [1, %d], got %r" % (MAX_K, k))
    iters = block.get("ITERS", _KEYS["ITERS"])
    if isinstance(iters, bool) or not isinstance(iters, int) or iters < 0:
        raise HipError("CODE_CLUSTERS: ITERS must be an int >= 0, got %r" % (iters,))
    seed = block.get("SEED", _KEYS["SEED"])
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise HipError("CODE_CLUSTERS: SEED must be an int, got %r" % (seed,))
    layer = block.get("LAYER", None)
    if layer is not None and (isinstance(layer, bool) or not isinstance(layer, int) or layer < 1):
        raise HipError("CODE_CLUSTERS: LAYER must be null or an int >= 1, got %r" % (layer,))
    return {"k": int(k), "iters": int(iters), "seed": int(seed), "layer": layer}
