"""Input noise of the denoising autoencoder: additive Gaussian, element masking and salt-and-pepper noise
(Vincent et al. 2010), the counterpart of the CODAE_NOISE_* kinds of include/codae_hip.h.

The noise of one element is a pure function of (seed, dataset row, column, optimizer step): Philox4x32-10 with
key = (seed & 0xffffffff, seed >> 32) and counter = (column // 4, dataset row, step, 0); the four output words belong to
columns 4g .. 4g + 3.  So a row is noised the same wherever it lands in a batch and on whichever data-parallel rank, a
run is reproducible, and a row that appears twice in one batch gets the same noise twice (the epoch sampler draws without
replacement).  Noise comes first, the Corrupter's whole-slot mask second: a blanked element is exactly 0.

InputNoise carries the parameters (as fp32, the type of the C struct), hands them to the HIP engine
(DaeEngine.set_input_noise, HipEmbeddingTrainer(input_noise=...)) and noises a dense batch for the drop-in scripts
(apply): on the GPU through codae_corrupt_batch, on host tensors through the numpy statement of the same definition
below - the same bits for masking and salt-and-pepper, fp64 arithmetic for the Gaussian kind.

Swap noise (kind "swap", CODAE_NOISE_SWAP) is the corruption of denoising autoencoders on categorical and entity data: with
probability p a whole slot of the input is replaced by the same slot of another dataset row, and the network is asked for the
clean row.  One draw per (dataset row, slot, step): counter = (slot, dataset row, step, 512), hit iff word 0 < T, source row
pool[(word 1 * P) >> 32]; a draw is accepted unless the source is the row itself or, with a presence table, either side lacks
the slot; a rejected draw leaves the slot as it is (no redraw).  The pool (default: every row) is what a training script sets to
its training rows, so that no validation item reaches a training input.  No arithmetic touches the values: both sides of apply
give the same bits.
"""
import math

import numpy as np

from ..hip import NOISE_GAUSSIAN, NOISE_MASKING, NOISE_SALT_PEPPER, NOISE_SWAP, HipError

KINDS = {"gaussian": NOISE_GAUSSIAN, "masking": NOISE_MASKING, "salt_pepper": NOISE_SALT_PEPPER, "swap": NOISE_SWAP}
SWAP_STREAM = 512      # counter word 3 of the swap draws (element noises 0, dropout 1 + layer, slot contrast 256)

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)
_SH = np.uint64(32)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al. 2011).  counter: four uint32 arrays (broadcast together), key: two ints.
    Returns the four output words as uint32 arrays."""
    c = [np.asarray(w, dtype=np.uint64) & _LOW for w in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]           # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> _SH) ^ c[1] ^ np.uint64(k0), p1 & _LOW, (p0 >> _SH) ^ c[3] ^ np.uint64(k1), p0 & _LOW]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return [w.astype(np.uint32) for w in c]


def noise_words(rows, io, step, seed):
    """uint32 [B, io]: the word of every element of dataset rows `rows` at optimizer step `step`."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 1)
    groups = np.arange((io + 3) // 4, dtype=np.int64).reshape(1, -1)
    r = philox4x32_10((groups, rows & 0xFFFFFFFF, np.int64(step) & 0xFFFFFFFF, 0), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(r, axis=-1).reshape(rows.shape[0], -1)[:, :io]


def unit_normals(rows, io, step, seed):
    """float64 [B, io]: Box-Muller over the word pairs (r0, r1), (r2, r3) of every group.  An odd io leaves the last pair
    half used: its second word comes out of the generator all the same."""
    w = noise_words(rows, io + (io & 1), step, seed)
    u1 = ((w[:, 0::2] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (w[:, 1::2] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    rho = np.sqrt(-2.0 * np.log(u1))
    n = np.empty(w.shape, dtype=np.float64)
    n[:, 0::2] = rho * np.cos(2.0 * np.pi * u2)
    n[:, 1::2] = rho * np.sin(2.0 * np.pi * u2)
    return n[:, :io]


def swap_words(rows, n_slots, step, seed):
    """(w0, w1) uint32 [B, S]: the hit word and the source word of every (dataset row, slot) at optimizer step `step`."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 1)
    slots = np.arange(int(n_slots), dtype=np.int64).reshape(1, -1)
    r = philox4x32_10((slots, rows & 0xFFFFFFFF, np.int64(step) & 0xFFFFFFFF, SWAP_STREAM), (seed & 0xFFFFFFFF, seed >> 32))
    return r[0], r[1]


def _presence_table(presence):
    """uint8 [n_rows, S] or None, from a SlotPresence, an array or a tensor."""
    if presence is None:
        return None
    t = getattr(presence, "table", presence)
    if t is None:
        return None
    if hasattr(t, "detach"):
        t = t.detach().cpu().numpy()
    return np.asarray(t) != 0


def _finite(name, v):
    if v is None:
        raise HipError("input noise: %s is missing" % name)
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise HipError("input noise: %s must be a number, got %r" % (name, v))
    v = float(np.float32(v)) if abs(float(v)) < 3.4e38 else float(v)
    if not math.isfinite(v):
        raise HipError("input noise: %s = %r is not finite" % (name, v))
    return v


class InputNoise:
    """InputNoise("gaussian", sigma=0.1) | InputNoise("masking", p=0.25) | InputNoise("salt_pepper", p=0.1, lo=0.0, hi=1.0) |
    InputNoise("swap", p=0.15, pool=None); seed: 64-bit stream id.  Parameters are kept as the fp32 values the C struct carries.
    pool (swap only): the dataset rows items may be taken from - an integer tensor, array or list, not empty; None = every row."""

    def __init__(self, kind, sigma=None, p=None, lo=None, hi=None, seed=0, pool=None):
        name = kind.lower() if isinstance(kind, str) else kind
        if name not in KINDS:
            raise HipError("input noise: unknown kind %r (use one of %s)" % (kind, ", ".join(sorted(KINDS))))
        self.kind = name
        self.code = KINDS[name]
        given = {"sigma": sigma, "p": p, "lo": lo, "hi": hi}
        wanted = {"gaussian": ("sigma",), "masking": ("p",), "salt_pepper": ("p", "lo", "hi"), "swap": ("p",)}[name]
        for k, v in given.items():
            if k not in wanted and v is not None:
                raise HipError("input noise: %s noise takes no %s" % (name, k))
        vals = {k: _finite(k, given[k]) for k in wanted}
        if name == "gaussian" and vals["sigma"] < 0:
            raise HipError("input noise: sigma = %r must be >= 0" % vals["sigma"])
        if name != "gaussian" and not 0.0 <= vals["p"] <= 1.0:
            raise HipError("input noise: p = %r outside [0, 1]" % vals["p"])
        self.sigma, self.p, self.lo, self.hi = (vals.get(k) for k in ("sigma", "p", "lo", "hi"))
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
            raise HipError("input noise: seed must be an integer in [0, 2^64), got %r" % (seed,))
        self.seed = int(seed)
        self.pool = None
        if pool is not None:
            if name != "swap":
                raise HipError("input noise: %s noise takes no pool" % name)
            if hasattr(pool, "detach"):
                pool = pool.detach().cpu().numpy()
            rows = np.asarray(pool)
            if rows.size == 0:
                raise HipError("input noise: pool is empty")
            if rows.dtype == np.bool_ or not np.issubdtype(rows.dtype, np.integer):
                raise HipError("input noise: pool must hold integer dataset rows, got dtype %s" % rows.dtype)
            rows = rows.reshape(-1).astype(np.int64)
            if rows.size == 0:
                raise HipError("input noise: pool is empty")
            if rows.size >= 2 ** 31 or rows.min() < 0 or rows.max() >= 2 ** 31:
                raise HipError("input noise: pool rows must lie in [0, 2^31), fewer than 2^31 of them")
            self.pool = np.ascontiguousarray(rows)

    def pool_rows(self, n_rows):
        """The pool as int64 rows checked against a dataset of n_rows rows, or None = every row."""
        if n_rows is None or isinstance(n_rows, bool) or int(n_rows) < 1 or int(n_rows) >= 2 ** 31:
            raise HipError("input noise: swap needs the dataset's row count in [1, 2^31), got %r" % (n_rows,))
        if self.pool is not None and int(self.pool.max()) >= int(n_rows):
            raise HipError("input noise: pool row %d outside the dataset's %d rows" % (int(self.pool.max()), int(n_rows)))
        return self.pool

    def swapped(self, rows, step, n_slots, n_rows=None, presence=None):
        """(accepted bool [B, S], source int64 [B, S]) on the host: which slots of dataset rows `rows` take another row's item at
        optimizer step `step`, and whose.  n_rows: the dataset's row count (required without a pool; checks the pool otherwise);
        presence: a SlotPresence or a [n_rows, S] table.  source is the drawn row for every slot, accepted or not."""
        if self.kind != "swap":
            raise HipError("InputNoise.swapped: %s noise swaps nothing" % self.kind)
        if isinstance(n_slots, bool) or not isinstance(n_slots, (int, np.integer)) or int(n_slots) < 1:
            raise HipError("InputNoise.swapped: n_slots must be a positive integer, got %r" % (n_slots,))
        if n_rows is None and self.pool is None:
            raise HipError("InputNoise.swapped: n_rows is required without a pool")
        pool = self.pool if n_rows is None else self.pool_rows(n_rows)
        rows = np.asarray(rows.detach().cpu().numpy() if hasattr(rows, "detach") else rows, dtype=np.int64).reshape(-1)
        w0, w1 = swap_words(rows, n_slots, step, self.seed)
        P = int(n_rows) if pool is None else int(pool.size)
        j = ((w1.astype(np.uint64) * np.uint64(P)) >> _SH).astype(np.int64)
        source = j if pool is None else pool[j]
        accepted = (w0.astype(np.uint64) < np.uint64(self.threshold)) & (source != rows.reshape(-1, 1))
        pres = _presence_table(presence)
        if pres is not None:
            if pres.ndim != 2 or pres.shape[1] != int(n_slots):
                raise HipError("InputNoise.swapped: presence shape %s, %d slots" % (tuple(pres.shape), int(n_slots)))
            slot = np.arange(int(n_slots)).reshape(1, -1)
            accepted &= pres[rows.reshape(-1, 1), slot] & pres[source, slot]
        return accepted, source

    def __repr__(self):
        args = ["%s=%r" % (k, getattr(self, k)) for k in ("sigma", "p", "lo", "hi") if getattr(self, k) is not None]
        if self.pool is not None:
            args.append("pool=<%d rows>" % self.pool.size)
        return "InputNoise(%r, %s, seed=%d)" % (self.kind, ", ".join(args), self.seed)

    @property
    def threshold(self):
        """T = floor(p 2^32): an element is hit iff its word is below T."""
        return int(math.floor(self.p * 4294967296.0))

    def as_struct(self):
        from ..hip import Noise
        p0 = self.sigma if self.kind == "gaussian" else self.p
        return Noise(self.code, p0, self.lo or 0.0, self.hi or 0.0, self.seed)

    # ---- a dense batch (drop-in scripts) ----------------------------------------------------------
    def apply(self, x, rows, step, mask=None, data=None, presence=None, n_slots=None):
        """Noised (then masked) copy of the dense fp32 batch x [B, io].  rows: the dataset index of every batch row (what
        the scripts hold as batch_indices); step: the 1-based optimizer step; mask [B, io]: 0 = blanked (the fmask of
        Corrupter.get_masks), applied after the noise.  A HIP tensor is noised by the library's kernel, a host tensor here.
        Swap noise needs data [n_rows, io] (the dataset the swapped slots are read from, on x's device) and n_slots; presence (a
        SlotPresence or a [n_rows, S] table, optional) keeps absent slots out of the swaps and zeroes them, as the step does."""
        import torch
        if not isinstance(x, torch.Tensor) or x.dim() != 2:
            raise HipError("InputNoise.apply: x must be a [B, io] tensor")
        B, io = x.shape
        rows_t = torch.as_tensor(rows).reshape(-1)
        if rows_t.numel() != B:
            raise HipError("InputNoise.apply: %d rows for a batch of %d" % (rows_t.numel(), B))
        if mask is not None and tuple(mask.shape) != (B, io):
            raise HipError("InputNoise.apply: mask shape %s, batch shape %s" % (tuple(mask.shape), (B, io)))
        if isinstance(step, bool) or not isinstance(step, (int, np.integer)) or not 0 <= int(step) < 2 ** 31:
            raise HipError("InputNoise.apply: step must be an integer in [0, 2^31), got %r" % (step,))
        if self.kind == "swap":
            if data is None or n_slots is None:
                raise HipError("InputNoise.apply: swap noise needs data (the dataset [n_rows, io]) and n_slots")
            if not isinstance(data, torch.Tensor) or data.dim() != 2 or data.shape[1] != io or data.device != x.device:
                raise HipError("InputNoise.apply: data must be a [n_rows, %d] tensor on %s" % (io, x.device))
            if isinstance(n_slots, bool) or not isinstance(n_slots, (int, np.integer)) or int(n_slots) < 1 or io % int(n_slots) != 0:
                raise HipError("InputNoise.apply: n_slots %r does not divide io %d" % (n_slots, io))
            self.pool_rows(int(data.shape[0]))
            pres = _presence_table(presence)
            if pres is not None and tuple(pres.shape) != (int(data.shape[0]), int(n_slots)):
                raise HipError("InputNoise.apply: presence shape %s, expected %s" % (tuple(pres.shape), (int(data.shape[0]), int(n_slots))))
        elif data is not None or presence is not None or n_slots is not None:
            raise HipError("InputNoise.apply: data / presence / n_slots go with swap noise only")
        if x.device.type == "cuda":
            if self.kind == "swap":
                return self._apply_swap_hip(x, rows_t, int(step), mask, data, pres, int(n_slots))
            return self._apply_hip(x, rows_t, int(step), mask)
        xs = x.detach().to(torch.float32).numpy()
        mk = None if mask is None else mask.detach().cpu().numpy()
        if self.kind == "swap":
            out = self.apply_numpy(xs, rows_t.cpu().numpy(), int(step), mk, data.detach().to(torch.float32).numpy(), pres, int(n_slots))
        else:
            out = self.apply_numpy(xs, rows_t.cpu().numpy(), int(step), mk)
        return torch.from_numpy(out)

    def apply_numpy(self, x, rows, step, mask=None, data=None, presence=None, n_slots=None):
        x = np.asarray(x, dtype=np.float32)
        if self.kind == "swap":
            # out[b, s-th slot] = data[source] where the draw was accepted, else x; then the blank, then the presence rule
            data = np.asarray(data, dtype=np.float32)
            S, E = int(n_slots), x.shape[1] // int(n_slots)
            rows = np.asarray(rows, dtype=np.int64).reshape(-1)
            pres = _presence_table(presence)
            accepted, source = self.swapped(rows, step, S, n_rows=data.shape[0], presence=pres)
            from_row = np.where(accepted, source, 0)
            taken = data.reshape(data.shape[0], S, E)[from_row, np.arange(S).reshape(1, -1)]      # [B, S, E]
            out = np.where(accepted[:, :, None], taken, x.reshape(-1, S, E)).reshape(x.shape)
            if mask is not None:
                out = np.where(np.asarray(mask) != 0, out, np.float32(0))
            if pres is not None:
                out = np.where(np.repeat(pres[rows], E, axis=1), out, np.float32(0))
            return np.ascontiguousarray(out, dtype=np.float32)
        if self.kind == "gaussian":
            out = (x.astype(np.float64) + np.float64(self.sigma) * unit_normals(rows, x.shape[1], step, self.seed)).astype(np.float32)
        else:
            w = noise_words(rows, x.shape[1], step, self.seed)
            hit = w.astype(np.uint64) < np.uint64(self.threshold)
            if self.kind == "masking":
                out = np.where(hit, np.float32(0), x)
            else:
                salt = w.astype(np.uint64) < np.uint64(self.threshold // 2)
                out = np.where(hit, np.where(salt, np.float32(self.lo), np.float32(self.hi)), x)
        if mask is not None:
            out = np.where(np.asarray(mask) != 0, out, np.float32(0))
        return np.ascontiguousarray(out, dtype=np.float32)

    def _apply_hip(self, x, rows, step, mask):
        import ctypes as C
        import torch
        from ..hip import Batch, check, current_stream, lib, ptr
        x = x.detach().to(torch.float32).contiguous()
        B, io = x.shape
        rows = rows.to(device=x.device, dtype=torch.int32).contiguous()
        table = mask_id = None
        if mask is not None:
            table = (mask.to(x.device) != 0).to(torch.uint8).contiguous()      # one table row per batch row
            mask_id = torch.arange(B, dtype=torch.int32, device=x.device)
        out = torch.empty_like(x)
        batch = Batch(ptr(x), None, ptr(mask_id), ptr(table), B, io, None, 0, 0)
        noise = self.as_struct()
        with torch.cuda.device(x.device):
            check(lib().codae_corrupt_batch(C.byref(batch), C.byref(noise), step, ptr(rows), ptr(out), 0, io, current_stream()))
        # (rows / table / mask_id were allocated on the current stream: the caching allocator reuses them in stream order)
        return out


    def _apply_swap_hip(self, x, rows, step, mask, data, pres, n_slots):
        import ctypes as C
        import torch
        from ..hip import Batch, Swap, check, current_stream, lib, ptr
        x = x.detach().to(torch.float32).contiguous()
        data = data.detach().to(torch.float32).contiguous()
        B, io = x.shape
        with torch.cuda.device(x.device):
            rows = rows.to(device=x.device, dtype=torch.int32).contiguous()
            table = mask_id = None
            if mask is not None:
                table = (mask.to(x.device) != 0).to(torch.uint8).contiguous()      # one table row per batch row
                mask_id = torch.arange(B, dtype=torch.int32, device=x.device)
            pool = None if self.pool is None else torch.from_numpy(self.pool.astype(np.int32)).to(x.device)
            present = None if pres is None else torch.from_numpy(np.ascontiguousarray(pres).astype(np.uint8)).to(x.device)
            out = torch.empty_like(x)
            batch = Batch(ptr(x), None, ptr(mask_id), ptr(table), B, io, None, 0, 0)
            noise = self.as_struct()
            swap = Swap(ptr(pool), int(data.shape[0]) if pool is None else int(pool.numel()), n_slots)
            check(lib().codae_corrupt_batch_swap(C.byref(batch), C.byref(noise), step, ptr(rows), ptr(data), C.byref(swap), ptr(out), 0, io,
                                                 ptr(present), 0, current_stream()))
        return out


def input_noise_from_config(block, data=None, train_rows=None):
    """The `HIP: INPUT_NOISE:` block of the embedding script's config: {KIND: gaussian | masking | salt_pepper | swap, SIGMA | P: ...,
    LO: ..., HI: ..., SEED: ..., POOL: train | all}.  None / empty -> None.  LO / HI default to the min / max of `data` (the resident
    matrix).  POOL (swap only; default train): the rows swapped items come from - train_rows, the script's training indices, or all."""
    if not block:
        return None
    if not isinstance(block, dict):
        raise HipError("INPUT_NOISE must be a mapping with a KIND, got %r" % (block,))
    known = {"KIND", "SIGMA", "P", "LO", "HI", "SEED", "POOL"}
    extra = sorted(set(block) - known)
    if extra:
        raise HipError("INPUT_NOISE: unknown key(s) %s (known: %s)" % (", ".join(map(str, extra)), ", ".join(sorted(known))))
    if "KIND" not in block:
        raise HipError("INPUT_NOISE: KIND is missing")
    kind = str(block["KIND"]).lower()
    lo, hi = block.get("LO"), block.get("HI")
    if kind == "salt_pepper" and data is not None:
        lo = float(data.min()) if lo is None else lo
        hi = float(data.max()) if hi is None else hi
    pool = None
    if "POOL" in block and kind != "swap":
        raise HipError("INPUT_NOISE: POOL goes with KIND: swap only")
    if kind == "swap":
        which = str(block.get("POOL", "train")).lower()
        if which not in ("train", "all"):
            raise HipError("INPUT_NOISE: unknown POOL %r (use train or all)" % (block.get("POOL"),))
        if which == "train":
            if train_rows is None:
                raise HipError("INPUT_NOISE: POOL: train needs the training rows")
            pool = train_rows
    return InputNoise(kind, sigma=block.get("SIGMA"), p=block.get("P"), lo=lo, hi=hi, seed=block.get("SEED", 0), pool=pool)
