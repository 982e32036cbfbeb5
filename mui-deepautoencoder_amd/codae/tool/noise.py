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
"""
import math

import numpy as np

from ..hip import NOISE_GAUSSIAN, NOISE_MASKING, NOISE_SALT_PEPPER, HipError

KINDS = {"gaussian": NOISE_GAUSSIAN, "masking": NOISE_MASKING, "salt_pepper": NOISE_SALT_PEPPER}

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
    """InputNoise("gaussian", sigma=0.1) | InputNoise("masking", p=0.25) | InputNoise("salt_pepper", p=0.1, lo=0.0, hi=1.0);
    seed: 64-bit stream id.  Parameters are kept as the fp32 values the C struct carries."""

    def __init__(self, kind, sigma=None, p=None, lo=None, hi=None, seed=0):
        name = kind.lower() if isinstance(kind, str) else kind
        if name not in KINDS:
            raise HipError("input noise: unknown kind %r (use one of %s)" % (kind, ", ".join(sorted(KINDS))))
        self.kind = name
        self.code = KINDS[name]
        given = {"sigma": sigma, "p": p, "lo": lo, "hi": hi}
        wanted = {"gaussian": ("sigma",), "masking": ("p",), "salt_pepper": ("p", "lo", "hi")}[name]
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

    def __repr__(self):
        args = ["%s=%r" % (k, getattr(self, k)) for k in ("sigma", "p", "lo", "hi") if getattr(self, k) is not None]
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
    def apply(self, x, rows, step, mask=None):
        """Noised (then masked) copy of the dense fp32 batch x [B, io].  rows: the dataset index of every batch row (what
        the scripts hold as batch_indices); step: the 1-based optimizer step; mask [B, io]: 0 = blanked (the fmask of
        Corrupter.get_masks), applied after the noise.  A HIP tensor is noised by the library's kernel, a host tensor here."""
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
        if x.device.type == "cuda":
            return self._apply_hip(x, rows_t, int(step), mask)
        xs = x.detach().to(torch.float32).numpy()
        out = self.apply_numpy(xs, rows_t.cpu().numpy(), int(step), None if mask is None else mask.detach().cpu().numpy())
        return torch.from_numpy(out)

    def apply_numpy(self, x, rows, step, mask=None):
        x = np.asarray(x, dtype=np.float32)
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


def input_noise_from_config(block, data=None):
    """The `HIP: INPUT_NOISE:` block of the embedding script's config: {KIND: gaussian | masking | salt_pepper, SIGMA | P: ...,
    LO: ..., HI: ..., SEED: ...}.  None / empty -> None.  LO / HI default to the min / max of `data` (the resident matrix)."""
    if not block:
        return None
    if not isinstance(block, dict):
        raise HipError("INPUT_NOISE must be a mapping with a KIND, got %r" % (block,))
    known = {"KIND", "SIGMA", "P", "LO", "HI", "SEED"}
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
    return InputNoise(kind, sigma=block.get("SIGMA"), p=block.get("P"), lo=lo, hi=hi, seed=block.get("SEED", 0))
