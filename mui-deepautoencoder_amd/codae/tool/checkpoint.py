"""Checkpoint files of the fused trainer, and the host restatement of the device's state digest.

StateDigest.get is include/codae_hip.h, "State digest", in numpy: what codae_state_digest computes on the device, for host-side
tools and the tests.  It is a fingerprint against accidents (a truncated file, a flipped bit, a replica that drifted), not a
cryptographic hash.

The file is ONE uncompressed .npz: one array per state tensor (HipEmbeddingTrainer / DaeEngine.state_tensors: params, adam_m, adam_v,
adam_vmax and weight_avg when kept, scalars) plus `meta`, a JSON string.  It is written to a temporary name in the target's directory
and moved into place with os.replace, so a reader never sees half a file, and read with allow_pickle=False.  The bf16 shadows are
derived from the parameters and are not stored.
"""
import json
import os
import tempfile
import zipfile

import numpy as np

FORMAT_VERSION = 1
_M64 = (1 << 64) - 1


class CheckpointError(ValueError):
    """A file that cannot be a checkpoint of this format: the message names the piece (the tensor, or `meta`)."""


class StateDigest:
    """(out[0], out[1]) of include/codae_hip.h, "State digest", as Python ints."""
    G = 0x9E3779B97F4A7C15

    @staticmethod
    def _mix(x):
        """numpy uint64 array -> mix(x), mod 2^64 (the wrap-around is what unsigned numpy arithmetic does)."""
        z = x + np.uint64(StateDigest.G)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))

    @staticmethod
    def mix_int(x):
        z = (x + StateDigest.G) & _M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        return z ^ (z >> 31)

    @staticmethod
    def words(data):
        """bytes / bytearray / memoryview / numpy array -> its bytes as little-endian uint32 words (length a multiple of 4)."""
        if isinstance(data, np.ndarray):
            raw = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        else:
            raw = np.frombuffer(bytes(data), dtype=np.uint8)
        if raw.size % 4:
            raise ValueError("state digest: %d bytes is not a multiple of 4" % raw.size)
        return raw.view("<u4")

    @staticmethod
    def get(data):
        w = StateDigest.words(data)
        n_bytes = 4 * int(w.size)
        if w.size % 4:
            w = np.concatenate([w, np.zeros(4 - w.size % 4, dtype="<u4")])
        w = w.astype(np.uint64).reshape(-1, 4)
        with np.errstate(over="ignore"):
            g = np.arange(w.shape[0], dtype=np.uint64)
            a = w[:, 0] | (w[:, 1] << np.uint64(32))
            b = w[:, 2] | (w[:, 3] << np.uint64(32))
            h = StateDigest._mix(a ^ StateDigest._mix(b + g * np.uint64(StateDigest.G)))
            s = int(np.add.reduce(h, dtype=np.uint64)) if h.size else 0
            x = int(np.bitwise_xor.reduce(StateDigest._mix(h ^ g))) if h.size else 0
        return (s & _M64) ^ StateDigest.mix_int(n_bytes), x

    @staticmethod
    def combine(digests):
        """The digest of the concatenated little-endian digests (an iterable of (d0, d1)): one fingerprint for a whole state."""
        flat = np.asarray([v for d in digests for v in d], dtype="<u8")
        return StateDigest.get(flat)

    @staticmethod
    def hex(d):
        return "%016x%016x" % (int(d[0]), int(d[1]))

    @staticmethod
    def from_hex(s):
        if len(s) != 32:
            raise ValueError("state digest: %r is not 32 hex digits" % (s,))
        return int(s[:16], 16), int(s[16:], 16)


def write_checkpoint(path, tensors, meta):
    """tensors: ordered {name: numpy array}; meta: a JSON-serialisable dict (the caller's keys; `format`, `tensors` and `digests` are
    set here when absent).  -> the number of bytes written."""
    meta = dict(meta)
    meta.setdefault("format", FORMAT_VERSION)
    meta["tensors"] = list(tensors)
    meta.setdefault("digests", {k: StateDigest.hex(StateDigest.get(v)) for k, v in tensors.items()})
    if "meta" in tensors:
        raise ValueError("checkpoint: a state tensor cannot be called 'meta'")
    d = os.path.dirname(os.path.abspath(path))
    fd, tmp = tempfile.mkstemp(prefix=os.path.basename(path) + ".", suffix=".tmp", dir=d)
    try:
        with os.fdopen(fd, "wb") as f:
            np.savez(f, meta=np.asarray(json.dumps(meta)), **{k: np.ascontiguousarray(v) for k, v in tensors.items()})
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.unlink(tmp)
        raise
    return os.path.getsize(path)


def _first_cut_member(path):
    """Which member of a zip whose directory is gone (a truncated file) runs past the file's end: walks the local headers, which
    np.savez writes with the sizes patched in (zip64 extra field).  None when no member does, or the file is no zip at all."""
    import struct
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        pos = 0
        while pos + 30 <= size:
            f.seek(pos)
            head = f.read(30)
            if head[:4] != b"PK\x03\x04":
                return None
            csize, _usize, nlen, elen = struct.unpack("<IIHH", head[18:30])
            name = f.read(nlen).decode("utf-8", "replace")
            extra = f.read(elen)
            name = name[:-4] if name.endswith(".npy") else name
            if len(extra) < elen:
                return name
            o = 0
            while csize == 0xFFFFFFFF and o + 4 <= len(extra):
                tag, n = struct.unpack("<HH", extra[o:o + 4])
                if tag == 1 and n >= 16:
                    csize = struct.unpack("<Q", extra[o + 12:o + 20])[0]
                o += 4 + n
            pos += 30 + nlen + elen + csize
            if pos > size:
                return name
    return None


def read_checkpoint(path, verify=True):
    """-> (ordered {name: numpy array}, meta dict).  CheckpointError naming the piece for a file that is truncated, not an .npz, lacks
    `meta` or a tensor `meta` lists, or (verify) holds a tensor whose bytes do not have the digest `meta` records - the host-side
    check; HipEmbeddingTrainer.load checks again on the device, after the upload."""
    try:
        z = np.load(path, allow_pickle=False)
    except (OSError, ValueError, zipfile.BadZipFile, EOFError) as e:
        cut = _first_cut_member(path)
        if cut is not None:
            raise CheckpointError("checkpoint %s: truncated inside '%s' (%s)" % (path, cut, e))
        raise CheckpointError("checkpoint %s: not a readable .npz (%s)" % (path, e))
    with z:
        def member(name):
            try:
                return z[name]
            except KeyError:
                raise CheckpointError("checkpoint %s: '%s' is missing" % (path, name))
            except (OSError, ValueError, zipfile.BadZipFile, EOFError, zipfile.zlib.error) as e:
                raise CheckpointError("checkpoint %s: '%s' cannot be read (%s)" % (path, name, e))
        try:
            meta = json.loads(str(member("meta")[()]))
        except (ValueError, IndexError) as e:
            raise CheckpointError("checkpoint %s: 'meta' does not parse (%s)" % (path, e))
        if not isinstance(meta, dict) or meta.get("format") != FORMAT_VERSION:
            raise CheckpointError("checkpoint %s: 'meta' has format %r, this reader knows %d"
                                  % (path, meta.get("format") if isinstance(meta, dict) else None, FORMAT_VERSION))
        tensors = {}
        for name in meta.get("tensors", []):
            t = member(name)
            want = meta.get("digests", {}).get(name)
            if verify:
                if want is None:
                    raise CheckpointError("checkpoint %s: 'meta' records no digest for '%s'" % (path, name))
                got = StateDigest.hex(StateDigest.get(t))
                if got != want:
                    raise CheckpointError("checkpoint %s: tensor '%s' has digest %s, 'meta' recorded %s" % (path, name, got, want))
            tensors[name] = t
    return tensors, meta
