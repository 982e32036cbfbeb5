"""The state digest of include/codae_hip.h ("State digest") restated twice for the tests: word by word in plain Python integers
(digest_ints, the independent reference) and in numpy (digest_numpy), and the vectors the definition was published with."""
import numpy as np

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15


def mix(x):
    z = (x + G) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def digest_ints(words):
    """words: a sequence of uint32 values -> (out0, out1)."""
    w = [int(v) for v in words]
    n_bytes = 4 * len(w)
    w += [0] * (-len(w) % 4)
    s = x = 0
    for g in range(len(w) // 4):
        a = w[4 * g] | (w[4 * g + 1] << 32)
        b = w[4 * g + 2] | (w[4 * g + 3] << 32)
        h = mix(a ^ mix((b + g * G) & M64))
        s = (s + h) & M64
        x ^= mix(h ^ g)
    return s ^ mix(n_bytes), x


def digest_numpy(array):
    """Any numpy array whose byte count is a multiple of 4 -> (out0, out1), vectorised."""
    w = np.ascontiguousarray(array).view(np.uint8).reshape(-1).view("<u4")
    n_bytes = 4 * int(w.size)
    w = np.concatenate([w, np.zeros(-w.size % 4, dtype="<u4")]).astype(np.uint64).reshape(-1, 4)
    u = np.uint64

    def vmix(v):
        z = v + u(G)
        z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
        return z ^ (z >> u(31))
    with np.errstate(over="ignore"):
        g = np.arange(w.shape[0], dtype=np.uint64)
        h = vmix((w[:, 0] | (w[:, 1] << u(32))) ^ vmix((w[:, 2] | (w[:, 3] << u(32))) + g * u(G)))
        s = int(h.sum(dtype=np.uint64)) if h.size else 0
        x = int(np.bitwise_xor.reduce(vmix(h ^ g))) if h.size else 0
    return s ^ mix(n_bytes), x


# (input as an array, out0, out1): the published vectors
VECTORS = [
    ("empty", np.zeros(0, dtype=np.uint32), 0xe220a8397b1dcdaf, 0x0000000000000000),
    ("words [0]", np.zeros(1, dtype=np.uint32), 0xc9753e5daf2af4a5, 0x238275bc38fcbe91),
    ("words [0,0,0,0]", np.zeros(4, dtype=np.uint32), 0xfae75bf3f76eec68, 0x238275bc38fcbe91),
    ("words [1..9]", np.arange(1, 10, dtype=np.uint32), 0xbd5ecaa3dafb33c9, 0x7e9b14bc1252b0cd),
    ("fp32 arange(8)", np.arange(8, dtype=np.float32), 0xfdc10e5f6cf943b8, 0xf9f958a45f46a835),
]
