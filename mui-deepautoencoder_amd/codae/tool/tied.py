"""Tied encoder / decoder weights (include/codae_hip.h, "Tied weights"): which layers pair up, and the two steps that keep a
materialised tie - the fold of the decoder gradients into the encoder's and the mirror of the encoder matrices into the
decoder's - in plain torch ops on host or device tensors.  The fused step runs both as HIP kernels (csrc/tied.hip); these twins
are for loops that drive the engine phase by phase, for checkpoints, and for the tests."""
import torch

from ..hip import HipError


class TiedWeights:
    """The decoder's Linear L-1-l uses the transpose of the encoder's Linear l, for every l < L/2; the middle layer of an odd
    stack and every bias stay free."""

    @staticmethod
    def pairs(schedule):
        """[(l, L-1-l)] for l < L/2.  schedule: (in_features, out_features, ...) per Linear.  Raises HipError, in the library's
        words, naming the first pair that is not a mirror image."""
        L = len(schedule)
        out = []
        for l in range(L // 2):
            m = L - 1 - l
            (ki, ni), (km, nm) = schedule[l][:2], schedule[m][:2]
            if int(ki) != int(nm) or int(ni) != int(km):
                raise HipError("tied weights: layers %d and %d are not mirror images (%d -> %d against %d -> %d)"
                               % (l, m, ki, ni, km, nm))
            out.append((l, m))
        return out

    @staticmethod
    def flat_pairs(schedule, w_off):
        """[(enc_off, dec_off, rows, cols)] of pairs(schedule) in a flat vector whose layer l matrix [out][in] starts at w_off[l]
        (DaeEngine.w_off: the layout has one source, codae_param_offsets)."""
        return [(int(w_off[l]), int(w_off[m]), int(schedule[l][1]), int(schedule[l][0])) for l, m in TiedWeights.pairs(schedule)]

    @staticmethod
    def free_parameter_count(schedule):
        """Weights and biases an optimizer of the tied stack owns."""
        L = len(schedule)
        return sum(int(k) * int(n) for (k, n, *_) in schedule[:(L + 1) // 2]) + sum(int(s[1]) for s in schedule)

    @staticmethod
    def sharded_refusal(n_layers):
        """The refusal of the sharded update, in the library's words (codae_step_update_span)."""
        return HipError("tied weights: the sharded update is not supported: the tied layers %d and %d lie in different shards"
                        % (0, n_layers - 1))

    @staticmethod
    def fold(grads_flat, schedule, w_off):
        """A copy of the flat gradient vector with g[W_l] + g[W_l']^T in every encoder range (fp32: one add, that operand
        order) and +0 in every decoder range: the gradient of the tied parameter set."""
        g = grads_flat.clone()
        for e, d, r, c in TiedWeights.flat_pairs(schedule, w_off):
            enc, dec = g[e:e + r * c].view(r, c), g[d:d + r * c].view(c, r)
            enc.copy_(enc + dec.t())
            dec.zero_()
        return g

    @staticmethod
    def mirror(params_flat, schedule, w_off):
        """A copy of the flat parameter vector with W_l^T in every decoder range (the encoder is the truth)."""
        p = params_flat.clone()
        for e, d, r, c in TiedWeights.flat_pairs(schedule, w_off):
            p[d:d + r * c].view(c, r).copy_(p[e:e + r * c].view(r, c).t())
        return p

    @staticmethod
    def from_config(value):
        """HIP: TIED_WEIGHTS of a training config: true / false (absent = false)."""
        if value is None:
            return False
        if isinstance(value, bool):
            return value
        raise HipError("HIP: TIED_WEIGHTS must be true or false, got %r" % (value,))
