"""Sparse code: a hard top-k code layer - the counterpart of "Sparse code" in include/codae_hip.h (the k-sparse autoencoder of
Makhzani & Frey 2013, the "TopK" form of sparse-autoencoder work).

SparseCode(keep, layer=None) sparsifies h_layer.  `layer` follows encode(layer=)'s convention: it is the index of the Linear that
READS the code; the default is trainer.code_layers.  The producing Linear is m = layer - 1, 1 <= layer <= L - 1, and Z = out[m].

Sparsifying is the last thing layer m does, after activation and dropout factor.  For each batch row:

    key(v)  the bit pattern of the STORED value v with the sign bit cleared, read as an unsigned integer.  The stored value is a
            bf16 number in the bf16 engine and fp32 in the fp32 engine; widening bf16 to fp32 keeps the order.  -0 and +0 have the
            same key, Inf sorts above every finite value, every NaN sorts above Inf, ordered by payload.
    Columns are ranked by (key descending, column ascending).  The first `keep` columns are KEPT and their bits stay as stored;
    every other column is stored as +0.  Because NaN ranks first, a NaN is always kept, so a NaN row still makes its outputs and
    the loss NaN.

Backward is selection, not multiplication: dA_m[b][j] is unchanged where column j was kept and exactly +0 elsewhere, even under a
NaN gradient; the bias-gradient partial column sums of layer m are rewritten from those final values.  keep == Z is accepted and
is OFF; keep < 1 and keep > Z are refused.

It is part of the MODEL, like the skips and the norm: training in every step form, eval_batch, complete*, score_outfits, encode*,
code_index and weights="average" run through it; encode returns codes with at most `keep` non-zeros per row, decode(z, layer)
starts at Linear `layer` and takes z as given.

Limits: no skip or norm on layer m itself (a skip around the bottleneck adds the dense h_m back; a norm's backward needs the full
xhat, which the in-place store has overwritten) - Residual("hidden") and Norm(...) with the default "hidden" include m, so name
the layers and leave out layer m; skips and norms on every other layer are allowed, a skip around Linear `layer` included.  The
activation of layer m is none, ReLU or LeakyReLU.  Never the last layer.

SparseCode carries the choice, resolves it against a stack (resolve), hands it to the HIP engine (DaeEngine.set_sparse_code,
HipEmbeddingTrainer(sparse_code=...)) and states the same network in whole-tensor torch ops with autograd (select, apply,
forward) for host tensors and tests.
"""
import torch

from ..hip import HipError
from .residual import ALLOWED_ACTS, _ACT_NAMES, _act_tuple, _apply_act


def _int(who, v, lo):
    v = v.item() if hasattr(v, "item") and not isinstance(v, (int, bool)) else v
    if isinstance(v, bool) or not isinstance(v, int) or v < lo:
        raise HipError("sparse code: %s must be an int >= %d, got %r" % (who, lo, v))
    return int(v)


def key(x):
    """key(v) of the definition for every element of a float32 or bfloat16 tensor, as int64 (any device)."""
    if x.dtype == torch.bfloat16:
        return x.contiguous().view(torch.int16).to(torch.int64) & 0x7FFF
    if x.dtype == torch.float32:
        return x.contiguous().view(torch.int32).to(torch.int64) & 0x7FFFFFFF
    raise HipError("sparse code: values must be float32 or bfloat16 (the stored types), got %s" % (x.dtype,))


def select(x, keep):
    """The bool mask [.., Z] of the columns the definition keeps in every row of x [.., Z] (float32 or bfloat16, any device): a
    stable descending sort of the integer key, so equal keys stay in ascending column order, and its first `keep` columns."""
    Z = int(x.shape[-1])
    keep = _int("keep", keep, 1)
    if keep > Z:
        raise HipError("sparse code: keep %d outside [1, %d]" % (keep, Z))
    order = torch.sort(key(x), dim=-1, descending=True, stable=True).indices
    mask = torch.zeros(x.shape, dtype=torch.bool, device=x.device)
    mask.scatter_(-1, order[..., :keep], True)
    return mask


class SparseCode:
    """SparseCode(32) | SparseCode(32, layer=5).  keep: the units kept per row, 1 <= keep <= Z (Z = off); layer: the Linear that
    reads the code, None = the stack's code layer (tool.codes.code_layers)."""

    def __init__(self, keep, layer=None):
        self.keep = _int("keep", keep, 1)
        self.layer = None if layer is None else _int("layer", layer, 1)

    def __repr__(self):
        return "SparseCode(%d, layer=%r)" % (self.keep, self.layer)

    select = staticmethod(select)

    def resolve(self, in_features, out_features, activation, residual=None, norm=None):
        """(m, Z) of this choice on a stack: in_features / out_features per layer, activation per layer (a bool = ReLU or none, a
        CODAE_ACT_* kind, or the engine's (kind, p0, p1, p2)); residual / norm: None or the codae.tool.Residual / Norm of the same
        stack.  HipError naming the layer and the reason when the stack cannot take it."""
        L = len(in_features)
        if len(out_features) != L or len(activation) != L:
            raise HipError("sparse code: %d input widths, %d output widths, %d activations" % (L, len(out_features), len(activation)))
        acts = [_act_tuple(a) for a in activation]
        layer = self.layer
        if layer is None:
            from .codes import code_layers
            layer = code_layers([(i, o, a) for i, o, a in zip(in_features, out_features, acts)])
        if layer == L:
            raise HipError("sparse code: layer %d: the last layer's output is the reconstruction and takes no sparse code" % (L - 1))
        if not 1 <= layer <= L - 1:
            raise HipError("sparse code: layer must be in [1, %d], got %d" % (L - 1, layer))
        m, Z = layer - 1, int(out_features[layer - 1])
        if acts[m][0] not in ALLOWED_ACTS:
            raise HipError("sparse code: layer %d: the sparse layer's activation must be none, ReLU or LeakyReLU (got %s)" % (
                m, _ACT_NAMES.get(acts[m][0], acts[m][0])))
        if not 1 <= self.keep <= Z:
            raise HipError("sparse code: keep %d outside [1, %d], the width of layer %d's output" % (self.keep, Z, m))
        if residual is not None and residual.resolve(in_features, out_features, acts)[m]:
            raise HipError("sparse code: layer %d: the sparse layer takes no skip (it would add the dense h_%d back): name the layers and "
                           "leave out layer %d" % (m, m, m))
        if norm is not None and norm.resolve(in_features, out_features, acts)[m]:
            raise HipError("sparse code: layer %d: the sparse layer takes no norm (its backward needs the full xhat): name the layers and "
                           "leave out layer %d" % (m, m))
        return m, Z

    def apply(self, x):
        """torch.where(select(x, keep), x, 0): the kept entries keep their bits and carry the gradient, the others are +0."""
        return torch.where(select(x.detach(), self.keep), x, torch.zeros((), dtype=x.dtype, device=x.device))

    def forward(self, x, weights, biases, activation, residual=None, norm=None, dropout_factors=None, layers=None):
        """h_L of the definition (codae.tool.norm's network with the sparse layer) in whole-tensor torch ops (autograd works through
        it).  weights[l]: [out, in], biases[l]: [out]; activation as resolve takes it; residual / norm: None or the stack's
        codae.tool.Residual / Norm; dropout_factors: None, or per layer None / a [B, out[l]] tensor that multiplies a_l.
        layers: stop behind Linear layers - 1 (h_layers); None = the whole stack."""
        L = len(weights)
        acts = [_act_tuple(a) for a in activation]
        ins, outs = [int(w.shape[1]) for w in weights], [int(w.shape[0]) for w in weights]
        m, Z = self.resolve(ins, outs, acts, residual, norm)
        skips = residual.resolve(ins, outs, acts) if residual is not None else [0] * L
        flags = norm.resolve(ins, outs, acts) if norm is not None else [0] * L
        h = x
        for l in range(L if layers is None else layers):
            a = _apply_act(acts[l], h @ weights[l].t() + biases[l])
            if dropout_factors is not None and l < len(dropout_factors) and dropout_factors[l] is not None:
                a = a * dropout_factors[l]
            s = a + h if skips[l] else a
            h = norm.normalise(s) if flags[l] else s
            if l == m and self.keep < Z:
                h = self.apply(h)
        return h


def meta_record(sparse, resolved):
    """What a checkpoint's meta keeps under "sparse_code" for a trainer whose setting resolved to `resolved` = (m, Z) or None:
    {keep, layer}, or None when it is off (the key is then not written at all)."""
    if sparse is None or not resolved or sparse.keep >= resolved[1]:
        return None
    return {"keep": int(sparse.keep), "layer": int(resolved[0]) + 1}


def meta_mismatch(meta, sparse, resolved):
    """The checkpoint's structure check: None when the file's record (meta["sparse_code"]: {keep, layer}; a file without the key has
    none) is the trainer's, else the sentence that says how they differ."""
    in_file = meta.get("sparse_code") or None
    mine = meta_record(sparse, resolved)

    def say(r):
        return "none" if r is None else "keep %d at layer %d" % (int(r["keep"]), int(r["layer"]))
    if in_file is None and mine is None:
        return None
    if in_file is not None and mine is not None and int(in_file.get("keep", 0)) == mine["keep"] and int(in_file.get("layer", 0)) == mine["layer"]:
        return None
    return "the file was written with sparse code: %s, this trainer has sparse code: %s" % (say(in_file), say(mine))


def sparse_from_meta(meta):
    """The SparseCode a checkpoint's record describes, or None."""
    r = meta.get("sparse_code") or None
    if r is None:
        return None
    return SparseCode(int(r["keep"]), layer=int(r["layer"]))


def sparse_from_config(block):
    """The `HIP: SPARSE_CODE:` block of the embedding script's config: {KEEP: 32, LAYER: null}.  None / empty -> None."""
    if not block:
        return None
    if not isinstance(block, dict):
        raise HipError("SPARSE_CODE must be a mapping with KEEP and LAYER, got %r" % (block,))
    known = {"KEEP", "LAYER"}
    extra = sorted(set(block) - known, key=str)
    if extra:
        raise HipError("SPARSE_CODE: unknown key(s) %s (known: %s)" % (", ".join(map(str, extra)), ", ".join(sorted(known))))
    if "KEEP" not in block:
        raise HipError("SPARSE_CODE: KEEP is required (the units kept per row)")
    return SparseCode(block["KEEP"], layer=block.get("LAYER", None))
