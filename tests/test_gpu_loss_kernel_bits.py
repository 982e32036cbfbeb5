"""The stored bits of the stand-alone loss kernels, pinned: mse_loss_kernel, emph_loss_kernel, recon_elem_kernel, slot_cosine_kernel
and slot_contrast_kernel through the C primitives, on inputs built on the CPU from fixed seeds, compared by the sha256 of the raw
bytes of dY (pad columns included, prefilled), the partial column-sum rows and the per-block sums with the recorded ones.
tests/golden/loss_kernel_bits.json names every group and case in order; the digests themselves (32 raw bytes per array, three
arrays per case, in that order) are in tests/golden/loss_kernel_bits.sha256 beside it (2064 digests: 190 KB as hex text).

The digests pin the code gfx950's compiler generates for these kernels - the order of every addition, which neighbouring columns
share a packed instruction - and not a definition: the definitions are checked, with tolerances, by test_gpu_emphasis.py,
test_gpu_recon_loss.py, test_gpu_presence.py and test_gpu_slot_contrast.py.  A change that only moves code around must leave every
digest as it is.  They are re-recorded (python tests/test_gpu_loss_kernel_bits.py, on an MI355X, from a build of the commit whose
arithmetic is the wanted one) only by a change that MEANS to change arithmetic and says so.

Shapes: the smallest at which each branch exists.  B = 33 (two row blocks, the second with one live row); io = 24 with S = 3 (a
16-byte group inside one slot) and S = 4 (E = 6: groups straddle slots), io = 21 with S = 3 (the scalar path); dY fp32 with
ld = io and bf16 with ld = 64.  Over these: MSE with and without gradient, emphasis (alpha 3, beta 0.5, slot weights 0.5 / 1 / 2),
L1, SmoothL1, Huber, the slot cosine with mse_weight 0 and 0.5, each with noise off and MASKING p = 0.25 and the criteria also
without emphasis; permuted row_idx + mask_id, null row_idx + mask_to_use / run, no mask; no presence table, and one with about 20 %
absent slots (at least one present per row) and NaN in x under the absent ones.  The contrast: io 48, S 4, K 33, fp32 and bf16,
with and without the table.
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "mui-deepautoencoder_amd")]

import contrast_ref as CR
import emphasis_ref as ER
import presence_ref as PR
import recon_loss_ref as RR

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_kernel_bits.json")
ARRAYS = ("dy", "colsum_part", "parts")
DEV = "cuda:0"
N, B, STEP, FILL = 120, 33, 5, 7.0
ALPHA, BETA = 3.0, 0.5
KIND_ID = dict(zip(("mse",) + RR.KINDS, range(5)))
SHAPES = [(24, 3), (24, 4), (21, 3)]
DY_FORMS = [("f32", False, None), ("bf16-ld64", True, 64)]
# (name, which, criterion (kind, param, mse_weight) or None, emphasis on, MASKING noise on, want dy)
KERNELS = [("mse", "mse", None, False, False, True), ("mse-sums-only", "mse", None, False, False, False)]
for _n in (False, True):
    KERNELS.append(("emph" + ("+masking" if _n else ""), "emph", None, True, _n, True))
for _k, _p, _mw in (("l1", 0.0, 0.0), ("smooth_l1", 0.5, 0.0), ("huber", 0.75, 0.0), ("slot_cosine", 0.0, 0.0), ("slot_cosine", 0.0, 0.5)):
    _name = _k + ("+mse0.5" if _mw else "")
    KERNELS.append((_name, "recon", (_k, _p, _mw), False, False, True))
    for _n in (False, True):
        KERNELS.append((_name + "+emph" + ("+masking" if _n else ""), "recon", (_k, _p, _mw), True, _n, True))


def _problem(io, S):
    """emphasis_ref.problem plus a presence table (about 20 % absent, every row keeps a slot), the data with NaN under the absent
    slots (used with the table) and with zeros there (used without), and the slot weights."""
    p = dict(ER.problem(io, S=S, N=N, B=B))
    E = io // S
    t = PR.make_table(N, S, p_absent=0.2, min_keep=1)
    assert (t.sum(axis=1) >= 1).all() and 0.1 < (t == 0).mean() < 0.3
    pm = np.repeat(t != 0, E, axis=1)
    p.update(E=E, present=t, data_nan=np.where(pm, p["data"], np.float32(np.nan)), data0=np.where(pm, p["data"], np.float32(0)),
             cw=np.repeat(np.float32([0.5, 1.0, 2.0, 1.0][:S]), E))
    return p


def _sha(t):
    import torch
    raw = t.contiguous().view(torch.uint8).cpu().numpy().tobytes()
    return hashlib.sha256(raw).hexdigest()


def _digests(dy, colsum, parts):
    return dict(zip(ARRAYS, (_sha(dy), _sha(colsum), _sha(parts))))


def _dev(p):
    import torch
    return {k: torch.tensor(p[k], device=DEV) for k in ("data_nan", "data0", "y", "table", "rows", "mask_id", "mtu", "present", "cw")}


def _routes(d):
    return [("mask_id", dict(row_idx=d["rows"], mask_id=d["mask_id"], table=d["table"])),
            ("mask_to_use", dict(table=d["table"], mask_to_use=d["mtu"], run=2)),
            ("no-mask", dict(row_idx=d["rows"]))]


def _batch(data, row_idx=None, mask_id=None, table=None, mask_to_use=None, run=0):
    from codae import hip
    return hip.Batch(hip.ptr(data), hip.ptr(row_idx), hip.ptr(mask_id), hip.ptr(table), B, int(data.shape[1]), hip.ptr(mask_to_use),
                     0 if mask_to_use is None else int(mask_to_use.shape[1]), run)


def _noise():
    from codae import hip
    return hip.Noise(2, 0.25, 0.0, 0.0, ER.SEED)          # CODAE_NOISE_MASKING


def loss_bits(d, io, S, kernel, bf16, ld, route, with_table):
    import torch
    from codae import hip
    lib = hip.lib()
    name, which, crit, emph_on, noise_on, want_dy = kernel
    ld = io if ld is None else ld
    blocks = (B + 31) // 32
    dy = torch.full((B, ld), FILL, dtype=torch.bfloat16 if bf16 else torch.float32, device=DEV)
    colsum = torch.full((blocks, io), FILL, dtype=torch.float32, device=DEV)
    parts = torch.full((blocks, 2 if which == "mse" else 3), FILL, dtype=torch.float64, device=DEV)
    batch = _batch(d["data_nan"] if with_table else d["data0"], **route)
    noise = C.byref(_noise()) if noise_on else None
    em = C.byref(hip.Emphasis(ALPHA, BETA, hip.ptr(d["cw"]))) if emph_on else None
    pres = (hip.ptr(d["present"]), S) if with_table else (None, 0)
    inv, s = 1.0 / (B * io), hip.current_stream()
    if which == "mse":
        rc = lib.codae_mse_loss_present(C.byref(batch), hip.ptr(d["y"]), hip.ptr(dy) if want_dy else None, int(bf16), ld, inv, hip.ptr(colsum),
                                        hip.ptr(parts), pres[0], pres[1], s)
    elif which == "emph":
        args = (C.byref(batch), noise, STEP, em, hip.ptr(d["y"]), hip.ptr(dy), int(bf16), ld, inv, hip.ptr(colsum), hip.ptr(parts))
        rc = lib.codae_emph_loss_present(*args, pres[0], pres[1], s) if with_table else lib.codae_emph_loss(*args, s)
    else:
        kind, param, mw = crit
        st = hip.ReconLoss(KIND_ID[kind], param, mw, S if kind == "slot_cosine" else 0)
        args = (C.byref(batch), noise, STEP, em, C.byref(st), hip.ptr(d["y"]), hip.ptr(dy), int(bf16), ld, inv, hip.ptr(colsum), hip.ptr(parts))
        rc = lib.codae_recon_loss_fwd_bwd_present(*args, pres[0], pres[1], s) if with_table else lib.codae_recon_loss_fwd_bwd(*args, s)
    torch.cuda.synchronize()
    assert rc == 0, lib.codae_last_error()
    return _digests(dy, colsum, parts)


def loss_cases(io, S, form):
    """{case name: digests} of every kernel x route x table for one shape and dY form."""
    _, bf16, ld = form
    d = _dev(_problem(io, S))
    out = {}
    for kernel in KERNELS:
        for rname, route in _routes(d):
            for with_table in (False, True):
                out["%s/%s/%s" % (kernel[0], rname, "table" if with_table else "no-table")] = loss_bits(d, io, S, kernel, bf16, ld, route, with_table)
    return out


def contrast_cases(bf16):
    """io 48, S 4, K 33 on the mask_id route, with emphasis and MASKING noise, on top of a fixed dY; with and without the table."""
    import torch
    from codae import hip
    lib = hip.lib()
    io, S, K = 48, 4, 33
    p = _problem(io, S)
    d = _dev(p)
    dt = torch.bfloat16 if bf16 else torch.float32
    blocks = (B + CR.BLOCK - 1) // CR.BLOCK
    dy_in = (np.random.default_rng(io + K).standard_normal((B, io)) * 1e-2).astype(np.float32)
    ids = torch.tensor(CR.item_ids(p["data0"], S).astype(np.int32), device=DEV)
    out = {}
    for with_table in (False, True):
        data = d["data_nan"] if with_table else d["data0"]
        g = dy_in.copy()
        if with_table:
            g[~PR.pmask(p["present"], p["rows"], p["E"])] = 0.0                  # what the criterion's kernel leaves there
        dy = torch.tensor(g, device=DEV).to(dt)
        colsum = torch.full((blocks, io), FILL, dtype=torch.float32, device=DEV)
        parts = torch.full((blocks,), FILL, dtype=torch.float64, device=DEV)
        ws = torch.full((lib.codae_slot_contrast_ws_bytes(S, K, io // S, int(bf16)),), 0xFF, dtype=torch.uint8, device=DEV)
        st = hip.SlotContrast(S, K, 0.1, 0.7, 0x5EED0000C0DA0001, N, 0, int(ws.numel()), None, hip.ptr(ids), hip.ptr(ws))
        batch = _batch(data, row_idx=d["rows"], mask_id=d["mask_id"], table=d["table"])
        noise, em = _noise(), hip.Emphasis(ALPHA, BETA, hip.ptr(d["cw"]))
        scale, s = float(np.float32(0.7 / (B * S))), hip.current_stream()
        args = (C.byref(batch), C.byref(noise), STEP, C.byref(em), C.byref(st), hip.ptr(d["y"]), hip.ptr(dy), int(bf16), io, scale, hip.ptr(colsum),
                hip.ptr(parts))
        if with_table:
            rc = lib.codae_slot_contrast_prepare_present(hip.ptr(data), io, C.byref(st), STEP, int(bf16), hip.ptr(d["present"]), S, s)
            rc = rc or lib.codae_slot_contrast_fwd_bwd_present(*args, hip.ptr(d["present"]), S, s)
        else:
            rc = lib.codae_slot_contrast_prepare(hip.ptr(data), io, C.byref(st), STEP, int(bf16), s)
            rc = rc or lib.codae_slot_contrast_fwd_bwd(*args, s)
        torch.cuda.synchronize()
        assert rc == 0, lib.codae_last_error()
        out["contrast/%s" % ("table" if with_table else "no-table")] = _digests(dy, colsum, parts)
    return out


GROUPS = [("io%d-s%d-%s" % (io, S, form[0]), (lambda io=io, S=S, form=form: loss_cases(io, S, form))) for io, S in SHAPES for form in DY_FORMS]
GROUPS += [("contrast-io48-k33-" + ("bf16" if b else "f32"), (lambda b=b: contrast_cases(b))) for b in (False, True)]


def write_golden(rec, path):
    """rec {group: {case: {array: hex digest}}} -> the index `path` and the digest file beside it."""
    index = {"arrays": list(ARRAYS), "digests": os.path.splitext(os.path.basename(path))[0] + ".sha256",
             "groups": [[g, sorted(rec[g])] for g in sorted(rec)]}
    # (the six shape groups run the same cases: their list is written once and referred to by the first group's name)
    first = {}
    for entry in index["groups"]:
        key = tuple(entry[1])
        if key in first:
            entry[1] = first[key]
        else:
            first[key] = entry[0]
    with open(path, "w") as f:
        json.dump(index, f, indent=1)
        f.write("\n")
    with open(os.path.join(os.path.dirname(path), index["digests"]), "wb") as f:
        for g in sorted(rec):
            for case in sorted(rec[g]):
                for arr in ARRAYS:
                    f.write(bytes.fromhex(rec[g][case][arr]))


def read_golden(path=GOLDEN):
    """-> {group: {case: {array: hex digest}}}"""
    with open(path) as f:
        index = json.load(f)
    with open(os.path.join(os.path.dirname(path), index["digests"]), "rb") as f:
        blob = f.read()
    lists = {g: cases for g, cases in index["groups"] if isinstance(cases, list)}
    rec, at = {}, 0
    for g, cases in index["groups"]:
        rec[g] = {}
        for case in (cases if isinstance(cases, list) else lists[cases]):
            rec[g][case] = {}
            for arr in index["arrays"]:
                rec[g][case][arr] = blob[at:at + 32].hex()
                at += 32
    assert at == len(blob), "the digest file does not match its index"
    return rec


@pytest.mark.parametrize("group,run", GROUPS, ids=[g for g, _ in GROUPS])
def test_stored_bits_are_the_recorded_ones(group, run):
    pytest.importorskip("torch")
    want = read_golden()[group]
    got = run()
    assert sorted(got) == sorted(want)
    moved = ["%s %s" % (case, arr) for case in sorted(got) for arr in ARRAYS if got[case][arr] != want[case][arr]]
    assert not moved, "%d of %d arrays moved: %s" % (len(moved), 3 * len(got), ", ".join(moved[:12]))


if __name__ == "__main__":
    out_path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    rec = {group: run() for group, run in GROUPS}
    write_golden(rec, out_path)
    print("recorded %d groups, %d cases -> %s" % (len(rec), sum(len(v) for v in rec.values()), out_path))
