"""The shapes of the far-offset tests (tests/test_gpu_far_offsets.py), in plain integers: no torch, no numpy.

A table is [n_obs][io] of `es`-byte elements, a view into an arena that starts HEADROOM bytes above the arena's base.  Its probe
rows are the rows whose offsets sit on the boundaries a 32-bit offset cannot pass:

  e31   element offset 2^31     every table
  e32   element offset 2^32     tables of 2-byte and 1-byte elements only (an fp32 table that large would be 16 GiB)
  b32   byte offset 2^32        every table (in a bf16 table it is the row of e31)

For each boundary: the row that straddles it (first element below, last element above; none where the width divides the boundary),
the first row wholly above it and two rows wholly below it as controls; and the last row of the table.  n_obs = ceil((top boundary + 2^20) / io).

trunc() restates what a kernel that formed the offset in 32 bits would address; tests/test_far_offset_shapes_host.py proves from
it that every such slip reads another address than the true one, and that the address lies inside the arena - a wrong value, never
a fault."""

GIB = 1 << 30
MIB = 1 << 20
HEADROOM = 8 * GIB                         # a signed 32-bit ELEMENT index into an fp32 table wraps at most 2^31 * 4 bytes below the base
TABLE_REGION = (1 << 33) + 64 * MIB
TAIL = 64 * MIB
ARENA_BYTES = HEADROOM + TABLE_REGION + TAIL
# the second arena holds the bf16 image of the fp32 dataset while the engine case has both: 2^31 + d elements of 2 bytes
IMAGE_HEADROOM = 4 * GIB                   # a signed 32-bit element index into a bf16 table wraps at most 2^31 * 2 bytes below the base
IMAGE_REGION = 4 * GIB + 64 * MIB
IMAGE_ARENA_BYTES = IMAGE_HEADROOM + IMAGE_REGION
CAP_BYTES = 26 * GIB
FILL16 = 0x7FC0                            # every aligned 16-bit word: a bf16 NaN, the fp32 NaN 0x7fc07fc0, non-zero bytes
GUARD = 64                                 # elements behind every written output row that must keep the fill
B = 70                                     # batch rows: not a multiple of 64
WIDTHS = (24, 1536)                        # the scalar and narrow paths (S = 3 or 4); the 16-byte paths and the 256 x 192 tile
SLOTS = {24: 3, 1536: 3}
E31, E32, B32 = 1 << 31, 1 << 32, 1 << 32

assert ARENA_BYTES + IMAGE_ARENA_BYTES <= CAP_BYTES


def top_boundary(es):
    """the highest element boundary a table of es-byte elements is taken past"""
    return E31 if es == 4 else E32


def n_obs(io, es):
    return -(-(top_boundary(es) + MIB) // io)


def boundaries(es):
    """(name, element offset) of every boundary inside a table of es-byte elements"""
    out = [("e31", E31), ("b32", B32 // es)]
    if es <= 2:
        out.append(("e32", E32))
    return out


def probe_rows(io, es, rows=None):
    """[(row, class)]: class is `<boundary>-straddle`, `<boundary>-above`, `<boundary>-control` or `last`; ascending rows, a row
    that belongs to two classes (b32 and e31 of a bf16 table) listed once per class.  `rows`: a shorter table of the same width (the
    bf16 image of an fp32 dataset has the dataset's n_obs)."""
    n = n_obs(io, es) if rows is None else rows
    out = []
    for name, off in boundaries(es):
        if off >= n * io:
            continue
        r = off // io
        if off % io:
            out += [(r - 2, name + "-control"), (r - 1, name + "-control"), (r, name + "-straddle"), (r + 1, name + "-above")]
        else:       # a width that divides the boundary (the inventory's E = 8 and 512): no row straddles, row r starts on it
            out += [(r - 2, name + "-control"), (r - 1, name + "-control"), (r, name + "-above")]
    out.append((n - 1, "last"))
    assert all(0 <= r < n for r, _ in out)
    return sorted(out)


def distinct_rows(io, es, rows=None):
    return sorted({r for r, _ in probe_rows(io, es, rows)})


def batch_rows(io, es, seed, rows=None):
    """B batch rows: the probe rows, repeated and shuffled (a plain LCG: no numpy here)"""
    pr = distinct_rows(io, es, rows)
    out = [pr[i % len(pr)] for i in range(B)]
    s = seed * 2654435761 % (1 << 32) or 1
    for i in range(B - 1, 0, -1):
        s = (s * 1664525 + 1013904223) % (1 << 32)
        j = (s >> 8) % (i + 1)
        out[i], out[j] = out[j], out[i]
    return out


def _s32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v & 0x80000000 else v


def trunc(off, es, kind):
    """the BYTE offset from the table base that a kernel reaches for element offset `off` when it forms, in 32 bits,
       i32 / u32    the element index (the pointer arithmetic behind it is 64-bit)
       b32s / b32u  the byte offset"""
    if kind == "i32":
        return _s32(off) * es
    if kind == "u32":
        return (off & 0xFFFFFFFF) * es
    if kind == "b32s":
        return _s32(off * es)
    if kind == "b32u":
        return (off * es) & 0xFFFFFFFF
    raise ValueError(kind)


KINDS = ("i32", "u32", "b32s", "b32u")


def slips_past(off, es):
    """the 32-bit forms that cannot hold element offset `off` of es-byte elements"""
    return tuple(k for k, over in (("i32", off >= 1 << 31), ("u32", off >= 1 << 32), ("b32s", off * es >= 1 << 31),
                                   ("b32u", off * es >= 1 << 32)) if over)


def detects(cls, es, last_off):
    """the slips a probe row of class `cls` must turn into another address, judged on its LAST element, offset last_off (a
    straddling row's first element lies below the boundary): every form that cannot hold the boundary the class is named after, or,
    for the last row, its own offset.  An unsigned element index passes 2^31 unharmed, so only rows past e32 catch it; a control
    row catches nothing by design."""
    if cls.endswith("control"):
        return ()
    return slips_past(last_off if cls == "last" else dict(boundaries(es))[cls.split("-")[0]], es)


# ---- leading dimensions -----------------------------------------------------------------------------------------------------------------

def far_ld(es, align):
    """the row spacing, in elements and a multiple of `align`, at which row B - 2 of a [B][ld] matrix ends just below or across the
    top boundary of its element size and row B - 1 starts ld - 68 * align or more above it"""
    ld = top_boundary(es) // (B - 2)
    return ld - ld % align


def ld_span_bytes(es, align, width):
    return ((B - 1) * far_ld(es, align) + width + GUARD) * es
