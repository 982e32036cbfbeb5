"""The far-offset shapes do what they are for (no GPU, no torch): from tests/far_offsets.py alone,

  - every table has a probe row in every class: straddling, wholly above and two controls below each boundary, and the last row;
  - for every probe row, the address a kernel would reach had it formed the offset as a signed 32-bit element index, an unsigned one,
    or a 32-bit byte offset of either sign differs from the 64-bit address wherever the row's class says that slip is its business
    (far_offsets.detects) - the proof that a truncating kernel reads something else than the near call, i.e. NaN fill or another row;
  - and every such address lies inside the arena: the slip is a failed assertion, not an illegal access.  This is the headroom
    arithmetic of DESIGN.md, "Far offsets"."""
import pytest

import far_offsets as F

# (name, io, element size, rows or None, bytes above the arena base, arena bytes)
TABLES = []
for io in F.WIDTHS:
    TABLES.append(("f32-io%d" % io, io, 4, None, F.HEADROOM, F.ARENA_BYTES))
    TABLES.append(("bf16-io%d" % io, io, 2, None, F.HEADROOM, F.ARENA_BYTES))
    TABLES.append(("u8-io%d" % io, io, 1, None, F.HEADROOM, F.ARENA_BYTES))
    # the bf16 image of the fp32 dataset, in the second arena
    TABLES.append(("image-io%d" % io, io, 2, F.n_obs(io, 4), F.IMAGE_HEADROOM, F.IMAGE_ARENA_BYTES))
    # the inventory [S][n_obs][E] read as S * n_obs rows of E
    S = F.SLOTS[io]
    TABLES.append(("inventory-E%d" % (io // S), io // S, 4, S * F.n_obs(io, 4), F.HEADROOM, F.ARENA_BYTES))
IDS = [t[0] for t in TABLES]


def test_the_arenas_fit_the_cap_and_the_regions_hold_the_tables():
    assert F.ARENA_BYTES + F.IMAGE_ARENA_BYTES <= F.CAP_BYTES
    assert F.B % 64 != 0 and F.B == 70
    for name, io, es, rows, head, arena in TABLES:
        n = F.n_obs(io, es) if rows is None else rows
        assert head + n * io * es + F.GUARD * es <= arena, name
        if rows is None:
            assert (n - 1) * io < F.top_boundary(es) + F.MIB <= n * io, name
    assert F.n_obs(24, 4) < 2 ** 31 and F.n_obs(24, 2) < 2 ** 31                 # row_idx stays int32
    assert F.n_obs(1536, 4) == 1398784                                           # the 1.4 M outfits of the headline width


@pytest.mark.parametrize("name,io,es,rows,head,arena", TABLES, ids=IDS)
def test_every_table_has_a_probe_row_of_every_class(name, io, es, rows, head, arena):
    n = F.n_obs(io, es) if rows is None else rows
    probes = F.probe_rows(io, es, rows)
    classes = [c for _, c in probes]
    inside = [b for b, off in F.boundaries(es) if off < n * io]
    assert "e31" in inside and "b32" in inside
    if es <= 2 and rows is None:
        assert "e32" in inside
    for b in inside:
        straddles = 0 if dict(F.boundaries(es))[b] % io == 0 else 1
        assert straddles == (0 if name.startswith("inventory") else 1), (name, b)   # E = 8 and 512 divide every power of two
        assert classes.count(b + "-straddle") == straddles and classes.count(b + "-above") == 1 and classes.count(b + "-control") == 2, (name, b)
    assert classes.count("last") == 1 and (n - 1, "last") in probes
    offs = dict(F.boundaries(es))
    for r, c in probes:
        b = c.split("-")[0]
        if c.endswith("straddle"):
            assert r * io < offs[b] <= r * io + io - 1                           # first element below, last element above
        elif c.endswith("above"):
            assert (r - 1) * io <= offs[b] <= r * io
        elif c.endswith("control"):
            assert (r + 1) * io <= offs[b]
    batch = F.batch_rows(io, es, 1, rows)
    assert len(batch) == F.B and set(batch) == set(F.distinct_rows(io, es, rows)) and batch != sorted(batch)


@pytest.mark.parametrize("name,io,es,rows,head,arena", TABLES, ids=IDS)
def test_a_32_bit_offset_reads_another_address_inside_the_arena(name, io, es, rows, head, arena):
    seen = set()
    for r, c in F.probe_rows(io, es, rows):
        last = r * io + io - 1
        true = last * es
        for kind in F.KINDS:
            got = F.trunc(last, es, kind)
            assert 0 <= head + got and head + got + es <= arena, (name, r, c, kind)          # inside the arena, element and all
            if kind in F.detects(c, es, last):
                assert got != true, (name, r, c, kind)
                seen.add(kind)
            elif kind not in F.slips_past(last, es):
                assert got == true, (name, r, c, kind)                                       # a form that holds the offset reads it right
    # an unsigned element index is caught only by a table of more than 2^32 elements (left out for fp32 tables)
    want = set(F.KINDS) if es <= 2 and rows is None else {"i32", "b32s", "b32u"}
    assert seen == want, (name, seen)
    # a control row holds at least one form that its boundary's rows do not: it is the same read with that slip harmless
    offs = dict(F.boundaries(es))
    for r, c in F.probe_rows(io, es, rows):
        if c.endswith("control"):
            assert set(F.slips_past(r * io + io - 1, es)) < set(F.slips_past(offs[c.split("-")[0]], es)), (name, r, c)


def test_the_leading_dimensions_put_the_last_row_past_the_boundary():
    for es, align, width in ((4, 4, 1536), (4, 1, 21), (2, 8, 1536), (2, 8, 24), (4, 4, 20), (4, 1, 1537)):
        ld = F.far_ld(es, align)
        top = F.top_boundary(es)
        assert ld % align == 0 and ld > width + F.GUARD
        assert (F.B - 2) * ld <= top < (F.B - 1) * ld                            # row 68 starts at or below it, row 69 wholly above
        assert top - (F.B - 2) * ld < (F.B - 2) * align + F.B - 2                # row 68 sits on it: within 68 (align + 1) elements
        assert F.HEADROOM + F.ld_span_bytes(es, align, width) <= F.ARENA_BYTES
        last = (F.B - 1) * ld + width - 1
        for kind in F.KINDS:
            got = F.trunc(last, es, kind)
            assert 0 <= F.HEADROOM + got and F.HEADROOM + got + es <= F.ARENA_BYTES
            if kind != "u32" or es <= 2:
                assert got != last * es, (es, align, kind)
