"""Helpers shared by the multi-key group-by tests: hand-built
row-v1 / row-v2 regions from dict rows, and a small Python group-by that is
the reference where the oracle, which takes one group-by expression, cannot
be asked directly. test_group_multi_ref_cpu.py pins this reference against
the oracle with one key."""
import ctypes as C

from topn_multi_util import (U64, cell_int, cell_null, cell_uint, orc,  # noqa: F401
                             region_of, row_key, split_int_rows)


def _v2_int(v):
    v &= U64
    if v <= 0x7F:
        return bytes([v])
    if v <= 0x7FFF:
        return v.to_bytes(2, "little")
    if v <= 0x7FFFFFFF:
        return v.to_bytes(4, "little")
    return v.to_bytes(8, "little")


def row_v2(r, unsigned=()):
    """row-v2 (small layout) of one dict row {col_id: int-or-None}; ids below
    256. Non-negative values below 2^(8w-1) take w bytes, which reads the same
    signed or unsigned; everything else takes 8."""
    nn = sorted(c for c in r if r[c] is not None)
    nul = sorted(c for c in r if r[c] is None)
    body, ends = b"", []
    for c in nn:
        body += _v2_int(r[c])
        ends.append(len(body))
    out = bytes([128, 0]) + len(nn).to_bytes(2, "little") \
        + len(nul).to_bytes(2, "little")
    out += bytes(nn) + bytes(nul)
    for e in ends:
        out += e.to_bytes(2, "little")
    return out + body


def row_v1(r, unsigned=()):
    v = b""
    for cid in sorted(r):
        x = r[cid]
        if x is None:
            v += cell_null(cid)
        elif cid in unsigned:
            v += cell_uint(cid, x)
        else:
            v += cell_int(cid, x)
    return v


def region_of_bytes(row_vals):
    """per-row value byte strings -> (keys, key_offs, vals, val_offs, n,
    keepalive), handles 0..n-1"""
    keys = b"".join(row_key(i) for i in range(len(row_vals)))
    vals = b"".join(row_vals)
    vo = [0]
    for v in row_vals:
        vo.append(vo[-1] + len(v))
    ko = [19 * i for i in range(len(row_vals) + 1)]
    kb = (C.c_uint8 * max(len(keys), 1)).from_buffer_copy(keys or b"\0")
    vb = (C.c_uint8 * max(len(vals), 1)).from_buffer_copy(vals or b"\0")
    return (C.cast(kb, C.POINTER(C.c_uint8)), (C.c_uint64 * len(ko))(*ko),
            C.cast(vb, C.POINTER(C.c_uint8)), (C.c_uint64 * len(vo))(*vo),
            len(row_vals), (kb, vb))


def build_region(rows, unsigned=(), v2=False, tail=None):
    """dict rows -> region arrays; tail(i) = raw cell bytes appended to
    row-v1 row i (cells of higher column ids that are not ints)"""
    out = []
    for i, r in enumerate(rows):
        if v2:
            out.append(row_v2(r, unsigned))
        else:
            out.append(row_v1(r, unsigned) + (tail(i) if tail else b""))
    return region_of_bytes(out)


class Key:
    """one group-by column of the reference: an absent cell takes `default`
    (None = NULL), the datum comes back as flag 4 when unsigned, else 3"""

    def __init__(self, col_id, unsigned=False, default=None):
        self.col_id = col_id
        self.unsigned = unsigned
        self.default = default

    def cell(self, r):
        return r[self.col_id] if self.col_id in r else self.default

    def datum(self, v):
        if v is None:
            return (0, None)
        return (4, v & U64) if self.unsigned else (3, v)


def group_ref(rows, keys, aggs, keep=None, agg_unsigned=()):
    """GROUP BY keys over dict rows. aggs: ("count_star",), ("count", col),
    ("max", col), ("min", col); an aggregate column's absent cell is NULL.
    keep(r) drops rows. Returns the sorted list of output rows in
    split_int_rows form: aggregate datums, then one datum per key."""
    groups = {}
    for r in rows:
        if keep is not None and not keep(r):
            continue
        t = tuple(k.cell(r) for k in keys)
        groups.setdefault(t, []).append(r)
    out = []
    for t, rs in groups.items():
        row = []
        for a in aggs:
            if a[0] == "count_star":
                row.append((3, len(rs)))
                continue
            vals = [r[a[1]] for r in rs if r.get(a[1]) is not None]
            if a[0] == "count":
                row.append((3, len(vals)))
            elif not vals:
                row.append((0, None))
            else:
                v = max(vals) if a[0] == "max" else min(vals)
                row.append((4, v) if a[1] in agg_unsigned else (3, v))
        for k, v in zip(keys, t):
            row.append(k.datum(v))
        out.append(tuple(row))
    return sorted(out, key=repr)


def rows_of(data, n_cols):
    """a datum-encoded response as group_ref returns rows"""
    return sorted(split_int_rows(data, n_cols), key=repr)
