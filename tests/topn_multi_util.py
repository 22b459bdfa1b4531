"""Helpers shared by test_topn_multi.py and test_topn_multi_oracle.py:
hand-built row-v1 regions with signed / unsigned int cells, NULL cells and
absent cells (test_topn_stream.py's region_of, plus VAR_UINT cells)."""
import ctypes as C
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

U64 = 2**64 - 1
INT64_MIN = -2**63
INT64_MAX = 2**63 - 1


def orc():
    spec = importlib.util.spec_from_file_location(
        "orc_ffi", os.path.join(ROOT, "oracle", "orc_ffi.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def var_u64(v):
    out = bytearray()
    while v >= 0x80:
        out.append(0x80 | (v & 0x7F))
        v >>= 7
    out.append(v)
    return bytes(out)


def var_i64(v):
    uv = (v << 1) ^ (U64 if v < 0 else 0)
    return var_u64(uv & U64)


def cell_int(col_id, v):
    return b"\x08" + var_i64(col_id) + b"\x08" + var_i64(v)


def cell_uint(col_id, v):
    """VAR_UINT datum (flag 9): the full unsigned 64-bit range"""
    return b"\x08" + var_i64(col_id) + b"\x09" + var_u64(v)


def cell_null(col_id):
    return b"\x08" + var_i64(col_id) + b"\x00"


def int_datum(v):
    """a column default_val: one VAR_INT datum"""
    return b"\x08" + var_i64(v)


def uint_datum(v):
    return b"\x09" + var_u64(v)


def row_key(handle, table_id=5):
    return (b"t" + table_id.to_bytes(8, "big") + b"_r"
            + ((handle ^ (1 << 63)) & U64).to_bytes(8, "big"))


def region_of(rows, unsigned=()):
    """rows: list of dicts {col_id: int-or-None}; a col_id missing from the
    dict is an absent cell. Columns in `unsigned` are written as VAR_UINT.
    Returns (keys, key_offs, vals, val_offs, n, keepalive)."""
    keys = b"".join(row_key(i) for i in range(len(rows)))
    parts = []
    vo = [0]
    total = 0
    for r in rows:
        v = b""
        for cid in sorted(r):
            x = r[cid]
            if x is None:
                v += cell_null(cid)
            elif cid in unsigned:
                v += cell_uint(cid, x)
            else:
                v += cell_int(cid, x)
        parts.append(v)
        total += len(v)
        vo.append(total)
    vals = b"".join(parts)
    ko = [19 * i for i in range(len(rows) + 1)]
    kb = (C.c_uint8 * max(len(keys), 1)).from_buffer_copy(keys or b"\0")
    vb = (C.c_uint8 * max(len(vals), 1)).from_buffer_copy(vals or b"\0")
    return (C.cast(kb, C.POINTER(C.c_uint8)), (C.c_uint64 * len(ko))(*ko),
            C.cast(vb, C.POINTER(C.c_uint8)), (C.c_uint64 * len(vo))(*vo),
            len(rows), (kb, vb))


def split_int_rows(data, n_cols):
    """datum-encoded rows of int / uint / NULL cells -> list of tuples;
    each cell is (flag, value) with value None for NULL. Var-int flags (8, 9)
    are raw cells, 3 / 4 are decoded ones."""
    rows = []
    p = 0
    while p < len(data):
        row = []
        for _ in range(n_cols):
            f = data[p]
            if f == 0:
                row.append((0, None))
                p += 1
            elif f == 3:
                u = int.from_bytes(data[p + 1:p + 9], "big") ^ (1 << 63)
                row.append((3, u - (1 << 64) if u >= (1 << 63) else u))
                p += 9
            elif f == 4:
                row.append((4, int.from_bytes(data[p + 1:p + 9], "big")))
                p += 9
            elif f in (8, 9):
                q = p + 1
                uv, sh = 0, 0
                while True:
                    b = data[q]
                    q += 1
                    uv |= (b & 0x7F) << sh
                    sh += 7
                    if not b & 0x80:
                        break
                if f == 8:
                    uv = ~(uv >> 1) if uv & 1 else uv >> 1
                row.append((f, uv))
                p = q
            else:
                raise AssertionError("unexpected datum flag %d" % f)
        rows.append(tuple(row))
    return rows
