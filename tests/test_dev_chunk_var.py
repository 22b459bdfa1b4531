"""Device TypeChunk encoder for bytes and decimal output columns
(chunk_var.hip dev_chunk_encode_var).

Every case runs the request three ways (device, COPR_DEV_CHUNK=0 host
re-encode, oracle) and compares the bytes; Engine.dev_chunk_runs() must rise
by exactly one over the pair of engine runs (the device run; the forced-host
run can never count), or by none where the request has to fall back."""
import pytest

import tikv_amd
from tikv_amd import _ffi as F

import test_topn_stream as T
import test_wide_decimal as WD
from test_dev_chunk import region_bytes, run_three_ways
from test_oracle_exec import idx_key, make_region, v2_row
from test_topn_stream import cell_int, cell_null, cell_real, var_bytes_cell

TILE = 15856                      # COPR_CHUNK_TILE_BYTES
VARCHAR, DEC = F.TP_VARCHAR, F.TP_NEWDECIMAL
LENS = [0, 1, 15, 16, 17, 255]


def payload(i):
    n = {40: TILE + 1, 200: 3 * TILE + 5}.get(i, LENS[i % 6])
    return bytes((i * 7 + k) & 0xFF for k in range(n))


def dec_datums():
    """(prec, frac) from the issue's list, both signs; zeros; a negative
    zero; a leading partial word and a leading full word that are zero."""
    vals = [(7, 0), (123456789, 0), (1234567890, 2), (10**17 + 5, 9),
            (10**19 + 7, 10), (10**37 + 3, 0), (10**64 + 9, 30)]
    out = [WD.enc_decimal(s * v, f) for v, f in vals for s in (1, -1)]
    out += [WD.enc_decimal(0, 0), WD.enc_decimal(0, 2)]
    z = bytearray(WD.enc_decimal(0, 2))
    out.append(bytes(z[:3]) + bytes(b ^ 0xFF for b in z[3:]))
    w = (123456789).to_bytes(4, "big")
    out.append(bytes([6, 11, 0, 0x80]) + w)
    out.append(bytes([6, 18, 0, 0x80, 0, 0, 0]) + w)
    return out


def bytes_case():
    """col2: every length class, two payloads beyond the tile, NULLs; col3
    missing with a NULL default, col4 missing with a bytes default, col5 NULL
    in the whole first chunk (32 rows), col6 never NULL (no bitmap)."""
    rows = [{1: i, 2: None if i % 7 == 3 else payload(i),
             5: None if i < 32 else b"r%d" % i, 6: b"k" * (i % 5)}
            for i in range(300)]
    cols = [tikv_amd.Col(1), tikv_amd.Col(2, tp=VARCHAR),
            tikv_amd.Col(3, tp=VARCHAR, default_val=b"\x00"),
            tikv_amd.Col(4, tp=0xFC,                # BLOB
                         default_val=b"\x02" + T.var_i64(5) + b"dflt!"),
            tikv_amd.Col(5, tp=VARCHAR), tikv_amd.Col(6, tp=VARCHAR)]
    want = [(r[1], r[2], None, b"dflt!", r[5], r[6]) for r in rows]
    req = tikv_amd.DagSelect(cols).chunked().build()
    return req, T.region_of_mixed(rows), 1, ("i64",) + ("bytes",) * 5, want


def decimal_case():
    ds = dec_datums()
    rows = []
    for i in range(150):
        v = cell_int(1, i)
        v += cell_null(2) if i % 11 == 5 else WD.cell(2, ds[i % len(ds)])
        rows.append(v)
    cols = [tikv_amd.Col(1), tikv_amd.Col(2, tp=DEC, decimal=30),
            tikv_amd.Col(3, tp=DEC, decimal=2,
                         default_val=WD.enc_decimal(-31415, 2))]
    return tikv_amd.DagSelect(cols).chunked().build(), region_bytes(rows), 1


def mixed_rows(n):
    ds = dec_datums()
    rows = []
    for i in range(n):
        v = cell_int(1, (i * 37) % 100 - 50) + cell_real(2, i * 0.25 - 9)
        if i % 4:
            v += cell_int(3, i * 7)
        v += WD.cell(4, ds[i % len(ds)])
        v += cell_null(5) if i % 9 == 0 else var_bytes_cell(5, payload(i % 30))
        rows.append(v)
    return region_bytes(rows)


def mixed_req(shape):
    cols = [tikv_amd.Col(1), tikv_amd.Col(2, tp=F.TP_DOUBLE),
            tikv_amd.Col(3, flag=F.FLAG_UNSIGNED), tikv_amd.Col(4, tp=DEC),
            tikv_amd.Col(5, tp=VARCHAR), tikv_amd.Col(-1, pk_handle=True)]
    q = tikv_amd.DagSelect(cols).where(
        tikv_amd.cmp_col_const(0, F.SIG_GT_INT, -40))
    return shape(q).chunked().build()


def v2_case():
    """row-v2 and v1 rows in one region. v2_row stores an int in 1/2/4/8
    bytes, so the v2 bytes and decimal cells are 4- and 8-byte ones."""
    as_int = lambda b: int.from_bytes(b, "little")
    d4 = WD.enc_decimal(-123, 0)[1:]            # [3][0] + 2 bytes
    d8 = WD.enc_decimal(987654321042, 3)[1:]    # [12][3] + 4 + 2 bytes
    assert len(d4) == 4 and len(d8) == 8
    rows = []
    for i in range(70):
        if i % 2:
            rows.append(cell_int(1, i) + var_bytes_cell(2, payload(i)) +
                        WD.cell(3, WD.enc_decimal(i - 30, 1)))
        else:
            rows.append(bytes(v2_row([
                (1, i), (2, as_int(b"ab%c%c" % (65 + i % 26, 97 + i % 26))),
                (3, as_int(d8 if i % 4 else d4))])))
    cols = [tikv_amd.Col(1), tikv_amd.Col(2, tp=VARCHAR),
            tikv_amd.Col(3, tp=DEC)]
    return tikv_amd.DagSelect(cols).chunked().build(), region_bytes(rows), 1


def index_bytes_case():
    """an index key carries memcomparable (flag 1) bytes: host path"""
    def memcmp(b):
        out = b""
        for g in range(0, len(b) + 1, 8):
            part = b[g:g + 8]
            out += part.ljust(8, b"\0") + bytes([0xFF - (8 - len(part))])
        return out
    rows = [(idx_key(1, 1, [b"\x01" + memcmp(b"key-%03d" % i * (i % 3))],
                     handle=i), b"0") for i in range(60)]
    kb, ko, vb, vo, n = make_region(rows)
    raw = (T.C.cast(kb, T.C.POINTER(T.C.c_uint8)), ko,
           T.C.cast(vb, T.C.POINTER(T.C.c_uint8)), vo, n, (kb, vb))
    cols = [tikv_amd.Col(1, tp=VARCHAR), tikv_amd.Col(-1, pk_handle=True)]
    return tikv_amd.DagSelect(cols, index=True).chunked().build(), raw, 0


def int_in_decimal_case():
    """one row's decimal column holds an int datum: host path"""
    rows = [cell_int(1, i) + (cell_int(2, 5) if i == 77 else
                              WD.cell(2, WD.enc_decimal(i * 3, 1)))
            for i in range(100)]
    cols = [tikv_amd.Col(1), tikv_amd.Col(2, tp=DEC)]
    return tikv_amd.DagSelect(cols).chunked().build(), region_bytes(rows), 0


def generated_case():
    g = tikv_amd.GenRegion(config_index=2, n_rows=40000, table_id=5)
    cols = [tikv_amd.Col(1), tikv_amd.Col(2, tp=DEC, decimal=2),
            tikv_amd.Col(3, tp=VARCHAR)]
    req = (tikv_amd.DagSelect(cols).where(
        tikv_amd.cmp_col_const(0, F.SIG_LT_INT, 32)).chunked().build())
    return req, (g.keys, g.key_offs, g.vals, g.val_offs, g.n_kv, g), 1


CASES = {
    "bytes": bytes_case,
    "decimal": decimal_case,
    "mixed": lambda: (mixed_req(lambda q: q), mixed_rows(300), 1),
    "mixed_limit": lambda: (mixed_req(lambda q: q.limit(41)),
                            mixed_rows(300), 1),
    "mixed_paging": lambda: (mixed_req(lambda q: q.paging(25)),
                             mixed_rows(300), 1),
    "v2_and_v1": v2_case,
    "index_bytes_key": index_bytes_case,
    "int_in_decimal": int_in_decimal_case,
    "generated": generated_case,
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_dev_chunk_var(engine, name):
    req, raw, delta, *decode = CASES[name]()
    before = engine.dev_chunk_runs()
    try:
        data, nrows = run_three_ways(engine, req, raw)
    finally:
        if hasattr(raw[5], "close"):
            raw[5].close()                  # the generated region
    assert engine.dev_chunk_runs() - before == delta
    assert nrows > 0 and data
    if decode:
        assert T.decode_chunks(data, decode[0]) == decode[1]
