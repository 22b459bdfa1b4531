"""GROUP BY with 5, 6 and 7 aggregates (kernels.hip d_row_accumulate,
d_hash_row_slot, d_hash_update, d_hash_lds_flush).

Such plans run on the kernel instances unrolled to COPR_MAX_AGGS = 8 while
every accumulator array (global table, reserved groups, ext limbs, the
per-block LDS table) is laid out with the plan's n_aggs, so they are the ones
that tell the two strides apart. One region serves every case: 4 096 rows,
300 distinct int keys against the 256 LDS slots (the table spills into the
global one), NULL keys, rows without the key column, INT64_MIN (the table's
EMPTY sentinel, group reserved[0]), row-v2 rows among row-v1 rows. Results
are compared exactly, as sorted per-row datum strings.
"""
import pytest

import tikv_amd
from tikv_amd import _ffi as F

from test_topn_stream import cell_int, cell_null, cell_real
from test_dev_chunk import region_bytes
from test_col_planes import env, _run, _oracle
from test_wide_decimal import enc_decimal
from test_hash_planes import (I64_MIN, _norm, cell_dec, one_region, v2_cells)

N = 4096
K = 300
MIN_KEY_ROWS = (7, 1207, 2407)      # i // K even: cells of the target frac


def row(i, wide, v2_every):
    """columns: 1 key, 2 int (NULL every 7th), 3 int (absent every 5th),
    4 decimal(., 2) of frac 2 or 1 (NULL every 11th), 5 real (row-v1 only).
    wide: every tenth decimal is a 30-digit value."""
    frac = 1 if (i // K) % 2 else 2
    dec = (i * 7919) % 2_000_003 - 1_000_000
    key = i % K - K // 2
    if i % v2_every == 5:
        cells = [(1, key), (2, i * 11 - 500)]
        if i % 5:
            cells.append((3, (i * 13) % 64 - 32))
        cells.append((4, enc_decimal(dec, frac)[1:]))
        return v2_cells(cells)
    v = b""
    if i in MIN_KEY_ROWS:
        v += cell_int(1, I64_MIN)
    elif i % 97 == 0:
        v += cell_null(1)
    elif i % 101 != 1:                    # else: key column absent
        v += cell_int(1, key)
    v += cell_null(2) if i % 7 == 0 else cell_int(2, i * 11 - 500)
    if i % 5:
        v += cell_int(3, (i * 13) % 64 - 32)
    if i % 11 == 3:
        v += cell_null(4)
    elif wide and i % 10 == 3:
        v += cell_dec(4, (10**29 + i * 10**20) * (1 if i % 20 == 3 else -1), 2)
    else:
        v += cell_dec(4, dec, frac)
    return v + cell_real(5, (i % 41) * 0.75 - 12.5)


_RAW = {}


def raw_rows(wide):
    """built once per shape and shared. The planes keep a column while at
    most 1/8 of its rows need the row bytes: row-v2 rows on every 16th row,
    or on every 64th beside the wide decimals on every tenth."""
    if wide not in _RAW:
        _RAW[wide] = region_bytes([row(i, wide, 64 if wide else 16)
                                   for i in range(N)])
    return _RAW[wide]


def cols():
    return [tikv_amd.Col(1), tikv_amd.Col(2), tikv_amd.Col(3),
            tikv_amd.Col(4, tp=F.TP_NEWDECIMAL, decimal=2),
            tikv_amd.Col(5, tp=F.TP_DOUBLE)]


def plane_aggs(n):
    """kinds the plane path serves, over columns 2, 3 and 4. Six kinds do not
    fit five aggregates: count(col) joins at six."""
    return [tikv_amd.count_star(), tikv_amd.sum_col(3, decimal=2),
            tikv_amd.min_col(1), tikv_amd.max_col(2), tikv_amd.sum_col(1),
            tikv_amd.count_col(2), tikv_amd.count_col(1)][:n]


def scan_aggs(n):
    """a bit-xor and real max/min: the plane path refuses the plan"""
    return [tikv_amd.count_star(), tikv_amd.bit_op(F.AGG_BIT_XOR, 1),
            tikv_amd.max_col(4, tp=F.TP_DOUBLE),
            tikv_amd.sum_col(3, decimal=2), tikv_amd.min_col(2),
            tikv_amd.min_col(4, tp=F.TP_DOUBLE), tikv_amd.sum_col(1)][:n]


def req_of(aggs):
    return (tikv_amd.DagSelect(cols())
            .hash_agg(aggs, tikv_amd.Expr().col(0)).build())


N_GROUPS = K + 2                    # + the NULL group and INT64_MIN


@pytest.mark.gpu
@pytest.mark.parametrize("n_aggs", [5, 6, 7])
def test_plane_kinds(engine, n_aggs):
    """planes == scan kernels == oracle"""
    res, _ = one_region(engine, req_of(plane_aggs(n_aggs)), raw_rows(False),
                        n_aggs + 1)
    assert res[0] == "ok" and res[2] == N_GROUPS


@pytest.mark.gpu
def test_plane_kinds_wide_decimals(engine):
    """every tenth decimal has 30 digits: the row takes a global slot
    whatever the LDS table holds, and adds in 256 bits into ext limbs laid
    out with stride n_aggs"""
    res, _ = one_region(engine, req_of(plane_aggs(5)), raw_rows(True), 6)
    assert res[0] == "ok" and res[2] == N_GROUPS


@pytest.mark.gpu
@pytest.mark.parametrize("n_aggs", [5, 7])
def test_scan_only_kinds(engine, n_aggs):
    """scan kernels == oracle, on the default leg as on the COPR_NO_PLANES=1
    leg: the plane path must not take the plan"""
    raw = raw_rows(False)
    req = req_of(scan_aggs(n_aggs))
    want = _norm(_oracle(req, raw), n_aggs + 1)
    assert want[0] == "ok" and want[2] == N_GROUPS
    rgn = engine.region_raw(*raw[:5])
    try:
        h0 = engine.hash_plane_launches()
        with env(COPR_NO_PLANES=None, COPR_PLANE_BUDGET_MB="64"):
            r_dflt = _norm(_run(engine, req, [rgn]), n_aggs + 1)
        with env(COPR_NO_PLANES="1", COPR_PLANE_BUDGET_MB="64"):
            r_scan = _norm(_run(engine, req, [rgn]), n_aggs + 1)
        assert engine.hash_plane_launches() == h0
    finally:
        rgn.close()
    assert r_scan == want
    assert r_dflt == want


@pytest.mark.gpu
@pytest.mark.parametrize("n_aggs", [5, 7])
def test_scan_only_kinds_no_pipe(engine, n_aggs):
    """COPR_NO_PLANES=1 COPR_NO_PIPE=1: the single-buffer k_scan_agg<.., true>,
    the kernel that serves rows too long for the pipeline, == oracle"""
    raw = raw_rows(False)
    req = req_of(scan_aggs(n_aggs))
    want = _norm(_oracle(req, raw), n_aggs + 1)
    assert want[0] == "ok" and want[2] == N_GROUPS
    rgn = engine.region_raw(*raw[:5])
    try:
        h0 = engine.hash_plane_launches()
        with env(COPR_NO_PLANES="1", COPR_NO_PIPE="1",
                 COPR_PLANE_BUDGET_MB="64"):
            r_nopipe = _norm(_run(engine, req, [rgn]), n_aggs + 1)
        assert engine.hash_plane_launches() == h0
    finally:
        rgn.close()
    assert r_nopipe == want
