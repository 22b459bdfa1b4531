"""Split narrow planes (narrow_planes.hip k_plane_split /
k_plane_fcs).

A narrow plane of width 4 is stored as a plane of high and a plane of low
16-bit halves; filter+count streams the high halves and fetches low halves
only for rows in the one or two buckets the constant cuts. Every case runs
one request the four ways of test_narrow_planes.py (default /
COPR_NO_NARROW=1 / COPR_NO_PLANES=1 / oracle, same bytes, narrow launch
count asserted) and, where all_lo is set, a fifth time under
COPR_SPLIT_ALL_LO=1, which sends every live row through the low-half phase
and must give the same bytes.

Column values are chosen with min = 0 (or base given), so the stored
n = v - min and the buckets n >> 16 are what the case says they are.
"""
import pytest

import tikv_amd
from tikv_amd import _ffi as F

from test_topn_stream import cell_int, cell_null
from test_dev_chunk import region_bytes
from test_col_planes import _run, cell_uint, count_req, env
from test_narrow_planes import four_ways, open_region

I_MIN, I_MAX = -(1 << 63), (1 << 63) - 1
U63 = 1 << 63
SIGS = (F.SIG_LT_INT, F.SIG_LE_INT, F.SIG_GT_INT, F.SIG_GE_INT,
        F.SIG_EQ_INT, F.SIG_NE_INT)
COLS1 = [tikv_amd.Col(1)]


def cmp(sig, c, **kw):
    return tikv_amd.cmp_col_const(0, sig, c, **kw)


def five_ways(engine, req, rgns, raw, narrow=True, grid=None, all_lo=True,
              split=None):
    """four_ways, then the default leg again under COPR_SPLIT_ALL_LO=1.
    split = how many of the narrow launches must run over a split plane, so
    take k_plane_fcs (default: all of them)."""
    s0 = engine.split_launches()
    res, launches, builds = four_ways(engine, req, rgns, raw, narrow=narrow,
                                      grid=grid)
    want_split = launches if split is None else split
    assert engine.split_launches() - s0 == want_split, \
        "split launches %d, expected %d" % (engine.split_launches() - s0,
                                            want_split)
    if all_lo:
        n0 = engine.narrow_stats()
        s1 = engine.split_launches()
        with env(COPR_NO_PLANES=None, COPR_NO_NARROW=None,
                 COPR_PLANE_BUDGET_MB="64", COPR_NARROW_GRID=grid,
                 COPR_SPLIT_ALL_LO="1"):
            r_all = _run(engine, req, rgns)
        assert engine.narrow_stats()[0] - n0[0] == launches
        assert engine.split_launches() - s1 == want_split
        assert r_all == res
    return res, launches, builds


# ---- row counts and grid stride ----------------------------------------
LAST = 0x12345678            # the last live row: bucket 0x1234, mid-bucket


def edge_rows(n):
    """row 0 holds 0 (the minimum), the last row LAST, the rest spread over
    3e9; n = 1 cannot span 32 bits and comes out at width 1"""
    vals = [(i * 1000003) % 3000000000 for i in range(n)]
    vals[0] = 0
    vals[-1] = LAST
    return region_bytes([cell_int(1, v) for v in vals])


_EDGE_RAW = {}


def edge_raw(n):
    if n not in _EDGE_RAW:
        _EDGE_RAW[n] = edge_rows(n)
    return _EDGE_RAW[n]


# the constant cuts the last row's bucket; the row is kept, then dropped
EDGE_CONDS = [(F.SIG_LT_INT, LAST + 1), (F.SIG_LT_INT, LAST),
              (F.SIG_GE_INT, LAST), (F.SIG_GE_INT, LAST + 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,grid", [(1, None), (7, None), (8, None),
                                    (9, None), (31, None), (32, None),
                                    (33, None), (8191, None), (8192, None),
                                    (8193, None), (8193, "1"), (16385, "2")])
def test_row_counts(engine, n, grid):
    """tail masking around the 8 rows of one load, the 32 of one lane and
    the 8192 of one block step (256 lanes x 4 loads x 8 rows); with the grid
    capped, one row past a grid-stride step. The last live row sits in the
    bucket the constant cuts, so a flag or a low half taken from the tail
    slack would change the count."""
    raw = edge_raw(n)
    rgn = open_region(engine, raw)
    try:
        for sig, c in EDGE_CONDS:
            # one row has a range of 0: width 1, the only plane here not split
            res, _, _ = five_ways(engine, count_req(COLS1, cmp(sig, c)),
                                  [rgn], raw, grid=grid,
                                  split=0 if n == 1 else None)
            assert res[0] == "ok", (sig, c)
    finally:
        rgn.close()


# ---- most rows ambiguous -----------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sig", SIGS)
def test_dense_ambiguity(engine, sig):
    """every row but two in buckets 1 and 2; one row at 0 and one at 0x2FFFF
    keep the width at 4. Constants inside a bucket leave about half the rows
    to the low halves; after each comparer's +-1 the folded bounds take the
    low halves 0x0000, 0x0001, 0xFFFE and 0xFFFF."""
    consts = (0x10000, 0x10001, 0x10002, 0x18000, 0x1FFFD, 0x1FFFE, 0x1FFFF,
              0x20000, 0x20001)
    vals = [0, 0x2FFFF] + [0x10000 + (i * 7919) % 0x20000 for i in range(600)]
    for c in consts:
        vals += [c - 1, c, c + 1]
    raw = region_bytes([cell_int(1, v) for v in vals])
    rgn = open_region(engine, raw)
    try:
        for c in consts:
            res, _, _ = five_ways(engine, count_req(COLS1, cmp(sig, c)),
                                  [rgn], raw)
            assert res[0] == "ok", c
    finally:
        rgn.close()


# ---- few rows ambiguous, at every position -----------------------------
@pytest.mark.gpu
def test_sparse_ambiguity_every_position(engine):
    """8193 rows; row 257 k sits in the bucket the constant cuts, on either
    side of it, the others far inside or far outside. 257 = 32 x 8 + 1, so
    the flagged rows walk through all 8 positions of a load and, 32 vectors
    apart, through the 4 unrolled loads and many lanes."""
    cut = 0x40008000

    def val(i):
        if i == 1:
            return 0
        if i % 257 == 0:
            return 0x40000000 + ((i // 257) * 0x1111) % 0x10000
        return (0x10000000 if i % 2 else 0x70000000) + i

    raw = region_bytes([cell_int(1, val(i)) for i in range(8193)])
    rgn = open_region(engine, raw)
    try:
        for sig, c in ((F.SIG_LT_INT, cut), (F.SIG_GE_INT, cut),
                       (F.SIG_EQ_INT, 0x40000000 + 3 * 0x1111),
                       (F.SIG_NE_INT, 0x40000000 + 5 * 0x1111)):
            res, _, _ = five_ways(engine, count_req(COLS1, cmp(sig, c)),
                                  [rgn], raw)
            assert res[0] == "ok", (sig, c)
    finally:
        rgn.close()


# ---- the smallest and the largest split plane --------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nmax", [0x10000, 0xFFFFFFFF])
@pytest.mark.parametrize("base", [I_MIN, I_MAX - 0xFFFFFFFF])
def test_width_limits(engine, base, nmax):
    """nmax = 0x10000 is the first range that no longer fits two bytes,
    0xFFFFFFFF the last that fits four; planes that start at INT64_MIN and
    (for the wide one) end at INT64_MAX. Constants on and beside the bottom
    and top values."""
    top = base + nmax
    vals = [base, top, base + 1, top - 1] + \
           [base + (i * 7919 * 65521) % (nmax + 1) for i in range(300)]
    raw = region_bytes([cell_int(1, v) for v in vals])
    rgn = open_region(engine, raw)
    consts = {base, base + 1, top - 1, top}
    if base > I_MIN:
        consts.add(base - 1)
    if top < I_MAX:
        consts.add(top + 1)
    try:
        first = True
        for sig in (F.SIG_LT_INT, F.SIG_GE_INT, F.SIG_EQ_INT, F.SIG_NE_INT):
            for c in sorted(consts):
                res, _, builds = five_ways(
                    engine, count_req(COLS1, cmp(sig, c)), [rgn], raw)
                assert res[0] == "ok", (sig, c)
                assert builds == (1 if first else 0)
                first = False
    finally:
        rgn.close()


# ---- unsigned ----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("lo", [U63 + 12345, 5])
def test_unsigned_reading(engine, lo):
    """uint cells spread over 3e9, all above 2^63 (negative as stored) or
    all below: min and max share a sign, so the unsigned request may use the
    split plane"""
    vals = [lo, lo + 2999999999] + \
           [lo + (i * 1000003) % 3000000000 for i in range(775)]
    raw = region_bytes([cell_uint(1, v) for v in vals])
    rgn = open_region(engine, raw)
    cols = [tikv_amd.Col(1, flag=F.FLAG_UNSIGNED)]
    mid = lo + 3 * 1000003          # a stored value
    try:
        for sig in SIGS:
            for c in (0, lo - 1, lo, mid, mid + 1, lo + 2999999999,
                      lo + 3000000000, (1 << 64) - 1):
                req = count_req(cols, cmp(sig, c, unsigned_const=True))
                res, _, _ = five_ways(engine, req, [rgn], raw)
                assert res[0] == "ok", (sig, c)
    finally:
        rgn.close()


# ---- several regions ---------------------------------------------------
def spread_rows(n, mul):
    return [cell_int(1, 0 if i == 0 else (i * mul) % 3000000000)
            for i in range(n)]


@pytest.mark.gpu
def test_two_split_regions_one_total(engine):
    """both regions take k_plane_fcs; the second launch finalizes and hands
    over the one total"""
    rows_a, rows_b = spread_rows(777, 1000003), spread_rows(1025, 7000003)
    raw_a, raw_b = region_bytes(rows_a), region_bytes(rows_b)
    raw_all = region_bytes(rows_a + rows_b)
    ra, rb = open_region(engine, raw_a), open_region(engine, raw_b)
    try:
        for sig, c in ((F.SIG_LT_INT, 1500000000), (F.SIG_GE_INT, 2000003),
                       (F.SIG_NE_INT, 0)):
            res, launches, _ = five_ways(
                engine, count_req(COLS1, cmp(sig, c)), [ra, rb], raw_all)
            assert res[0] == "ok" and launches == 2
    finally:
        ra.close()
        rb.close()


@pytest.mark.gpu
def test_split_region_beside_a_declined_one(engine):
    """region B holds one NULL row and keeps k_plane_fc; region A's split
    kernel adds into the usual accumulator through the mixed sequence"""
    rows_a = spread_rows(777, 1000003)
    rows_b = [cell_int(1, i % 50) for i in range(300)]
    rows_b[7] = cell_null(1)
    raw_a, raw_b = region_bytes(rows_a), region_bytes(rows_b)
    ra, rb = open_region(engine, raw_a), open_region(engine, raw_b)
    try:
        for order, rows in (([ra, rb], rows_a + rows_b),
                            ([rb, ra], rows_b + rows_a)):
            res, launches, _ = five_ways(
                engine, count_req(COLS1, cmp(F.SIG_LT_INT, 1000003 * 5 + 1)),
                order, region_bytes(rows), narrow=1)
            assert res[0] == "ok" and launches == 1
    finally:
        ra.close()
        rb.close()


# ---- the device words reset themselves ---------------------------------
@pytest.mark.gpu
def test_same_request_twice(engine):
    """the same request twice on one engine, plain and with every row sent
    through the low halves: the count words and the ticket are back at zero
    after each, so the counts repeat"""
    raw = edge_raw(8193)
    rgn = open_region(engine, raw)
    req = count_req(COLS1, cmp(F.SIG_LT_INT, LAST + 1))
    try:
        first, launches, _ = five_ways(engine, req, [rgn], raw)
        again, launches2, _ = five_ways(engine, req, [rgn], raw)
        assert first[0] == "ok" and first == again
        assert launches == launches2 == 1
    finally:
        rgn.close()
