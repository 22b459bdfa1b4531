"""The packed 16-bit row test of filter+count over 2-byte planes and the
engine's reused event pair (narrow_planes.hip k_plane_fcs and
k_plane_fcn<uint16_t>, copr_engine.cpp).

An iteration of a block (256 lanes x 4 vectors x 8 rows = 8192 rows, for the
high halves of a split plane and for a 2-byte plane alike) whose every row is
inside the plane counts its rows packed, two per instruction; the iteration
with the plane's last vector keeps the per-row loop. The cases here sit on
that boundary and on the rule that sends a wave from the packed count to the
per-row classification. Every request runs the four ways of
test_narrow_planes.py (default / COPR_NO_NARROW=1 / COPR_NO_PLANES=1 /
oracle, launch counts asserted) and, over a split plane, a fifth time under
COPR_SPLIT_ALL_LO=1 (test_split_planes.five_ways).
"""
import pytest

import tikv_amd
from tikv_amd import _ffi as F

from test_topn_stream import cell_int
from test_dev_chunk import region_bytes
from test_col_planes import _oracle, count_req, env
from test_narrow_planes import four_ways, open_region
from test_split_planes import five_ways

SIGS = (F.SIG_LT_INT, F.SIG_LE_INT, F.SIG_GT_INT, F.SIG_GE_INT,
        F.SIG_EQ_INT, F.SIG_NE_INT)
COLS1 = [tikv_amd.Col(1)]
# the last vector in each of a lane's four slots (2048 vectors = 256 lanes x
# 8 rows apart), one row either side of a full iteration, two iterations and
# a row; with the grid capped, the row past a grid-stride step
ROW_COUNTS = [(1, None), (7, None), (8, None), (9, None), (2047, None),
              (2048, None), (2049, None), (8191, None), (8192, None),
              (8193, None), (16385, None), (8193, "1"), (8193, "2")]


def cmp(sig, c):
    return tikv_amd.cmp_col_const(0, sig, c)


def null_cmp(sig):
    return tikv_amd.Expr().col(0).const_null().func(sig, 2)


_RAW = {}


def cached(key, make):
    if key not in _RAW:
        _RAW[key] = region_bytes([cell_int(1, v) for v in make()])
    return _RAW[key]


# ---- split planes: row counts ------------------------------------------
CUT = 0x12345678             # the first and the last row sit in its bucket


def split_vals(n):
    """rows spread over 3e9; row 0 is 0 when there is room for it, the first
    row of the last vector and the last row sit in the bucket CUT cuts, on
    either side of it"""
    vals = [(i * 1000003) % 3000000000 for i in range(n)]
    vals[0] = 0
    vals[-1] = CUT
    if n > 2:
        vals[1] = CUT - 1
        vals[(n - 1) // 8 * 8] = CUT + 1 if (n - 1) % 8 else CUT
    return vals


@pytest.mark.gpu
@pytest.mark.parametrize("n,grid", ROW_COUNTS)
def test_split_row_counts(engine, n, grid):
    """the boundary between packed iterations and the per-row tail, plain
    and with every live row sent through phase two (COPR_SPLIT_ALL_LO=1)"""
    raw = cached(("split", n), lambda: split_vals(n))
    rgn = open_region(engine, raw)
    try:
        for sig, c in ((F.SIG_LT_INT, CUT + 1), (F.SIG_LT_INT, CUT),
                       (F.SIG_GE_INT, CUT), (F.SIG_NE_INT, CUT)):
            res, _, _ = five_ways(engine, count_req(COLS1, cmp(sig, c)),
                                  [rgn], raw, grid=grid,
                                  split=0 if n == 1 else None)
            assert res[0] == "ok", (sig, c)
    finally:
        rgn.close()


# ---- split planes: constants -------------------------------------------
N_CONST = 8192 + 77          # one packed iteration and a tail


def const_vals(top, consts):
    vals = [0, top] + [(i * 7919 * 65521) % (top + 1)
                       for i in range(N_CONST - 2 - 3 * len(consts))]
    for c in consts:
        vals += [min(max(c - 1, 0), top), min(max(c, 0), top),
                 min(max(c + 1, 0), top)]
    return vals


@pytest.mark.gpu
@pytest.mark.parametrize("top", [0x2FFFF, 0x7FFFFFF0])
def test_split_constants(engine, top):
    """a plane with a range just over 2^16 and one near 2^31. Constants whose
    folded bounds fall on and one off a bucket boundary (low halves 0, 1,
    0xFFFE, 0xFFFF) under all six comparers; EQ and NE give an interval
    inside one bucket (the sure interval empty without all_lo); constants
    below and above the plane; the NULL constant."""
    mid = (top >> 17) << 16
    consts = [mid, mid + 1, mid + 0xFFFE, mid + 0xFFFF, mid + 0x8000,
              0x10000, 0xFFFF]
    raw = cached(("const", top), lambda: const_vals(top, consts))
    rgn = open_region(engine, raw)
    try:
        for sig in SIGS:
            for c in consts + [-1, -5, top + 1, top + 70000]:
                res, _, _ = five_ways(engine, count_req(COLS1, cmp(sig, c)),
                                      [rgn], raw)
                assert res[0] == "ok", (sig, c)
            res, _, _ = five_ways(engine, count_req(COLS1, null_cmp(sig)),
                                  [rgn], raw)
            assert res[0] == "ok", sig
    finally:
        rgn.close()


# ---- split planes: open rows dense and sparse --------------------------
@pytest.mark.gpu
def test_dense_open_rows(engine):
    """nearly every row in the bucket the constant cuts: more than 16 lanes
    of every wave hold an open row, in the packed iterations and in the
    tail"""
    n = 2 * 8192 + 13
    vals = [0, 0x7FFF0000] + [0x40000000 + (i * 7919) % 0x10000
                              for i in range(n - 2)]
    raw = cached("dense", lambda: vals)
    rgn = open_region(engine, raw)
    try:
        for sig, c in ((F.SIG_LT_INT, 0x40008000), (F.SIG_GE_INT, 0x40000001),
                       (F.SIG_EQ_INT, 0x40000000 + 7919),
                       (F.SIG_NE_INT, 0x40000000 + 7919)):
            res, _, _ = five_ways(engine, count_req(COLS1, cmp(sig, c)),
                                  [rgn], raw)
            assert res[0] == "ok", (sig, c)
    finally:
        rgn.close()


N_SPARSE = 8192 + 21         # the last vector holds 5 rows
SPARSE_AT = {"first vector": 3, "middle vector": 8 * 517 + 6,
             "last partial vector": N_SPARSE - 2}


@pytest.mark.gpu
@pytest.mark.parametrize("where", sorted(SPARSE_AT))
@pytest.mark.parametrize("below", [True, False])
def test_one_open_row(engine, where, below):
    """exactly one row of the region in the bucket the constant cuts, below
    the constant or above it: one lane of one wave leaves the packed count
    (or, in the tail, flags one row), every other row is far away"""
    at = SPARSE_AT[where]
    cut = 0x40008000

    def vals():
        v = [(0x10000000 if i % 2 else 0x70000000) + i
             for i in range(N_SPARSE)]
        v[0] = 0
        v[at] = cut - 5 if below else cut + 5
        return v

    raw = cached(("sparse", where, below), vals)
    rgn = open_region(engine, raw)
    try:
        for sig in (F.SIG_LT_INT, F.SIG_GE_INT):
            res, _, _ = five_ways(engine, count_req(COLS1, cmp(sig, cut)),
                                  [rgn], raw)
            assert res[0] == "ok", sig
    finally:
        rgn.close()


# ---- 2-byte planes -----------------------------------------------------
BASE2, NMAX2 = -25000, 0xFFFF


def two_byte_vals(n):
    vals = [BASE2 + (i * 131) % (NMAX2 + 1) for i in range(n)]
    vals[0] = BASE2
    vals[-1] = BASE2 + NMAX2 if n > 1 else BASE2
    return vals


@pytest.mark.gpu
@pytest.mark.parametrize("n,grid", ROW_COUNTS)
def test_two_byte_row_counts(engine, n, grid):
    """k_plane_fcn<uint16_t> on the same boundary, all six comparers against
    constants at 0, nmax and nmax + 1 above the plane's minimum, one inside
    and one below; n = 1 has a range of 0 and comes out one byte wide"""
    raw = cached(("w2", n), lambda: two_byte_vals(n))
    rgn = open_region(engine, raw)
    nmax = NMAX2 if n > 1 else 0
    try:
        for sig in SIGS:
            for c in (BASE2, BASE2 + nmax, BASE2 + nmax + 1, BASE2 + 131 * 7,
                      BASE2 - 1):
                res, launches, _ = four_ways(
                    engine, count_req(COLS1, cmp(sig, c)), [rgn], raw,
                    grid=grid)
                assert res[0] == "ok" and launches == 1, (sig, c)
    finally:
        rgn.close()


# ---- two regions, the same request twice, the reused events ------------
@pytest.mark.gpu
def test_two_regions_twice_timed(engine):
    """a split region and a 2-byte region, each with packed iterations, in
    one request on the one-dispatch path, run twice in a row: the count
    words reset themselves and the event pair is reused, so both runs give
    the oracle's bytes and a kernel time"""
    vals_a = split_vals(8193)
    vals_b = two_byte_vals(8200)
    raw_a = region_bytes([cell_int(1, v) for v in vals_a])
    raw_b = region_bytes([cell_int(1, v) for v in vals_b])
    raw_all = region_bytes([cell_int(1, v) for v in vals_a + vals_b])
    ra, rb = open_region(engine, raw_a), open_region(engine, raw_b)
    try:
        for sig, c in ((F.SIG_LT_INT, CUT), (F.SIG_GE_INT, 17)):
            req = count_req(COLS1, cmp(sig, c))
            res, launches, _ = five_ways(engine, req, [ra, rb], raw_all,
                                         split=1)
            assert res[0] == "ok" and launches == 2
            want = _oracle(req, raw_all)
            for _ in range(2):
                n0, s0 = engine.narrow_stats(), engine.split_launches()
                with env(COPR_NO_PLANES=None, COPR_NO_NARROW=None,
                         COPR_PLANE_BUDGET_MB="64", COPR_NARROW_GRID=None,
                         COPR_SPLIT_ALL_LO=None):
                    data, n, kernel_ns = engine.dag_run(req, [ra, rb])
                assert ("ok", data, n) == want
                assert engine.narrow_stats()[0] - n0[0] == 2
                assert engine.split_launches() - s0 == 1
                assert kernel_ns > 0
    finally:
        ra.close()
        rb.close()


def _timed_count(eng, raw, req):
    rgn = open_region(eng, raw)
    try:
        n0 = eng.narrow_stats()
        with env(COPR_NO_PLANES=None, COPR_NO_NARROW=None,
                 COPR_PLANE_BUDGET_MB="64", COPR_NARROW_GRID=None,
                 COPR_SPLIT_ALL_LO=None):
            data, n, kernel_ns = eng.dag_run(req, [rgn])
        assert eng.narrow_stats()[0] - n0[0] == 1
        return ("ok", data, n), kernel_ns
    finally:
        rgn.close()


@pytest.mark.gpu
def test_event_pair_lives_with_the_engine():
    """the pair is created by an engine's first request, whatever kind that
    is, and goes with the engine: a fresh engine's first filter+count is
    timed; so is one on an engine whose first requests were a hash
    aggregation and a TopN; after close() a new engine works the same"""
    raw = cached(("split", 8193), lambda: split_vals(8193))
    req = count_req(COLS1, cmp(F.SIG_LT_INT, CUT))
    want = _oracle(req, raw)

    eng = tikv_amd.Engine(0)
    try:
        res, kernel_ns = _timed_count(eng, raw, req)
        assert res == want and kernel_ns > 0
    finally:
        eng.close()

    eng = tikv_amd.Engine(0)
    try:
        small = cached(("w2", 2049), lambda: two_byte_vals(2049))
        rgn = open_region(eng, small)
        try:
            hreq = (tikv_amd.DagSelect(COLS1)
                    .hash_agg([tikv_amd.count_star()],
                              tikv_amd.Expr().col(0)).build())
            _, n, _ = eng.dag_run(hreq, [rgn])
            assert n == _oracle(hreq, small)[2] > 0
            treq = (tikv_amd.DagSelect(COLS1)
                    .topn(tikv_amd.Expr().col(0), 5).build())
            data, n, _ = eng.dag_run(treq, [rgn])
            assert ("ok", data, n) == _oracle(treq, small)
        finally:
            rgn.close()
        for _ in range(2):
            res, kernel_ns = _timed_count(eng, raw, req)
            assert res == want and kernel_ns > 0
    finally:
        eng.close()
