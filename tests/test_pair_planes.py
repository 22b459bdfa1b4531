"""count(*) under two conditions over narrow planes:
k_plane_fc2 over two columns' planes, and plane_fc_and folding two conditions
on one column into the single-condition kernels. Every request runs the four
ways of test_narrow_planes.py (default / COPR_NO_NARROW=1 / COPR_NO_PLANES=1 /
oracle, same bytes, narrow launches asserted) with pair_launches,
split_launches and bucket_stats()[0] asserted. Column minima are 0 unless said
otherwise, so a stored n is the value and its bucket n >> 16.
"""
import pytest

import tikv_amd
from tikv_amd import _ffi as F

from test_topn_stream import cell_int, cell_null
from test_dev_chunk import region_bytes
from test_col_planes import cell_uint, count_req, env
from test_narrow_planes import four_ways, open_region
from test_split_planes import COLS1, LAST

LT, LE, GT, GE, EQ, NE = (F.SIG_LT_INT, F.SIG_LE_INT, F.SIG_GT_INT,
                          F.SIG_GE_INT, F.SIG_EQ_INT, F.SIG_NE_INT)
COLS2 = [tikv_amd.Col(1), tikv_amd.Col(2)]
cmp = tikv_amd.cmp_col_const
LAST2 = 0x0BADC0DE
# (multiplier, modulus, shift) of six columns: two 1-byte, two 2-byte, two split
MODS = ((37, 200, -100), (91, 251, 0), (131, 50000, -25000), (977, 60000, 0),
        (1000003, 3000000000, -1500000000), (7000003, 4000000000, 0))
COLS6 = [tikv_amd.Col(c + 1) for c in range(6)]


def ways(engine, req, raws, pair=None, bucket=0, narrow=True, grid=None, **sw):
    """four_ways over one region per raw under the switches sw; pair / bucket
    = how far pair_launches and bucket_stats()[0] must move (pair: one per
    region). A pair launch is never a split or a bucket launch."""
    rgns = [open_region(engine, region_bytes(r)) for r in raws]
    want = len(rgns) if pair is None else pair
    before = (engine.pair_launches(), engine.bucket_stats()[0])
    s0, w0 = engine.split_launches(), sum(engine.fc_wait_stats())
    try:
        with env(**sw):
            res, _, _ = four_ways(engine, req, rgns,
                                  region_bytes(sum(raws, [])), narrow=narrow,
                                  grid=grid)
    finally:
        for r in rgns:
            r.close()
    assert res[0] == "ok"
    assert (engine.pair_launches() - before[0],
            engine.bucket_stats()[0] - before[1]) == (want, bucket)
    if want:
        assert engine.split_launches() == s0
    return res, sum(engine.fc_wait_stats()) - w0


def rows2(n, mul_a=1000003, mul_b=7000003):
    """two split columns spread over 3e9, row 0 = (0, 0), the last row (LAST,
    LAST2); a single row has no range and comes out at width 1"""
    a = [(i * mul_a) % 3000000000 for i in range(n)]
    b = [(i * mul_b) % 3000000000 for i in range(n)]
    a[0] = b[0] = 0
    a[-1], b[-1] = LAST, LAST2
    return [cell_int(1, x) + cell_int(2, y) for x, y in zip(a, b)]


def six_val(c, i):
    return (i * MODS[c][0]) % MODS[c][1] + MODS[c][2]


def six_rows():
    return [b"".join(cell_int(c + 1, six_val(c, i)) for c in range(6))
            for i in range(1100)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,grid", [(1, None), (15, None), (16, None),
                                    (17, None), (31, None), (32, None),
                                    (33, None), (8191, None), (8192, None),
                                    (8193, None), (8193, "1"), (16385, "2")])
def test_row_counts(engine, n, grid):
    """around one unit (16 rows), one lane (32) and one block step (8192),
    and one row past a grid-stride step. The last live row sits in the bucket
    both constants cut and is kept, dropped by A, dropped by B: a flag or a
    low half taken from the tail slack would change the count."""
    for ca, cb in ((LAST + 1, LAST2), (LAST, LAST2), (LAST + 1, LAST2 + 1)):
        ways(engine, count_req(COLS2, cmp(0, LT, ca), cmp(1, GE, cb)),
             [rows2(n)], grid=grid)


@pytest.mark.gpu
@pytest.mark.parametrize("a,b", [(0, 1), (0, 2), (0, 4), (2, 3), (2, 4),
                                 (4, 5), (1, 0), (2, 0), (4, 0), (3, 2),
                                 (4, 2), (5, 4)])
def test_width_pairs(engine, a, b):
    """the six width pairs, narrower first and wider first; the constants are
    stored values, so EQ and NE hit a row"""
    for sa, sb in ((LT, GE), (NE, LT), (GT, NE), (NE, NE), (EQ, LE)):
        ways(engine, count_req(COLS6, cmp(a, sa, six_val(a, 5)),
                               cmp(b, sb, six_val(b, 7))), [six_rows()])


def prune_side(i, every, bucket):
    """every `every`-th row in `bucket`, which the constant cuts (open); the
    rest far inside or far outside"""
    if i == 1:
        return 0
    if i % every == 0:
        return (bucket << 16) + (i * 0x1111) % 0x10000
    return (0x10000000 if (i // every) % 2 else 0x70000000) + i


@pytest.mark.gpu
def test_cross_pruning(engine):
    """rows open on A that B rejects or keeps, the reverse, rows open on both;
    NE on an open row; a NULL constant (B never); each again with every row
    through the low halves"""
    rows = [cell_int(1, prune_side(i, 4, 0x4000)) +
            cell_int(2, prune_side(i, 3, 0x2000)) for i in range(2100)]
    cut_a, cut_b = 0x40008000, 0x20008000
    null_b = tikv_amd.Expr().col(1).const_null().func(LT, 2)
    for conds in ((cmp(0, LT, cut_a), cmp(1, GE, cut_b)),
                  (cmp(0, GE, cut_a), cmp(1, LT, cut_b)),
                  (cmp(0, NE, prune_side(8, 4, 0x4000)), cmp(1, LT, cut_b)),
                  (cmp(0, LT, cut_a), null_b)):
        req = count_req(COLS2, *conds)
        res = ways(engine, req, [rows])[0]
        assert ways(engine, req, [rows], COPR_SPLIT_ALL_LO="1")[0] == res


@pytest.mark.gpu
def test_unsigned_straddle_stays_wide(engine):
    """uint cells 2^64 - 50 .. 2^64 - 1 and 0 .. 49: a 1-byte plane from -50
    to 49 as stored, where signed and unsigned order disagree, so
    narrow_fc_fold refuses the unsigned request"""
    rows = [cell_uint(1, (i % 100 - 50) % (1 << 64)) + cell_int(2, i % 77)
            for i in range(500)]
    cols = [tikv_amd.Col(1, flag=F.FLAG_UNSIGNED), tikv_amd.Col(2)]
    for c in (10, 1 << 63, (1 << 64) - 10):
        ways(engine, count_req(cols, cmp(0, LT, c, unsigned_const=True),
                               cmp(1, GE, 30)), [rows], pair=0, narrow=False)


@pytest.mark.gpu
def test_regions(engine):
    """three qualifying regions: one one-dispatch request, three pair
    launches. A NULL in one region's second column leaves it without a narrow
    plane: two pair launches join k_plane_agg's count, nothing is polled."""
    rows = [rows2(777), rows2(1025, 3000017, 5000011), rows2(300)]
    odd = rows2(300)
    odd[7] = cell_int(1, 5) + cell_null(2)
    req = count_req(COLS2, cmp(0, LT, 1500000000), cmp(1, GE, 1000000000))
    assert ways(engine, req, rows)[1] == 1
    assert ways(engine, req, rows[:2] + [odd], pair=2, narrow=2)[1] == 0


def edge_col(n):
    """test_split_planes' one-column region as rows"""
    vals = [(i * 1000003) % 3000000000 for i in range(n)]
    vals[0], vals[-1] = 0, LAST
    return [cell_int(1, v) for v in vals]


@pytest.mark.gpu
@pytest.mark.parametrize("a,b,narrow", [
    ((GE, LAST - 5), (LT, LAST + 5), True),              # cuts in one bucket
    ((GE, 0x1234F000), (LT, 0x12351000), True),          # adjacent buckets
    ((GE, 1000000000), (LT, 2000000000), True),          # far apart
    ((GE, 2000000000), (LT, 1000000000), True),          # empty intersection
    ((GE, LAST), (NE, LAST), True),                      # NE on an end folds
    ((GE, 0), (NE, LAST), False)])                       # NE inside: wide
def test_between_over_bucket_index(engine, a, b, narrow):
    ways(engine, count_req(COLS1, cmp(0, *a), cmp(0, *b)), [edge_col(8193)],
         pair=0, bucket=1 if narrow else 0, narrow=narrow,
         COPR_BUCKET_MIN_ROWS="0")


@pytest.mark.gpu
@pytest.mark.parametrize("col", [0, 2])
def test_between_over_one_and_two_bytes(engine, col):
    lo, hi = sorted((six_val(col, 5), six_val(col, 7)))
    for a, b, narrow in (((GE, lo), (LT, hi), True), ((LT, lo), (GE, hi), True),
                         ((LE, hi), (NE, hi), True), ((LE, hi), (NE, lo), False)):
        ways(engine, count_req(COLS6, cmp(col, *a), cmp(col, *b)),
             [six_rows()], pair=0, narrow=narrow)


@pytest.mark.gpu
def test_no_pair_switch(engine):
    req = count_req(COLS2, cmp(0, LT, LAST + 1), cmp(1, GE, LAST2))
    res = ways(engine, req, [rows2(8193)])[0]
    assert ways(engine, req, [rows2(8193)], pair=0, narrow=False,
                COPR_NO_PAIR="1")[0] == res
