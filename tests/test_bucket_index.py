"""The bucket index of a split plane (narrow_planes.hip
bucket_index_build / k_plane_fcb, plane_fold.h bucket_fc_fold).

A split plane of at least COPR_BUCKET_MIN_ROWS rows carries its low halves
grouped by bucket h = n >> 16 and the 65 537 group offsets; a range
filter+count then takes two offsets on the host and one k_plane_fcb launch
over the one or two buckets the constant cuts. Every case here runs with
COPR_BUCKET_MIN_ROWS=0 and COPR_PLANE_BUDGET_MB=64 unless it says otherwise,
and compares the answer byte for byte with the same request under
COPR_NO_BUCKETS=1 (k_plane_fcs), under COPR_NO_PLANES=1 (the row scan) and
with the oracle. bucket_stats must move by exactly the expected launches and
builds, split_launches by the launches that kept k_plane_fcs, and
fc_wait_stats by one.

Column values are chosen with min = 0, so the stored n = v - min and the
buckets n >> 16 are what the case says they are.
"""
import pytest

from tikv_amd import _ffi as F

from test_topn_stream import cell_int
from test_dev_chunk import region_bytes
from test_col_planes import _oracle, _run, count_req, env
from test_narrow_planes import open_region
from test_split_planes import COLS1, EDGE_CONDS, LAST, SIGS, cmp, edge_raw


def ways(engine, req, rgns, raw, bucket=None, builds=0, split=0, grid=None,
         min_rows="0", budget="64", poll=None, all_lo=None):
    """The default leg, then COPR_NO_BUCKETS=1, COPR_NO_PLANES=1 and the
    oracle. bucket / split = the regions that must take k_plane_fcb /
    k_plane_fcs on the default leg (bucket defaults to all, every region is
    on a narrow plane), builds = the indexes it must build."""
    want = len(rgns) if bucket is None else bucket
    b0, s0 = engine.bucket_stats(), engine.split_launches()
    n0, w0 = engine.narrow_stats(), engine.fc_wait_stats()
    with env(COPR_NO_PLANES=None, COPR_NO_NARROW=None, COPR_NO_BUCKETS=None,
             COPR_BUCKET_MIN_ROWS=min_rows, COPR_PLANE_BUDGET_MB=budget,
             COPR_NARROW_GRID=grid, COPR_FC_POLL_US=poll,
             COPR_SPLIT_ALL_LO=all_lo):
        r_idx = _run(engine, req, rgns)
    b1, s1 = engine.bucket_stats(), engine.split_launches()
    n1, w1 = engine.narrow_stats(), engine.fc_wait_stats()
    assert (b1[0] - b0[0], b1[1] - b0[1]) == (want, builds), (b0, b1)
    assert s1 - s0 == split, "split launches %d, expected %d" % (s1 - s0, split)
    assert n1[0] - n0[0] == len(rgns), "a region left the narrow planes"
    assert sum(w1) - sum(w0) == 1, (w0, w1)
    if poll == "0":
        assert w1[1] - w0[1] == 1
    with env(COPR_NO_PLANES=None, COPR_NO_NARROW=None, COPR_NO_BUCKETS="1",
             COPR_BUCKET_MIN_ROWS=min_rows, COPR_PLANE_BUDGET_MB=budget,
             COPR_NARROW_GRID=grid):
        r_scan = _run(engine, req, rgns)
    assert engine.bucket_stats() == b1, "COPR_NO_BUCKETS=1 used or built an index"
    assert engine.narrow_stats()[0] - n1[0] == len(rgns)
    with env(COPR_NO_PLANES="1", COPR_PLANE_BUDGET_MB=budget):
        r_rows = _run(engine, req, rgns)
    assert engine.bucket_stats() == b1
    assert r_idx[0] == "ok"
    assert r_idx == r_scan
    assert r_idx == r_rows
    assert r_idx == _oracle(req, raw)
    return r_idx


# ---- row counts ----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 7, 8, 9, 8193])
def test_row_counts(engine, n):
    """around the 8 rows of one load and one past a block's 8192. The last
    row sits in the bucket the constant cuts and, sorted by bucket, at or near
    the end of the grouped low halves, so a slack byte read as a low half
    would change the count. The whole list runs twice: the second pass finds
    the index built and the device words as the first left them."""
    raw = edge_raw(n)
    rgn = open_region(engine, raw)
    try:
        first = []
        for rep in range(2):
            res = []
            for i, (sig, c) in enumerate(EDGE_CONDS):
                res.append(ways(engine, count_req(COLS1, cmp(sig, c)), [rgn],
                                raw, builds=1 if rep == 0 and i == 0 else 0))
            first = first or res
            assert res == first
    finally:
        rgn.close()


# ---- dense edge buckets ----------------------------------------------------
DENSE_TOP = 0x2F000


def dense_vals():
    """20 000 rows in bucket 1 and 8192 + 1 in bucket 2, one row at 0 and one
    at DENSE_TOP: the maximum's low half is not 0xFFFF, so c < v cuts two
    buckets. Bucket 1 is long enough for a block step wholly inside it (the
    packed count), bucket 2 for a second stride and the clamped vector."""
    vals = [0, DENSE_TOP]
    vals += [0x10000 + (i * 7919) % 0x10000 for i in range(20000)]
    vals += [0x20000 + (i * 7919) % 0xF000 for i in range(8193)]
    return vals


DENSE_CONSTS = (0x10000, 0x10001, 0x18000, 0x1FFFE, 0x1FFFF, 0x20000, 0x20001,
                0x27777)
_DENSE = {}


def dense_raw():
    if not _DENSE:
        vals = dense_vals()
        for c in DENSE_CONSTS:
            vals += [c - 1, c, c + 1]
        _DENSE["raw"] = region_bytes([cell_int(1, v) for v in vals])
    return _DENSE["raw"]


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [None, "1"])
def test_dense_buckets(engine, grid):
    """every row but two in two adjacent buckets, all six comparers, constants
    on the bucket bounds (low halves 0x0000 and 0xFFFF) and inside; at the
    default grid and with one block striding over both slices"""
    raw = dense_raw()
    rgn = open_region(engine, raw)
    try:
        first = True
        for sig in SIGS:
            for c in DENSE_CONSTS:
                ways(engine, count_req(COLS1, cmp(sig, c)), [rgn], raw,
                     builds=1 if first else 0, grid=grid)
                first = False
    finally:
        rgn.close()


# ---- constants that cut nothing --------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sig", SIGS)
def test_empty_bucket_and_outside(engine, sig):
    """a constant in a bucket that holds no row, below the minimum, above the
    maximum, and on the minimum and the maximum themselves"""
    n = 8193
    vals = [(i * 1000003) % 3000000000 for i in range(n)]
    vals[0], vals[-1] = 0, LAST
    empty_h = next(h for h in range(1, 0x10000)
                   if not any(v >> 16 == h for v in vals))
    raw = edge_raw(n)
    rgn = open_region(engine, raw)
    try:
        first = True
        for c in ((empty_h << 16) | 0x1234, empty_h << 16,
                  (empty_h << 16) | 0xFFFF, -5, -1, 0, 1, max(vals) - 1,
                  max(vals), max(vals) + 1, 1 << 40):
            ways(engine, count_req(COLS1, cmp(sig, c)), [rgn], raw,
                 builds=1 if first else 0)
            first = False
    finally:
        rgn.close()


# ---- several regions -------------------------------------------------------
def spread_rows(n, mul, top):
    return [cell_int(1, 0 if i == 0 else (i * mul) % top) for i in range(n)]


@pytest.mark.gpu
def test_three_regions_three_kernels(engine):
    """one request over an indexed region (3000 rows), a 2-byte region and a
    split region of 1000 rows that a threshold of 2000 rows keeps off the
    index: k_plane_fcb, k_plane_fcn<uint16_t> and k_plane_fcs add into the
    same count words, the first launch stamps and the last finalizes, in
    every order of the three"""
    rows = [spread_rows(3000, 1000003, 3000000000),
            spread_rows(500, 131, 50000),
            spread_rows(1000, 7000003, 3000000000)]
    raws = [region_bytes(r) for r in rows]
    rgns = [open_region(engine, r) for r in raws]
    try:
        first = True
        for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
            raw_all = region_bytes(sum((rows[i] for i in order), []))
            for sig, c in ((F.SIG_LT_INT, 1500000000), (F.SIG_GE_INT, 40000),
                           (F.SIG_NE_INT, 0)):
                ways(engine, count_req(COLS1, cmp(sig, c)),
                     [rgns[i] for i in order], raw_all, bucket=1, split=1,
                     builds=1 if first else 0, min_rows="2000")
                first = False
    finally:
        for r in rgns:
            r.close()


# ---- switches --------------------------------------------------------------
@pytest.mark.gpu
def test_stream_wait_instead_of_poll(engine):
    """COPR_FC_POLL_US=0: the host waits for the stream and reads the same
    words"""
    raw = edge_raw(8193)
    rgn = open_region(engine, raw)
    try:
        for i, (sig, c) in enumerate(EDGE_CONDS):
            ways(engine, count_req(COLS1, cmp(sig, c)), [rgn], raw,
                 builds=1 if i == 0 else 0, poll="0")
    finally:
        rgn.close()


@pytest.mark.gpu
def test_all_lo_takes_the_scan(engine):
    """COPR_SPLIT_ALL_LO=1 means every row through both halves of the scan:
    an indexed plane then takes k_plane_fcs"""
    raw = edge_raw(8193)
    rgn = open_region(engine, raw)
    try:
        sig, c = EDGE_CONDS[0]
        req = count_req(COLS1, cmp(sig, c))
        plain = ways(engine, req, [rgn], raw, builds=1)
        assert ways(engine, req, [rgn], raw, bucket=0, split=1,
                    all_lo="1") == plain
    finally:
        rgn.close()


@pytest.mark.gpu
def test_budget_without_room_for_the_index(engine):
    """40 000 rows under a budget of 1 MiB: the wide plane (9 B per row) and
    the split plane (4 B) fit, the index (2 B per row and the offsets) does
    not. No index is built, then or later, and the scan answers."""
    n = 40000
    vals = [(i * 1000003) % 3000000000 for i in range(n)]
    vals[0] = 0
    raw = region_bytes([cell_int(1, v) for v in vals])
    rgn = open_region(engine, raw)
    try:
        for sig, c in ((F.SIG_LT_INT, 1500000000), (F.SIG_GE_INT, 1500000000)):
            ways(engine, count_req(COLS1, cmp(sig, c)), [rgn], raw, bucket=0,
                 split=1, builds=0, budget="1")
        # the verdict is remembered when the budget has grown
        ways(engine, count_req(COLS1, cmp(F.SIG_LT_INT, 1500000000)), [rgn],
             raw, bucket=0, split=1, builds=0)
    finally:
        rgn.close()


@pytest.mark.gpu
def test_region_closed_after_a_polled_request(engine):
    """the region, its index and its offsets go right after the request's
    sequence word arrived; the next region starts from clean words"""
    req = count_req(COLS1, cmp(F.SIG_LT_INT, LAST + 1))
    for n in (8193, 9):
        raw = edge_raw(n)
        rgn = open_region(engine, raw)
        try:
            b0 = engine.bucket_stats()
            with env(COPR_NO_PLANES=None, COPR_NO_NARROW=None,
                     COPR_NO_BUCKETS=None, COPR_BUCKET_MIN_ROWS="0",
                     COPR_PLANE_BUDGET_MB="64", COPR_FC_POLL_US=None):
                res = _run(engine, req, [rgn])
        finally:
            rgn.close()
        b1 = engine.bucket_stats()
        assert (b1[0] - b0[0], b1[1] - b0[1]) == (1, 1)
        assert res == _oracle(req, raw)
