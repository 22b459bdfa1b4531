"""The atomic-free tail of a one-block launch that opens and finalizes its
request (narrow_planes.hip fcn_block_count and
fcn_hand_over, copr_engine.cpp).

A solo launch touches no device word, so what can go wrong is a launch that
takes the solo tail when it should not (a second block's rows missing, an
earlier launch's count left in the count words) or that does not when the
host says it did, and a hand-over whose count or ticks belong to another
request. Every response is checked against the oracle and against
COPR_NARROW_NO_FINALIZE=1 (the same kernel, counted through the usual
accumulator), every request against Engine.fc_solo(), fc_wait_stats() and
narrow_stats(), and every kernel time against the host clock of its own call
(test_fc_step.fc_step).
"""
import pytest

import tikv_amd
from tikv_amd import _ffi as F
from tikv_amd import in_col_consts as IN

from test_topn_stream import cell_int
from test_dev_chunk import region_bytes
from test_col_planes import _oracle, _run, count_req, env
from test_narrow_planes import open_region
from test_packed_fc import CUT
from test_fc_step import (COLS1, KINDS, count_in, fc_step, lt_req, raw_of,
                          step, want_of)
from test_pair_planes import COLS2, LAST, LAST2, rows2

pytestmark = pytest.mark.gpu
cmp = tikv_amd.cmp_col_const


def in_step(eng, req, rgns):
    """fc_step for an IN list, whose launches in_stats() and
    in_split_launches() count, not narrow_stats()"""
    i0 = sum(eng.in_stats()) + eng.in_split_launches()
    n0, w0 = eng.narrow_stats(), eng.fc_wait_stats()
    res, kernel_ns, host_ns = step(eng, req, rgns)
    assert sum(eng.in_stats()) + eng.in_split_launches() - i0 == len(rgns)
    assert eng.narrow_stats()[0] == n0[0]
    assert sum(eng.fc_wait_stats()) - sum(w0) == 1
    assert 0 < kernel_ns < host_ns, (kernel_ns, host_ns)
    return res


def solo_step(eng, req, rgns, want, solo, in_list=False, **kw):
    """fc_step that must (not) count as solo, equal to the request's own
    response under COPR_NARROW_NO_FINALIZE=1 and to want: the oracle's stored
    response, a region's raw bytes to put to the oracle, or a count"""
    s0 = eng.fc_solo()
    res = in_step(eng, req, rgns) if in_list else fc_step(eng, req, rgns, **kw)
    assert eng.fc_solo() - s0 == (1 if solo else 0), (solo, kw)
    w0 = eng.fc_wait_stats()
    with env(COPR_NARROW_NO_FINALIZE="1", COPR_PLANE_BUDGET_MB="64",
             COPR_NARROW_GRID=kw.get("grid")):
        plain = _run(eng, req, rgns)
    assert eng.fc_wait_stats() == w0 and eng.fc_solo() - s0 == (1 if solo else 0)
    assert res == plain
    if isinstance(want, int):
        assert count_in(res) == want and res[2] == 1
    elif want[0] == "ok":
        assert res == want
    else:
        assert res == _oracle(req, want)
    return res


# ---- one block's iteration, to the row ----------------------------------
@pytest.mark.parametrize("edge", [None, -1, 0, 1])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_rows_of_one_block(engine, kind, edge):
    """1, R - 1 and R rows are one block and solo, R + 1 rows are two blocks
    and ticketed; twice each, the second finds what the first left"""
    r = KINDS[kind][2]
    n = 1 if edge is None else r + edge
    c = KINDS[kind][1]
    raw = raw_of(kind, n)
    rgn = open_region(engine, raw)
    try:
        for _ in range(2):
            solo_step(engine, lt_req(c), [rgn], want_of(kind, n, c), n <= r)
    finally:
        rgn.close()


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_grid_stride_solo(engine, kind):
    """3R + 5 rows under a grid of one block: solo with a grid-stride loop"""
    n = 3 * KINDS[kind][2] + 5
    c = KINDS[kind][1]
    rgn = open_region(engine, raw_of(kind, n))
    try:
        solo_step(engine, lt_req(c), [rgn], want_of(kind, n, c), True,
                  grid="1")
        solo_step(engine, lt_req(c), [rgn], want_of(kind, n, c), False)
    finally:
        rgn.close()


# ---- device words stay zero ---------------------------------------------
def test_solo_and_ticketed_alternating(engine):
    """32 requests on one engine, a solo and a ticketed region in turn, four
    different right answers: a tail that left a count word, the ticket or the
    stamp non-zero shows as a wrong count in the request behind it"""
    sizes = (8191, 3 * 8192 + 5)
    consts = (CUT, 1500000000)
    order = [(0, 0), (1, 1), (0, 1), (1, 0)]
    wants = {(r, c): want_of("split", sizes[r], consts[c]) for r, c in order}
    assert len({count_in(w) for w in wants.values()}) == 4
    rgns = [open_region(engine, raw_of("split", n)) for n in sizes]
    try:
        for i in range(32):
            r, c = order[i % 4]
            solo_step(engine, lt_req(consts[c]), [rgns[r]], wants[(r, c)],
                      r == 0)
    finally:
        for rgn in rgns:
            rgn.close()


@pytest.mark.parametrize("n_regions", [2, 3])
def test_one_block_regions_are_not_solo(engine, n_regions):
    """every launch is one block, the first has a stamp and no ticket, the
    last a ticket and no stamp: none is solo, the count is the sum"""
    parts = [("split", 8191), ("w2", 1000), ("w1", 16384)][:n_regions]
    c = 1100
    rgns = [open_region(engine, raw_of(k, n)) for k, n in parts]
    try:
        total = sum(count_in(want_of(k, n, c)) for k, n in parts)
        for _ in range(2):
            solo_step(engine, lt_req(c), rgns, total, False)
        k, n = parts[0]
        solo_step(engine, lt_req(c), [rgns[0]], want_of(k, n, c), True)
    finally:
        for rgn in rgns:
            rgn.close()


# ---- the bucket index ----------------------------------------------------
N_BKT = 20000
_BKT = {}


def bkt_vals():
    vals = [(i * 1000003) % 3000000000 for i in range(N_BKT)]
    vals[-1] = CUT
    return vals


def bkt_raw():
    if "raw" not in _BKT:
        _BKT["raw"] = region_bytes([cell_int(1, v) for v in bkt_vals()])
    return _BKT["raw"]


def empty_bucket_const():
    """a constant in a bucket of 65536 values that holds no row"""
    full = {v >> 16 for v in bkt_vals()}
    return next(h for h in range(100, 40000) if h not in full) * 65536 + 9


@pytest.mark.parametrize("case", ["one edge", "two edges", "empty", "inverted"])
def test_bucket_index_solo(engine, case):
    """k_plane_fcb over 20 000 rows reads a few rows of one or two edge
    buckets in one block. With both slices empty nothing is loaded between
    the two clock reads, and the kernel time must still be above zero"""
    conds = {"one edge": [cmp(0, F.SIG_LT_INT, CUT)],
             "two edges": [cmp(0, F.SIG_GE_INT, 1000003 * 7),
                           cmp(0, F.SIG_LT_INT, CUT)],
             "empty": [cmp(0, F.SIG_LT_INT, empty_bucket_const())],
             "inverted": [cmp(0, F.SIG_GE_INT, CUT)]}[case]
    req = count_req(COLS1, *conds)
    raw = bkt_raw()
    rgn = open_region(engine, raw)
    try:
        with env(COPR_BUCKET_MIN_ROWS="0", COPR_NO_BUCKETS=None):
            for _ in range(3):
                b0 = engine.bucket_stats()[0]
                res = solo_step(engine, req, [rgn], raw, True)
                # once on the one-dispatch branch, once without finalizing
                assert engine.bucket_stats()[0] - b0 == 2
                assert 0 < count_in(res) < N_BKT
    finally:
        rgn.close()


@pytest.mark.parametrize("n,solo", [(12000, True), (30000, False)])
def test_bucket_slice_of_two_iterations_takes_one_block(engine, n, solo):
    """an edge bucket of n rows: up to two iterations of one block (16384
    slice rows) an opening-and-finalizing launch is one block and solo with a
    grid-stride loop, beyond that the grid is the ticketed one; under
    COPR_NARROW_GRID=2 two iterations are two blocks again"""
    vals = [(0x1234 << 16) + (i * 7) % 65536 for i in range(n)] + \
           [(i * 1000003) % 3000000000 for i in range(1000)]
    raw = region_bytes([cell_int(1, v) for v in vals])
    req = count_req(COLS1, cmp(0, F.SIG_LT_INT, (0x1234 << 16) + 40000))
    rgn = open_region(engine, raw)
    try:
        with env(COPR_BUCKET_MIN_ROWS="0", COPR_NO_BUCKETS=None):
            for _ in range(2):
                b0 = engine.bucket_stats()[0]
                res = solo_step(engine, req, [rgn], raw, solo)
                assert engine.bucket_stats()[0] - b0 == 2
                assert 0 < count_in(res) < len(vals)
            assert solo_step(engine, req, [rgn], raw, False, grid="2") == res
    finally:
        rgn.close()


# ---- the other kernels that end in the tail --------------------------------
@pytest.mark.parametrize("span", [60000, 2 * 10**9])
def test_in_list_solo(engine, span):
    """k_plane_inb over a 2-byte plane and k_plane_ins over a split plane"""
    n = 1100
    vals = [(i * 7919) % (span + 1) - 500 for i in range(n)]
    vals[0], vals[-1] = -500, span - 500
    items = [vals[i] for i in (0, 1, 77, 500, n - 1)] + [span + 5, -501]
    want = sum(v in set(items) for v in vals)
    assert 0 < want < n
    req = (tikv_amd.DagSelect(COLS1).where(IN(0, items, False))
           .simple_agg([tikv_amd.count_star()]).build())
    rgn = open_region(engine, region_bytes([cell_int(1, v) for v in vals]))
    try:
        with env(COPR_NO_IN_SPLIT=None, COPR_NO_IN_PLANES=None,
                 COPR_IN_GRID=None):
            for _ in range(2):
                solo_step(engine, req, [rgn], want, True, in_list=True)
    finally:
        rgn.close()


def test_pair_solo(engine):
    """k_plane_fc2 over two split planes"""
    raw = region_bytes(rows2(1100))
    req = count_req(COLS2, cmp(0, F.SIG_LT_INT, LAST + 1),
                    cmp(1, F.SIG_GE_INT, LAST2))
    rgn = open_region(engine, raw)
    try:
        with env(COPR_NO_PAIR=None):
            p0 = engine.pair_launches()
            for _ in range(2):
                solo_step(engine, req, [rgn], raw, True)
            assert engine.pair_launches() - p0 == 4
    finally:
        rgn.close()


# ---- both waits, and the region's lifetime -----------------------------
def test_solo_fallback_and_poll(engine):
    """COPR_FC_POLL_US=0 reads the words after the stream wait, a
    deadline of 10 s after the polled word (fc_step checks which wait it
    was)"""
    n, c = 8000, CUT
    rgn = open_region(engine, raw_of("split", n))
    try:
        for i in range(6):
            solo_step(engine, lt_req(c), [rgn], want_of("split", n, c), True,
                      poll=("0", "10000000", None)[i % 3])
    finally:
        rgn.close()


def test_region_closed_right_after_a_solo_request(engine):
    c = CUT
    for n in (8000, 1, 8192, 8193):
        rgn = open_region(engine, raw_of("split", n))
        try:
            solo_step(engine, lt_req(c), [rgn], want_of("split", n, c),
                      n <= 8192)
            # the region goes right behind a request of the branch
            s0 = engine.fc_solo()
            res = fc_step(engine, lt_req(c), [rgn])
        finally:
            rgn.close()
        assert engine.fc_solo() - s0 == (1 if n <= 8192 else 0)
        assert res == want_of("split", n, c), n
