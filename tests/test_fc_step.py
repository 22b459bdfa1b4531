"""The filter+count step that ends without events or a stream wait (DESIGN.md
§9n; narrow_planes.hip fcn_block_count, copr_engine.cpp, fc_wait.h).

The launch that opens a request stamps the wall clock, the block that draws
the last ticket hands the host count, ticks and the request's sequence number,
and the host waits for the number. What can go wrong shows up as a wrong
count (a stale host word, a sequence number reused, state words not
re-zeroed) or as a kernel time that is zero or longer than the call that
produced it (a stamp stored after its ticket, a stamp left over). Every
expected response is the oracle's, computed once per region and request.
COPR_FC_POLL_US=0 sends a request through the fallback (the stream wait).
Engine.fc_wait_stats() says which wait ended a request: every request of the
one-dispatch branch moves exactly one of its two counters, the non-finalizing
narrow branch and every other branch move neither.
"""
import time

import pytest

import tikv_amd
from tikv_amd import _ffi as F

from test_topn_stream import cell_int
from test_dev_chunk import region_bytes
from test_col_planes import _oracle, count_req, env
from test_narrow_planes import open_region
from test_packed_fc import BASE2, CUT, split_vals, two_byte_vals

COLS1 = [tikv_amd.Col(1)]
BASE1 = 1000


def one_byte_vals(n):
    vals = [BASE1 + (i * 7) % 256 for i in range(n)]
    vals[0] = BASE1
    vals[-1] = BASE1 + 255 if n > 1 else BASE1
    return vals


# values, a constant that cuts them, rows of one block's iteration
KINDS = {"split": (split_vals, CUT, 8 * 1024),
         "w2": (two_byte_vals, BASE2 + 131 * 7, 8 * 1024),
         "w1": (one_byte_vals, BASE1 + 100, 16 * 1024)}

_RAW = {}
_WANT = {}


def raw_of(kind, n):
    if (kind, n) not in _RAW:
        _RAW[(kind, n)] = region_bytes(
            [cell_int(1, v) for v in KINDS[kind][0](n)])
    return _RAW[(kind, n)]


def lt_req(c):
    return count_req(COLS1, tikv_amd.cmp_col_const(0, F.SIG_LT_INT, c))


def want_of(kind, n, c):
    """the oracle's response to col < c over the region, computed once"""
    if (kind, n, c) not in _WANT:
        _WANT[(kind, n, c)] = _oracle(lt_req(c), raw_of(kind, n))
        assert _WANT[(kind, n, c)][0] == "ok"
    return _WANT[(kind, n, c)]


def count_in(res):
    data = res[1]
    assert len(data) == 9 and data[0] == 3
    return int.from_bytes(data[1:9], "big") ^ (1 << 63)


def step(eng, req, rgns, grid=None, poll=None, no_narrow=None):
    """one request on the default path unless a switch says otherwise;
    returns (result, kernel_ns, ns of the host clock around the call)"""
    with env(COPR_NO_PLANES=None, COPR_NO_NARROW=no_narrow,
             COPR_NARROW_NO_FINALIZE=None, COPR_PLANE_BUDGET_MB="64",
             COPR_NARROW_GRID=grid, COPR_SPLIT_ALL_LO=None,
             COPR_FC_POLL_US=poll):
        t0 = time.perf_counter_ns()
        data, n, kernel_ns = eng.dag_run(req, rgns)
        host_ns = time.perf_counter_ns() - t0
    return ("ok", data, n), kernel_ns, host_ns


def fc_step(eng, req, rgns, **kw):
    """step() that must take the one-dispatch filter+count branch: one narrow
    launch per region and one wait, on the word or on the stream. With
    COPR_FC_POLL_US=0 it is the stream; with a deadline of its own (the tests
    give 10 s) it is the word; the derived deadline (2 ms and more) leaves
    that to the machine. The kernel's own time lies inside the call that
    launched it and waited for it, whatever the machine does."""
    n0, w0 = eng.narrow_stats(), eng.fc_wait_stats()
    res, kernel_ns, host_ns = step(eng, req, rgns, **kw)
    assert eng.narrow_stats()[0] - n0[0] == len(rgns)
    polled, fell = (b - a for a, b in zip(w0, eng.fc_wait_stats()))
    assert polled + fell == 1, (polled, fell)
    if kw.get("poll") is not None:
        assert fell == (1 if kw["poll"] == "0" else 0), (kw["poll"], fell)
    assert 0 < kernel_ns < host_ns, (kernel_ns, host_ns)
    return res


# ---- one engine, 64 consecutive requests -------------------------------
@pytest.mark.gpu
def test_sixty_four_requests(engine):
    """two regions of different size and two constants, alternating so that
    consecutive right answers differ"""
    sizes = (8193, 3 * 8192 + 5)
    consts = (CUT, 1500000000)
    order = [(0, 0), (1, 1), (0, 1), (1, 0)]
    wants = {(r, c): want_of("split", sizes[r], consts[c]) for r, c in order}
    assert len({count_in(w) for w in wants.values()}) == 4
    rgns = [open_region(engine, raw_of("split", n)) for n in sizes]
    try:
        for i in range(64):
            r, c = order[i % 4]
            res = fc_step(engine, lt_req(consts[c]), [rgns[r]])
            assert res == wants[(r, c)], (i, count_in(res))
    finally:
        for rgn in rgns:
            rgn.close()


# ---- row counts per kernel ---------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("grid", [None, "1", "3"])
@pytest.mark.parametrize("edge", [None, -1, 0, 1])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_row_counts(engine, kind, edge, grid):
    """one row, and one block's iteration less a row, exactly, plus a row.
    With one block, block 0 stamps and finalizes; with two, the block that
    draws the last ticket need not be the one that stamped. Each request
    runs twice: the second finds the words the first left."""
    n = 1 if edge is None else KINDS[kind][2] + edge
    c = KINDS[kind][1]
    rgn = open_region(engine, raw_of(kind, n))
    try:
        for _ in range(2):
            assert fc_step(engine, lt_req(c), [rgn], grid=grid) == \
                want_of(kind, n, c)
    finally:
        rgn.close()


# ---- multi-region requests ---------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_regions", [2, 3])
def test_multi_region(engine, n_regions):
    """stamp on the first launch, finalize on the last: the count is the sum
    of the regions' own counts, and the request repeated gives the same
    bytes"""
    parts = [("split", 8193), ("w2", 8200), ("w1", 16385)][:n_regions]
    c = 1100                      # cuts the 1- and 2-byte values, not the split
    rgns = [open_region(engine, raw_of(k, n)) for k, n in parts]
    try:
        total = sum(count_in(want_of(k, n, c)) for k, n in parts)
        first = fc_step(engine, lt_req(c), rgns)
        assert count_in(first) == total and first[2] == 1
        for _ in range(2):
            assert fc_step(engine, lt_req(c), rgns) == first
        # and each region alone still answers for itself
        for (k, n), rgn in zip(parts, rgns):
            assert fc_step(engine, lt_req(c), [rgn]) == want_of(k, n, c)
    finally:
        for rgn in rgns:
            rgn.close()


# ---- the fallback ------------------------------------------------------
@pytest.mark.gpu
def test_fallback_alternating(engine):
    """COPR_FC_POLL_US=0, unset and a deadline of 10 s, in turn on one
    engine: the same bytes and a kernel time each way; 0 ends on the stream
    wait and 10 s on the polled word (fc_step checks the counters), so the
    switch is read and both waits are taken"""
    n, c = 8193, CUT
    rgn = open_region(engine, raw_of("split", n))
    try:
        for i in range(9):
            res = fc_step(engine, lt_req(c), [rgn],
                          poll=("0", None, "10000000")[i % 3])
            assert res == want_of("split", n, c), i
    finally:
        rgn.close()


# ---- requests of another branch in between -----------------------------
@pytest.mark.gpu
def test_interleaved_with_other_branches(engine):
    """between two polled requests, a request that records events and waits
    for the stream: the same filter+count under COPR_NO_NARROW=1, then a sum
    aggregate"""
    n, c = 8193, CUT
    raw = raw_of("split", n)
    sum_req = (tikv_amd.DagSelect(COLS1)
               .where(tikv_amd.cmp_col_const(0, F.SIG_LT_INT, c))
               .simple_agg([tikv_amd.sum_col(0), tikv_amd.count_star()])
               .build())
    want_sum = _oracle(sum_req, raw)
    assert want_sum[0] == "ok"
    rgn = open_region(engine, raw)
    try:
        assert fc_step(engine, lt_req(c), [rgn]) == want_of("split", n, c)
        n0, w0 = engine.narrow_stats(), engine.fc_wait_stats()
        res, kernel_ns, _ = step(engine, lt_req(c), [rgn], no_narrow="1")
        assert engine.narrow_stats() == n0 and engine.fc_wait_stats() == w0
        assert res == want_of("split", n, c) and kernel_ns > 0
        assert fc_step(engine, lt_req(c), [rgn]) == want_of("split", n, c)
        n0, w0 = engine.narrow_stats(), engine.fc_wait_stats()
        res, kernel_ns, _ = step(engine, sum_req, [rgn])
        assert engine.narrow_stats() == n0 and engine.fc_wait_stats() == w0
        assert res == want_sum and kernel_ns > 0
        assert fc_step(engine, lt_req(c), [rgn]) == want_of("split", n, c)
    finally:
        rgn.close()


# ---- lifetimes ---------------------------------------------------------
@pytest.mark.gpu
def test_region_closed_right_after_a_polled_request(engine):
    """the region goes directly after the request returns, a region of
    another size takes its place and answers for itself"""
    c = CUT
    for n in (8193, 16385, 8191, 3 * 8192 + 5):
        rgn = open_region(engine, raw_of("split", n))
        try:
            res = fc_step(engine, lt_req(c), [rgn])
        finally:
            rgn.close()
        assert res == want_of("split", n, c), n


@pytest.mark.gpu
def test_two_engines_alternating():
    """each engine has its own state words, host words and sequence numbers;
    both go right after their last request"""
    n_a, n_b, c = 8193, 8200, 1100
    a, b = tikv_amd.Engine(0), tikv_amd.Engine(0)
    try:
        ra = open_region(a, raw_of("split", n_a))
        rb = open_region(b, raw_of("w2", n_b))
        try:
            for _ in range(6):
                assert fc_step(a, lt_req(c), [ra]) == want_of("split", n_a, c)
                assert fc_step(b, lt_req(c), [rb]) == want_of("w2", n_b, c)
        finally:
            ra.close()
            rb.close()
    finally:
        a.close()
        b.close()
