"""Narrow filter planes and the one-dispatch filter+count step (DESIGN.md
§9e; kernels.hip k_plane_stats / k_plane_narrow / k_plane_fcn).

Every case runs one request four ways and wants the same bytes (or the same
error) from all of them:
  - default: the narrow path, asserted through Engine.narrow_stats();
  - COPR_NO_NARROW=1: the wide k_plane_fc;
  - COPR_NO_PLANES=1: the scan path;
  - the oracle.

Regions are tiny. Rows are short, so the plane budget is raised with
COPR_PLANE_BUDGET_MB as in test_col_planes.py.
"""
import pytest

import tikv_amd
from tikv_amd import _ffi as F

import test_topn_stream as T
from test_topn_stream import cell_int, cell_null, cell_real
from test_dev_chunk import region_bytes
from test_col_planes import _oracle, _run, cell_uint, count_req, env

I_MIN, I_MAX = -(1 << 63), (1 << 63) - 1
U63 = 1 << 63
SIGS = (F.SIG_LT_INT, F.SIG_LE_INT, F.SIG_GT_INT, F.SIG_GE_INT,
        F.SIG_EQ_INT, F.SIG_NE_INT)


def four_ways(engine, req, rgns, oracle_raw, narrow=True, budget_mb="64",
              grid=None):
    """narrow = how many regions must take k_plane_fcn on the default leg
    (True = all). Every region must be served from a plane, narrow or wide,
    on the first two legs. Returns (result, narrow launches, narrow builds)
    of the default leg."""
    want = len(rgns) if narrow is True else int(narrow)
    n0 = engine.narrow_stats()
    p0 = engine.plane_stats()
    with env(COPR_NO_PLANES=None, COPR_NO_NARROW=None,
             COPR_PLANE_BUDGET_MB=budget_mb, COPR_NARROW_GRID=grid):
        r_narrow = _run(engine, req, rgns)
    n1 = engine.narrow_stats()
    p1 = engine.plane_stats()
    assert n1[0] - n0[0] == want, \
        "narrow launches %d, expected %d" % (n1[0] - n0[0], want)
    assert p1[0] - p0[0] == len(rgns), "a region left the plane path"
    with env(COPR_NO_PLANES=None, COPR_NO_NARROW="1",
             COPR_PLANE_BUDGET_MB=budget_mb):
        r_wide = _run(engine, req, rgns)
    assert engine.narrow_stats() == n1, "COPR_NO_NARROW=1 used narrow planes"
    assert engine.plane_stats()[0] - p1[0] == len(rgns)
    with env(COPR_NO_PLANES="1", COPR_PLANE_BUDGET_MB=budget_mb):
        r_scan = _run(engine, req, rgns)
    assert engine.narrow_stats() == n1
    assert r_narrow == r_wide
    assert r_narrow == r_scan
    r_orc = _oracle(req, oracle_raw)
    if r_orc[0] == "ok":
        assert r_narrow == r_orc
    else:
        assert r_narrow[0] == "err"
    return r_narrow, n1[0] - n0[0], n1[1] - n0[1]


def open_region(engine, raw):
    k, ko, v, vo, n = raw[:5]
    return engine.region_raw(k, ko, v, vo, n)


def lt(off, c, **kw):
    return tikv_amd.cmp_col_const(off, F.SIG_LT_INT, c, **kw)


# ---- row counts: one column per width ----------------------------------
def width_row(i):
    return (cell_int(1, (i * 37) % 200 - 100)                  # W = 1
            + cell_int(2, (i * 131) % 50000 - 25000)           # W = 2
            + cell_int(3, (i * 1000003) % 3000000000 - 1500000000))  # W = 4


COLS3 = [tikv_amd.Col(1), tikv_amd.Col(2), tikv_amd.Col(3)]
_WIDTH_RAW = {}


def width_raw(n):
    if n not in _WIDTH_RAW:
        _WIDTH_RAW[n] = region_bytes([width_row(i) for i in range(n)])
    return _WIDTH_RAW[n]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 257, 1023, 1024,
                               1025, 2999])
def test_row_counts(engine, n):
    """tail masking: sizes around the 4, 8 and 16 rows one lane loads and
    around one block's 1024 vectors, for each element width"""
    raw = width_raw(n)
    rgn = open_region(engine, raw)
    try:
        for off, c in ((0, 7), (1, -1000), (2, 123456789)):
            res, _, builds = four_ways(engine, count_req(COLS3, lt(off, c)),
                                       [rgn], raw)
            assert res[0] == "ok" and builds == 1
    finally:
        rgn.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 65, 1025])
def test_row_counts_no_pipe(engine, n):
    """COPR_NO_PIPE=1 beside COPR_NO_PLANES=1: the single-buffer
    k_scan_agg<1, false> gives the bytes of the pipelined scan leg"""
    raw = width_raw(n)
    rgn = open_region(engine, raw)
    try:
        for off, c in ((0, 7), (1, -1000), (2, 123456789)):
            req = count_req(COLS3, lt(off, c))
            with env(COPR_NO_PLANES="1", COPR_NO_PIPE=None,
                     COPR_PLANE_BUDGET_MB="64"):
                r_scan = _run(engine, req, [rgn])
            with env(COPR_NO_PLANES="1", COPR_NO_PIPE="1",
                     COPR_PLANE_BUDGET_MB="64"):
                r_nopipe = _run(engine, req, [rgn])
            assert r_scan[0] == "ok"
            assert r_nopipe == r_scan
            assert r_nopipe == _oracle(req, raw)
    finally:
        rgn.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,off,grid", [(8193, 2, "2"), (8193, 1, "1"),
                                        (16385, 0, "1")])
def test_one_row_past_a_grid_stride_step(engine, n, off, grid):
    """k_plane_fcn steps grid x 256 lanes x 4 loads x (16 / W) rows. The
    default grid makes that millions of rows, so the grid is capped with
    COPR_NARROW_GRID: W = 4 with two blocks and W = 2 with one step 8192
    rows, W = 1 with one block 16384; each region is one row longer."""
    raw = width_raw(n)
    rgn = open_region(engine, raw)
    try:
        for c in (-90, 0, 40000):
            res, _, _ = four_ways(engine, count_req(COLS3, lt(off, c)), [rgn],
                                  raw, grid=grid)
            assert res[0] == "ok"
    finally:
        rgn.close()


# ---- each width at its limit -------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w", [1, 2, 4])
@pytest.mark.parametrize("over", [0, 1])
def test_width_limits(engine, w, over):
    """max - min = 2^(8W) - 1 fits W bytes; one more takes the next width,
    and past 32 bits the plane is declined for good. Constants sit on and
    beside the top value, which a too-narrow store would alias to 0."""
    span = (1 << (8 * w)) - 1 + over
    lo = -1000
    vals = [lo, lo + span, lo + span - 1, lo + 1] + \
           [lo + (i * 7919) % (span + 1) for i in range(300)]
    raw = region_bytes([cell_int(1, v) for v in vals])
    rgn = open_region(engine, raw)
    cols = [tikv_amd.Col(1)]
    declined = w == 4 and over == 1
    try:
        first = True
        for sig in (F.SIG_LT_INT, F.SIG_GE_INT, F.SIG_EQ_INT):
            for c in (lo, lo + span - 1, lo + span, lo + span + 1,
                      lo + (span + 1) // 2):
                req = count_req(cols, tikv_amd.cmp_col_const(0, sig, c))
                res, _, builds = four_ways(engine, req, [rgn], raw,
                                           narrow=not declined)
                assert res[0] == "ok"
                assert builds == (1 if first and not declined else 0)
                first = False
    finally:
        rgn.close()


# ---- comparers x constants x base positions ----------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("base", [I_MIN, I_MAX - 200, -100, 1000])
def test_comparers_constants_bases(engine, base):
    """all six comparers against constants below min, on min, inside, on
    max, above max, at both ends of int64, and NULL; planes that start at
    INT64_MIN, end at INT64_MAX, straddle zero and sit above it"""
    top = base + 200
    raw = region_bytes([cell_int(1, base + (i * 37) % 201) for i in range(300)])
    rgn = open_region(engine, raw)
    cols = [tikv_amd.Col(1)]
    consts = {I_MIN, I_MAX, base, base + 77, top}
    if base > I_MIN:
        consts.add(base - 1)
    if top < I_MAX:
        consts.add(top + 1)
    try:
        for sig in SIGS:
            for c in sorted(consts):
                req = count_req(cols, tikv_amd.cmp_col_const(0, sig, c))
                res, _, _ = four_ways(engine, req, [rgn], raw)
                assert res[0] == "ok", (sig, c)
            sel = tikv_amd.Expr().col(0).const_null().func(sig, 2)
            res, _, _ = four_ways(engine, count_req(cols, sel), [rgn], raw)
            assert res[0] == "ok", sig
    finally:
        rgn.close()


# ---- unsigned ----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("lo", [U63 + 12345, 5])
def test_unsigned_column(engine, lo):
    """uint cells all above 2^63 (negative as stored) and all below: either
    way signed and unsigned order agree on the plane, so it is narrow"""
    raw = region_bytes([cell_uint(1, lo + (i * 7) % 1000) for i in range(777)])
    rgn = open_region(engine, raw)
    cols = [tikv_amd.Col(1, flag=F.FLAG_UNSIGNED)]
    try:
        for sig in SIGS:
            for c in (0, lo - 1, lo, lo + 500, lo + 999, lo + 1000,
                      (1 << 64) - 1):
                req = count_req(cols, tikv_amd.cmp_col_const(
                    0, sig, c, unsigned_const=True))
                res, _, _ = four_ways(engine, req, [rgn], raw)
                assert res[0] == "ok", (sig, c)
    finally:
        rgn.close()


@pytest.mark.gpu
def test_int_cells_read_as_unsigned_decline(engine):
    """int cells -5..5 under a column flagged unsigned: the plane straddles
    the sign, unsigned order differs from the stored order, so the request
    keeps k_plane_fc; a signed request on the same plane is narrow"""
    raw = region_bytes([cell_int(1, i % 11 - 5) for i in range(300)])
    rgn = open_region(engine, raw)
    try:
        ucols = [tikv_amd.Col(1, flag=F.FLAG_UNSIGNED)]
        for sig in SIGS:
            for c in (0, 3, U63, (1 << 64) - 3):
                req = count_req(ucols, tikv_amd.cmp_col_const(
                    0, sig, c, unsigned_const=True))
                res, launches, _ = four_ways(engine, req, [rgn], raw,
                                             narrow=False)
                assert res[0] == "ok" and launches == 0
        res, _, builds = four_ways(
            engine, count_req([tikv_amd.Col(1)], lt(0, 3)), [rgn], raw)
        assert res[0] == "ok" and builds == 0     # built by the first request
    finally:
        rgn.close()


# ---- planes that cannot be narrowed ------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("odd", ["null", "absent", "real"])
def test_plane_with_one_other_row_declines(engine, odd):
    """exactly one NULL, ABSENT or REAL row among ints: not narrowed, the
    verdict is remembered, results (for REAL: the error) unchanged"""
    rows = [cell_int(2, i) + cell_int(1, i % 90 - 45) for i in range(300)]
    rows[131] = cell_int(2, 131) + {"null": cell_null(1), "absent": b"",
                                    "real": cell_real(1, 2.5)}[odd]
    raw = region_bytes(rows)
    rgn = open_region(engine, raw)
    cols = [tikv_amd.Col(2), tikv_amd.Col(1)]
    try:
        for c in (3, -20):
            res, launches, builds = four_ways(
                engine, count_req(cols, lt(1, c)), [rgn], raw, narrow=False)
            assert (launches, builds) == (0, 0)
            assert res[0] == ("err" if odd == "real" else "ok")
    finally:
        rgn.close()


# ---- budget ------------------------------------------------------------
@pytest.mark.gpu
def test_budget_admits_wide_plane_only(engine):
    """1 MiB budget, 110000 rows: the wide plane (9 B per row) fits, the
    2-byte narrow plane on top of it does not; the request takes k_plane_fc
    and the narrow build is not tried again"""
    n = 110000
    raw = region_bytes([cell_int(1, (i * 37) % 1000 - 500) for i in range(n)])
    rgn = open_region(engine, raw)
    cols = [tikv_amd.Col(1)]
    try:
        for c in (0, 400):
            res, launches, builds = four_ways(
                engine, count_req(cols, lt(0, c)), [rgn], raw, narrow=False,
                budget_mb="1")
            assert res[0] == "ok" and (launches, builds) == (0, 0)
        # the verdict stays even when a later request brings a larger budget
        res, launches, builds = four_ways(
            engine, count_req(cols, lt(0, 7)), [rgn], raw, narrow=False)
        assert (launches, builds) == (0, 0)
    finally:
        rgn.close()


# ---- several regions ---------------------------------------------------
@pytest.mark.gpu
def test_two_narrow_regions_one_total(engine):
    rows_a = [cell_int(1, i % 90 - 45) for i in range(777)]
    rows_b = [cell_int(1, 100000 + (i * 31) % 70000) for i in range(1025)]
    raw_a, raw_b = region_bytes(rows_a), region_bytes(rows_b)
    raw_all = region_bytes(rows_a + rows_b)
    ra, rb = open_region(engine, raw_a), open_region(engine, raw_b)
    cols = [tikv_amd.Col(1)]
    try:
        for sig, c in ((F.SIG_LT_INT, 20), (F.SIG_GE_INT, 120000),
                       (F.SIG_NE_INT, 0)):
            req = count_req(cols, tikv_amd.cmp_col_const(0, sig, c))
            res, launches, _ = four_ways(engine, req, [ra, rb], raw_all)
            assert res[0] == "ok" and launches == 2
    finally:
        ra.close()
        rb.close()


@pytest.mark.gpu
def test_narrow_region_beside_a_declined_one(engine):
    """region B holds one NULL row and keeps k_plane_fc; region A's narrow
    kernel adds into the same accumulator through the usual sequence"""
    rows_a = [cell_int(1, i % 90 - 45) for i in range(777)]
    rows_b = [cell_int(1, i % 50) for i in range(300)]
    rows_b[7] = cell_null(1)
    raw_a, raw_b = region_bytes(rows_a), region_bytes(rows_b)
    raw_all = region_bytes(rows_a + rows_b)
    ra, rb = open_region(engine, raw_a), open_region(engine, raw_b)
    cols = [tikv_amd.Col(1)]
    try:
        for order in ([ra, rb], [rb, ra]):
            raw = raw_all if order[0] is ra else region_bytes(rows_b + rows_a)
            res, launches, _ = four_ways(engine, count_req(cols, lt(0, 20)),
                                         order, raw, narrow=1)
            assert res[0] == "ok" and launches == 1
    finally:
        ra.close()
        rb.close()


# ---- the device words reset themselves ---------------------------------
@pytest.mark.gpu
def test_self_reset_between_requests(engine):
    """five narrow requests in a row, a sum() through k_plane_agg, a narrow
    request, a request that fails with a row parse error on another region,
    a narrow request: every count is right"""
    rows = [cell_int(1, (i * 37) % 1000 - 500) + cell_int(2, i)
            for i in range(2999)]
    raw = region_bytes(rows)
    bad_rows = [cell_int(1, i % 50) + cell_int(2, i) for i in range(300)]
    bad_rows[131] = b"\x08\x02\x0f\x01" + bad_rows[131]
    raw_bad = region_bytes(bad_rows)
    raw_both = region_bytes(rows + bad_rows)
    rgn, rgn_bad = open_region(engine, raw), open_region(engine, raw_bad)
    cols = [tikv_amd.Col(1), tikv_amd.Col(2)]

    def narrow(c):
        res, launches, _ = four_ways(engine, count_req(cols, lt(0, c)),
                                     [rgn], raw)
        assert res[0] == "ok" and launches == 1
        return res

    try:
        seen = {narrow(c)[1] for c in (-400, -123, 0, 77, 499)}
        assert len(seen) == 5                    # five different counts
        req = (tikv_amd.DagSelect(cols).where(lt(0, 10))
               .simple_agg([tikv_amd.sum_col(1), tikv_amd.count_star()])
               .build())
        with env(COPR_NO_PLANES=None, COPR_PLANE_BUDGET_MB="64"):
            r_sum = _run(engine, req, [rgn])
        assert r_sum == _oracle(req, raw)
        narrow(33)
        # parse error in the other region of a two-region request
        n0 = engine.narrow_stats()
        with env(COPR_NO_PLANES=None, COPR_PLANE_BUDGET_MB="64"):
            r_err = _run(engine, count_req(cols, lt(0, 10)), [rgn, rgn_bad])
        assert r_err[0] == "err" and "row parse error" in r_err[1]
        assert _oracle(count_req(cols, lt(0, 10)), raw_both)[0] == "err"
        assert engine.narrow_stats()[0] - n0[0] == 1
        narrow(-250)
        narrow(250)
    finally:
        rgn.close()
        rgn_bad.close()
