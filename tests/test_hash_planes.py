"""Int-key hash aggregation over decoded column planes (DESIGN.md §9d;
kernels.hip k_plane_hash).

FastHashAgg over a table scan reads the group, filter and aggregate columns
from cached planes; decimal cells of at most 18 digits live in the planes
too (state PST_DEC0 + frac). Every case runs one request three ways:
  - default, which must take the new path: hash_plane_launches() advances by
    one per eligible region per attempt;
  - COPR_NO_PLANES=1, the scan kernels, which must not move that counter;
  - the oracle.
plane_stats()[0], the simple-aggregate launch counter, never moves. Group
order is not part of the contract: responses are compared as sorted lists of
per-row datum strings, row counts as row counts, errors as errors.
"""
import pytest

import tikv_amd
from tikv_amd import _ffi as F

import test_topn_stream as T
from test_topn_stream import cell_int, cell_null, cell_real
from test_dev_chunk import region_bytes
from test_col_planes import SIZES, U63, cell_uint, env, gen_raw, _run, _oracle
from test_wide_decimal import D2B, WIDE_VALS, cell, enc_decimal

I64_MIN = -(1 << 63)


def split_datums(data, n_cols):
    """datum-encoded response -> sorted per-row byte strings (NULL, int,
    uint, real, decimal, varint and compact-bytes datums)"""
    rows, p = [], 0
    while p < len(data):
        start = p
        for _ in range(n_cols):
            f = data[p]
            if f == 0:
                p += 1
            elif f in (3, 4, 5):
                p += 9
            elif f == 6:
                prec, frac = data[p + 1], data[p + 2]
                ic = prec - frac
                p += (3 + (ic // 9) * 4 + D2B[ic % 9]
                      + (frac // 9) * 4 + D2B[frac % 9])
            elif f in (8, 9):
                p += 1
                while data[p] & 0x80:
                    p += 1
                p += 1
            else:
                raise AssertionError("unexpected datum flag %d" % f)
        rows.append(bytes(data[start:p]))
    return sorted(rows)


def _norm(res, n_cols):
    if res[0] == "ok":
        return ("ok", split_datums(res[1], n_cols), res[2])
    return res


def hash_three_ways(engine, req, rgns, oracle_raw, n_cols, launches=None,
                    budget_mb="64", oracle=True):
    """default / COPR_NO_PLANES=1 / oracle on one request. launches = how far
    hash_plane_launches() must advance on the default leg (None = one per
    region). Returns (normalised result, planes built)."""
    want = len(rgns) if launches is None else launches
    h0 = engine.hash_plane_launches()
    l0, b0 = engine.plane_stats()
    with env(COPR_NO_PLANES=None, COPR_PLANE_BUDGET_MB=budget_mb):
        r_plane = _norm(_run(engine, req, rgns), n_cols)
    h1 = engine.hash_plane_launches()
    l1, b1 = engine.plane_stats()
    with env(COPR_NO_PLANES="1", COPR_PLANE_BUDGET_MB=budget_mb):
        r_scan = _norm(_run(engine, req, rgns), n_cols)
    assert engine.hash_plane_launches() == h1, "COPR_NO_PLANES=1 used planes"
    assert engine.plane_stats() == (l0, b1), \
        "simple-aggregate launches moved, or COPR_NO_PLANES=1 built a plane"
    assert h1 - h0 == want, "k_plane_hash launches %d, expected %d" % (h1 - h0, want)
    assert r_plane == r_scan
    if oracle:
        r_orc = _oracle(req, oracle_raw)
        if r_orc[0] == "ok":
            assert r_plane == _norm(r_orc, n_cols)
        else:
            assert r_plane[0] == "err"
    return r_plane, b1 - b0


def one_region(engine, req, raw, n_cols, **kw):
    rgn = engine.region_raw(*raw[:5])
    try:
        return hash_three_ways(engine, req, [rgn], raw, n_cols, **kw)
    finally:
        rgn.close()


def cell_dec(col_id, scaled, frac):
    return cell(col_id, enc_decimal(scaled, frac))


# ---- the cfg3 shape: int key, decimal(.,2), a bytes column nobody reads ----
def cfg3_row(i, k):
    v = cell_int(1, (i * 7) % k - k // 2)
    if i % 11 == 3:
        v += cell_null(2)
    else:
        v += cell_dec(2, (i * 7919) % 2_000_003 - 1_000_000, 2)
    return v + T.var_bytes_cell(3, b"pad-%05d" % i)


def cfg3_cols():
    return [tikv_amd.Col(1), tikv_amd.Col(2, tp=F.TP_NEWDECIMAL, decimal=2),
            tikv_amd.Col(3, tp=F.TP_VARCHAR)]


def cfg3_req(*conds):
    """count(*), sum(decimal), avg(key) BY key: 5 datums per row"""
    ds = tikv_amd.DagSelect(cfg3_cols())
    if conds:
        ds = ds.where(*conds)
    return ds.hash_agg([tikv_amd.count_star(), tikv_amd.sum_col(1, decimal=2),
                        tikv_amd.avg_col(0)], tikv_amd.Expr().col(0)).build()


_RAW = {}


def cfg3_raw(n, k):
    if (n, k) not in _RAW:
        _RAW[n, k] = region_bytes([cfg3_row(i, k) for i in range(n)])
    return _RAW[n, k]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("k", [3, 64])
def test_cfg3_shape(engine, n, k):
    """the flagship request; the key column is grouped by and averaged, so
    two planes serve three channels"""
    res, builds = one_region(engine, cfg3_req(), cfg3_raw(n, k), 5)
    assert res[0] == "ok" and res[2] == min(n, k)
    assert builds == 2


# ---- group key edge values ----------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 777])
def test_group_key_reserved_groups(engine, n):
    """NULL key cells and rows without the key column share the NULL group;
    INT64_MIN, the table's EMPTY sentinel, has its own"""
    rows = []
    for i in range(n):
        m = i % 6
        v = b""
        if m == 0:
            v += cell_null(1)
        elif m == 1:
            v += cell_int(1, I64_MIN)
        elif m != 2:                      # m == 2: column absent
            v += cell_int(1, (1 << 63) - 1 - (i % 3))
        rows.append(v + cell_int(2, i - 40))
    cols = [tikv_amd.Col(1), tikv_amd.Col(2)]
    req = (tikv_amd.DagSelect(cols)
           .hash_agg([tikv_amd.count_star(), tikv_amd.sum_col(1),
                      tikv_amd.min_col(1), tikv_amd.count_col(0)],
                     tikv_amd.Expr().col(0)).build())
    res, _ = one_region(engine, req, region_bytes(rows), 5)
    assert res[0] == "ok" and res[2] == 5


@pytest.mark.gpu
def test_group_key_unsigned_above_2_63(engine):
    """an UNSIGNED key column: keys above 2^63 travel as negative i64 and
    must come back as uint datums; a row-v2 cell decodes by that signedness"""
    rows = [cell_uint(1, U63 + (i % 5) * 1000) + cell_int(2, i)
            for i in range(777)]
    rows[100] = v2_cells([(1, 200), (2, 5)])     # 200, not -56
    rows[300] = v2_cells([(1, 200), (2, 7)])
    cols = [tikv_amd.Col(1, flag=F.FLAG_UNSIGNED), tikv_amd.Col(2)]
    req = (tikv_amd.DagSelect(cols)
           .hash_agg([tikv_amd.count_star(),
                      tikv_amd.max_col(0, flag=F.FLAG_UNSIGNED),
                      tikv_amd.sum_col(1)], tikv_amd.Expr().col(0)).build())
    res, _ = one_region(engine, req, region_bytes(rows), 4)
    assert res[0] == "ok" and res[2] == 6


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 257, 2999])
def test_single_group(engine, n):
    """K = 1: every row of every block meets in one LDS slot"""
    res, _ = one_region(engine, cfg3_req(), cfg3_raw(n, 1), 5)
    assert res[0] == "ok" and res[2] == 1


@pytest.mark.gpu
def test_lds_table_overflows_into_global(engine):
    """300 distinct keys against a 256-slot per-block table"""
    res, _ = one_region(engine, cfg3_req(), cfg3_raw(2999, 300), 5)
    assert res[0] == "ok" and res[2] == 300


@pytest.mark.gpu
def test_table_growth_reuses_planes(engine):
    """70 001 distinct keys fill the 65 536-slot table: one grow-and-retry,
    so exactly two k_plane_hash launches over planes built once"""
    n = 70_001
    rows = [cell_int(1, i * 3 - 100_000) + cell_int(2, i % 977 - 400)
            for i in range(n)]
    cols = [tikv_amd.Col(1), tikv_amd.Col(2)]
    req = (tikv_amd.DagSelect(cols)
           .hash_agg([tikv_amd.count_star(), tikv_amd.sum_col(1)],
                     tikv_amd.Expr().col(0)).build())
    res, builds = one_region(engine, req, region_bytes(rows), 3, launches=2)
    assert res[0] == "ok" and res[2] == n and builds == 2


# ---- filters --------------------------------------------------------------
def filt_row(i):
    v = cell_int(1, i % 13 - 6)
    v += cell_null(2) if i % 7 == 0 else cell_int(2, i * 11 - 500)
    if i % 5 != 0:                        # absent in every fifth row
        v += cell_int(3, (i * 13) % 64 - 32)
    v += cell_real(4, (i % 41) * 0.75 - 12.5)
    return v + cell_dec(5, i * 17 - 9000, 2)


def filt_cols(default3=None):
    return [tikv_amd.Col(1), tikv_amd.Col(2),
            tikv_amd.Col(3, default_val=default3),
            tikv_amd.Col(4, tp=F.TP_DOUBLE),
            tikv_amd.Col(5, tp=F.TP_NEWDECIMAL, decimal=2)]


def real_lt(off, x):
    return tikv_amd.Expr().col(off).const_real(x).func(F.SIG_LT_REAL, 2)


def lt_int(off, c):
    return tikv_amd.cmp_col_const(off, F.SIG_LT_INT, c)


def gt_int(off, c):
    return tikv_amd.cmp_col_const(off, F.SIG_GT_INT, c)


FILTERS = {
    "none": lambda: (),
    "int": lambda: (gt_int(1, 0),),
    "real": lambda: (real_lt(3, 2.5),),
    "absent-default": lambda: (lt_int(2, 0),),
    "int+int": lambda: (gt_int(1, 0), lt_int(2, 10)),
    "int+real": lambda: (tikv_amd.cmp_col_const(0, F.SIG_NE_INT, 2),
                         real_lt(3, 2.5)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 2999])
@pytest.mark.parametrize("name", sorted(FILTERS))
def test_filters(engine, n, name):
    """0, 1 and 2 conjuncts over int and real columns; column 3 is absent in
    every fifth row and takes a non-NULL default that passes the filter"""
    raw = region_bytes([filt_row(i) for i in range(n)])
    ds = tikv_amd.DagSelect(filt_cols(b"\x08" + T.var_i64(-7)))
    if FILTERS[name]():
        ds = ds.where(*FILTERS[name]())
    req = (ds.hash_agg([tikv_amd.count_star(), tikv_amd.sum_col(4, decimal=2),
                      tikv_amd.max_col(1)], tikv_amd.Expr().col(0)).build())
    res, _ = one_region(engine, req, raw, 4)
    assert res[0] == "ok"


# ---- decimal scaling and its errors --------------------------------------
def dec_rows(n, odd_cell):
    """key, filter column (row 40 is the only one with 1), decimal cells of
    frac 0..2; row 40 carries odd_cell instead"""
    rows = []
    for i in range(n):
        v = cell_int(1, i % 5) + cell_int(2, 1 if i == 40 else 0)
        v += odd_cell if i == 40 else cell_dec(3, i * 31 - 2000, i % 3)
        rows.append(v)
    return region_bytes(rows)


def dec_req(keep_row_40):
    cols = [tikv_amd.Col(1), tikv_amd.Col(2),
            tikv_amd.Col(3, tp=F.TP_NEWDECIMAL, decimal=2)]
    sig = F.SIG_GE_INT if keep_row_40 else F.SIG_LT_INT
    return (tikv_amd.DagSelect(cols)
            .where(tikv_amd.cmp_col_const(1, sig, 0 if keep_row_40 else 1))
            .hash_agg([tikv_amd.count_star(), tikv_amd.sum_col(2, decimal=2)],
                      tikv_amd.Expr().col(0)).build())


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 777])
def test_decimal_frac_below_target(engine, n):
    """cells of frac 0, 1 and 2 under a target frac of 2: scaled by 100, 10
    and 1"""
    raw = dec_rows(n, cell_dec(3, 123, 1))
    res, builds = one_region(engine, dec_req(True), raw, 3)
    assert res[0] == "ok" and builds == 3


ODD_CELLS = {"frac-above-target": cell_dec(3, 12345, 3),
             "int-cell": cell_int(3, 77)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ODD_CELLS))
def test_bad_decimal_on_kept_row_is_an_error(engine, name):
    """a cell with more fraction digits than the target, or an int cell
    under sum(decimal), fails the request when its row is kept. The oracle
    adds a frac-3 cell into a frac-2 sum without complaint where the engine
    has always refused to: no oracle leg for that cell."""
    raw = dec_rows(257, ODD_CELLS[name])
    res, _ = one_region(engine, dec_req(True), raw, 3,
                        oracle=name != "frac-above-target")
    assert res[0] == "err" and "row parse error" in res[1]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ODD_CELLS))
def test_bad_decimal_on_filtered_row_is_not(engine, name):
    """the same cells on a row the filter removes: no error. The oracle
    decodes every scanned column before it filters and fails on the int
    cell where the scan kernels have always skipped it: no oracle leg for
    that cell."""
    raw = dec_rows(257, ODD_CELLS[name])
    res, _ = one_region(engine, dec_req(False), raw, 3,
                        oracle=name != "int-cell")
    assert res[0] == "ok" and res[2] == 5


# ---- rows resolved from the row bytes --------------------------------------
def v2_cells(cells):
    """row-v2 (small layout) of (id, int | payload bytes) cells, ids
    ascending; a decimal payload is the datum without its flag byte"""
    body, ends = b"", []
    for _, v in cells:
        if isinstance(v, bytes):
            body += v
        elif 0 <= v <= 0xFF:
            body += bytes([v])
        elif 0 <= v <= 0xFFFF:
            body += v.to_bytes(2, "little")
        else:
            body += (v & (2**64 - 1)).to_bytes(8, "little")
        ends.append(len(body))
    out = bytes([128, 0, len(cells), 0, 0, 0])
    out += bytes(cid for cid, _ in cells)
    for e in ends:
        out += e.to_bytes(2, "little")
    return out + body


def wide_req(target):
    cols = [tikv_amd.Col(1), tikv_amd.Col(2, tp=F.TP_NEWDECIMAL, decimal=target)]
    return (tikv_amd.DagSelect(cols)
            .hash_agg([tikv_amd.count_star(),
                       tikv_amd.sum_col(1, decimal=target)],
                      tikv_amd.Expr().col(0)).build())


@pytest.mark.gpu
@pytest.mark.parametrize("n", [257, 2999])
def test_wide_decimals_every_20th_row(engine, n):
    """19..38-digit values stay ROWPARSE and resolve from the row bytes; a
    wide row takes a global slot and adds in 256 bits. 1/20 of the rows is
    under the 1/8 cap, so the plane is kept: two builds. At n = 2999 group
    0 sums 150 wide values of both signs to 3.0e38 at frac 4, past i128:
    there the scan kernels and the oracle disagree (the oracle's 39-digit
    sum is the exact one), so that size has no oracle leg; the all-positive
    sum past i128 below has one."""
    rows = []
    for i in range(n):
        if i % 20 == 0:
            sc, fr = WIDE_VALS[(i // 20) % len(WIDE_VALS)]
        else:
            sc, fr = i * 1009 - 50_000, i % 5
        rows.append(cell_int(1, i % 4) + cell_dec(2, sc, fr))
    res, builds = one_region(engine, wide_req(4), region_bytes(rows), 3,
                             oracle=n != 2999)
    assert res[0] == "ok" and res[2] == min(n, 4) and builds == 2


@pytest.mark.gpu
def test_wide_decimal_sum_past_i128(engine):
    """150 rows of 10^37 over 3 groups: each group's sum, 5e38, is past
    i128 and lives in the ext limbs"""
    rows = []
    for i in range(2999):
        sc = 10**37 if i % 20 == 0 else i - 1500
        rows.append(cell_int(1, i % 3) + cell_dec(2, sc, 0))
    res, builds = one_region(engine, wide_req(0), region_bytes(rows), 3)
    assert res[0] == "ok" and res[2] == 3 and builds == 2


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 2999])
def test_mixed_row_formats(engine, n):
    """row-v2 rows on every 16th row among row-v1 rows, wide decimals on
    every 20th: 1/16 + 1/20 of the rows is under the 1/8 cap. Every group
    holds a cell of the target frac: the oracle reports a sum in the
    largest frac it met, the engine always in the target frac."""
    rows = []
    for i in range(n):
        if i % 16 == 5:
            rows.append(v2_cells([(1, i % 7), (2, enc_decimal(i * 3 - 99, 1)[1:])]))
        elif i % 20 == 0:
            sc, fr = WIDE_VALS[(i // 20) % len(WIDE_VALS)]
            rows.append(cell_int(1, i % 7) + cell_dec(2, sc, fr))
        else:
            rows.append(cell_int(1, i % 7) + cell_dec(2, i * 13 - 700, 2 + i % 3))
    res, builds = one_region(engine, wide_req(4), region_bytes(rows), 3)
    assert res[0] == "ok" and builds == 2


@pytest.mark.gpu
def test_two_regions_one_on_planes(engine):
    """region B is row-v2 throughout (tombstoned, stays on the scan kernel),
    region A reads planes; both feed one table"""
    rows_a = [cell_int(1, i % 9 - 4) + cell_int(3, i) for i in range(777)]
    rows_b = [v2_cells([(1, i % 12), (3, i)]) for i in range(300)]
    raw_a, raw_b = region_bytes(rows_a), region_bytes(rows_b)
    raw_all = region_bytes(rows_a + rows_b)
    cols = [tikv_amd.Col(1), tikv_amd.Col(3)]
    req = (tikv_amd.DagSelect(cols)
           .hash_agg([tikv_amd.count_star(), tikv_amd.sum_col(1)],
                     tikv_amd.Expr().col(0)).build())
    ra = engine.region_raw(*raw_a[:5])
    rb = engine.region_raw(*raw_b[:5])
    try:
        res, _ = hash_three_ways(engine, req, [ra, rb], raw_all, 3, launches=1)
        assert res[0] == "ok" and res[2] == 16
    finally:
        ra.close()
        rb.close()


# ---- budget, eligibility, cache ---------------------------------------------
@pytest.mark.gpu
def test_budget_zero_and_ineligible_plans_scan(engine):
    raw = region_bytes([filt_row(i) for i in range(777)])
    rgn = engine.region_raw(*raw[:5])
    try:
        grp = tikv_amd.Expr().col(0)
        ok = (tikv_amd.DagSelect(filt_cols())
              .hash_agg([tikv_amd.count_star(), tikv_amd.sum_col(1)], grp)
              .build())
        res, builds = hash_three_ways(engine, ok, [rgn], raw, 3, launches=0,
                                      budget_mb="0")
        assert res[0] == "ok" and builds == 0
        real = (tikv_amd.DagSelect(filt_cols())
                .hash_agg([tikv_amd.count_star(), tikv_amd.sum_real(3)], grp)
                .build())
        # sum(real) adds in arrival order: the two GPU legs may differ in the
        # last bit from each other, so only the path taken is asserted
        h0 = engine.hash_plane_launches()
        with env(COPR_NO_PLANES=None, COPR_PLANE_BUDGET_MB="64"):
            assert _run(engine, real, [rgn])[0] == "ok"
        assert engine.hash_plane_launches() == h0
        rpn = (tikv_amd.Expr().col(0).const_int(3).func(F.SIG_LT_INT, 2)
               .col(1).const_int(100).func(F.SIG_GT_INT, 2)
               .func(F.SIG_LOGICAL_OR, 2))
        req = (tikv_amd.DagSelect(filt_cols()).where(rpn)
               .hash_agg([tikv_amd.count_star(), tikv_amd.sum_col(1)], grp)
               .build())
        res, builds = hash_three_ways(engine, req, [rgn], raw, 3, launches=0)
        assert res[0] == "ok" and builds == 0
    finally:
        rgn.close()


@pytest.mark.gpu
def test_default_budget_on_generated_region(engine):
    """two planes, 18 B per row, fit the default cap of a generated cfg3
    region: its own value bytes"""
    g = tikv_amd.GenRegion(config_index=2, n_rows=2999, table_id=1)
    try:
        rgn = engine.region(g)
        try:
            res, builds = hash_three_ways(engine, cfg3_req(), [rgn],
                                          gen_raw(g), 5, budget_mb=None)
            assert res[0] == "ok" and builds == 2
        finally:
            rgn.close()
    finally:
        g.close()


@pytest.mark.gpu
def test_plane_cache_shared_with_simple_aggregates(engine):
    raw = cfg3_raw(2999, 64)
    rgn = engine.region_raw(*raw[:5])
    try:
        with env(COPR_NO_PLANES=None, COPR_PLANE_BUDGET_MB="64"):
            # a simple aggregate builds the key column's plane ...
            simple = (tikv_amd.DagSelect(cfg3_cols())
                      .where(tikv_amd.cmp_col_const(0, F.SIG_LT_INT, 3))
                      .simple_agg([tikv_amd.count_star()]).build())
            l0, b0 = engine.plane_stats()
            assert _run(engine, simple, [rgn])[0] == "ok"
            assert engine.plane_stats() == (l0 + 1, b0 + 1)
        # ... and a hash request grouping by it builds nothing new
        grp = (tikv_amd.DagSelect(cfg3_cols())
               .hash_agg([tikv_amd.count_star(), tikv_amd.max_col(0)],
                         tikv_amd.Expr().col(0)).build())
        res, builds = hash_three_ways(engine, grp, [rgn], raw, 3)
        assert res[0] == "ok" and builds == 0
        # the decimal column's plane is first built by a hash request ...
        res, builds = hash_three_ways(engine, cfg3_req(), [rgn], raw, 5)
        assert res[0] == "ok" and builds == 1
        # ... and a simple count(col) over it declines that plane: decimal
        # rows are ROWPARSE rows to k_plane_agg, as before decimals had a
        # state of their own. Same bytes as the scan kernel and the oracle.
        cnt = (tikv_amd.DagSelect(cfg3_cols())
               .simple_agg([tikv_amd.count_col(1)]).build())
        st0 = engine.plane_stats()
        with env(COPR_NO_PLANES=None, COPR_PLANE_BUDGET_MB="64"):
            r_dflt = _run(engine, cnt, [rgn])
        assert engine.plane_stats() == st0
        with env(COPR_NO_PLANES="1", COPR_PLANE_BUDGET_MB="64"):
            r_scan = _run(engine, cnt, [rgn])
        assert r_dflt == r_scan == _oracle(cnt, raw)
    finally:
        rgn.close()
