"""Decoded column planes (kernels.hip k_build_colplane /
k_plane_agg).

Simple aggregates with compare filters over int/real columns read a cached
per-(region, column) plane of decoded values + state bytes instead of the
row bytes. Every case here runs one request three ways and wants the same
bytes (or the same error) from all of them:
  - the plane path, asserted taken through the engine's launch counter;
  - COPR_NO_PLANES=1, the scan path as it was before planes existed;
  - the oracle.

Regions are a few hundred to ~3000 rows (more than one 256-thread block,
not a multiple of 64) plus the sizes 1, 63, 64, 65 and 257. Rows here are
short, so most cases raise the plane budget with COPR_PLANE_BUDGET_MB; the
default cap (half the region's value bytes) is exercised on generated
16-column regions.
"""
import contextlib
import ctypes as C
import os

import pytest

import tikv_amd
from tikv_amd import _ffi as F

import test_topn_stream as T
from test_topn_stream import cell_int, cell_null, cell_real, row_key
from test_dev_chunk import region_bytes
from test_oracle_exec import v2_row

SIZES = [1, 63, 64, 65, 257, 777, 2999]
U63 = 1 << 63


def cell_uint(col_id, v):
    return b"\x08" + T.var_i64(col_id) + b"\x09" + T.var_u64(v)


@contextlib.contextmanager
def env(**kv):
    """set (value) / unset (None) environment switches for one engine call"""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _run(engine, req, rgns):
    try:
        data, n, _ = engine.dag_run(req, rgns)
        return ("ok", data, n)
    except RuntimeError as e:
        return ("err", str(e))


def _oracle(req, raw):
    k, ko, v, vo, n = raw[:5]
    try:
        data, rows = T._orc().dag_run(req, k, ko, v, vo, n)
        return ("ok", data, rows)
    except RuntimeError:
        return ("err",)


def three_ways(engine, req, rgns, oracle_raw, plane=True, budget_mb="64"):
    """plane path / COPR_NO_PLANES=1 / oracle on the same request. plane =
    how many of the regions must take the plane path (True = all, False =
    none). Returns (result, plane launches, planes built)."""
    want = len(rgns) if plane is True else int(plane)
    l0, b0 = engine.plane_stats()
    with env(COPR_NO_PLANES=None, COPR_PLANE_BUDGET_MB=budget_mb):
        r_plane = _run(engine, req, rgns)
    l1, b1 = engine.plane_stats()
    with env(COPR_NO_PLANES="1", COPR_PLANE_BUDGET_MB=budget_mb):
        r_scan = _run(engine, req, rgns)
    l2, b2 = engine.plane_stats()
    assert (l2, b2) == (l1, b1), "COPR_NO_PLANES=1 still used planes"
    assert l1 - l0 == want, "plane launches %d, expected %d" % (l1 - l0, want)
    assert r_plane == r_scan
    r_orc = _oracle(req, oracle_raw)
    if r_orc[0] == "ok":
        assert r_plane == r_orc
    else:
        assert r_plane[0] == "err"
    return r_plane, l1 - l0, b1 - b0


def one_region(engine, req, raw, **kw):
    k, ko, v, vo, n, keep = raw
    rgn = engine.region_raw(k, ko, v, vo, n)
    try:
        return three_ways(engine, req, [rgn], raw, **kw)
    finally:
        rgn.close()


# ---- fixtures: five int columns with NULLs, a sometimes-missing column and
# an unsigned column whose values sit above 2^63 -------------------------
def basic_row(i, n):
    v = cell_int(1, (i * 37) % 100 - 50)
    v += cell_null(2) if i % 7 == 0 else cell_int(2, i * 11 - 500)
    if i % 5 != 0:
        v += cell_int(3, (i * 13) % 64 - 32)
    v += cell_uint(4, U63 + (i * 7) % 1000)
    v += cell_int(5, i - n // 2)
    return v


_RAW = {}


def basic_raw(n):
    if n not in _RAW:
        _RAW[n] = region_bytes([basic_row(i, n) for i in range(n)])
    return _RAW[n]


def basic_cols(default3=None):
    return [tikv_amd.Col(1), tikv_amd.Col(2),
            tikv_amd.Col(3, default_val=default3),
            tikv_amd.Col(4, flag=F.FLAG_UNSIGNED), tikv_amd.Col(5)]


def count_req(cols, *conds):
    return (tikv_amd.DagSelect(cols).where(*conds)
            .simple_agg([tikv_amd.count_star()]).build())


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("off,const", [(0, 3), (2, -5), (4, 10)])
def test_filter_count_column_position(engine, n, off, const):
    """int filter + count(*), filter column first / middle / last in the
    row. The middle column is missing in every fifth row (NULL default)."""
    req = count_req(basic_cols(), tikv_amd.cmp_col_const(off, F.SIG_LT_INT, const))
    res, _, _ = one_region(engine, req, basic_raw(n))
    assert res[0] == "ok"


@pytest.mark.gpu
@pytest.mark.parametrize("sig", [F.SIG_LT_INT, F.SIG_LE_INT, F.SIG_GT_INT,
                                 F.SIG_GE_INT, F.SIG_EQ_INT, F.SIG_NE_INT])
def test_all_compare_kinds(engine, sig):
    """six comparers over a column with NULL cells (col 2), const on an
    exact hit (row 50: 50 * 11 - 500 = 50)"""
    req = count_req(basic_cols(), tikv_amd.cmp_col_const(1, sig, 50))
    res, _, _ = one_region(engine, req, basic_raw(777))
    assert res[0] == "ok"


@pytest.mark.gpu
def test_extreme_constants_and_values(engine):
    """the filter+count kernel folds comparer and constant into one range
    test on the host: every comparer against the ends of the signed and of
    the unsigned range, over values that sit on those ends, with a missing
    column whose default is such an end"""
    i_min, i_max, u_max = -(1 << 63), (1 << 63) - 1, (1 << 64) - 1
    sv = [i_min, i_min + 1, -1, 0, 1, i_max - 1, i_max]
    uv = [0, 1, i_max, U63, u_max - 1, u_max]
    rows = []
    for i in range(300):
        v = cell_int(1, sv[i % len(sv)])
        if i % 4:
            v += cell_uint(2, uv[i % len(uv)])
        rows.append(v)
    raw = region_bytes(rows)
    k, ko, v, vo, n, keep = raw
    rgn = engine.region_raw(k, ko, v, vo, n)
    sigs = (F.SIG_LT_INT, F.SIG_LE_INT, F.SIG_GT_INT, F.SIG_GE_INT,
            F.SIG_EQ_INT, F.SIG_NE_INT)
    try:
        for sig in sigs:
            for c in (i_min, -1, 0, i_max):
                cols = [tikv_amd.Col(1), tikv_amd.Col(2, flag=F.FLAG_UNSIGNED)]
                req = count_req(cols, tikv_amd.cmp_col_const(0, sig, c))
                res, _, _ = three_ways(engine, req, [rgn], raw)
                assert res[0] == "ok", (sig, c)
            for c in (0, U63, u_max):
                for dflt in (None, b"\x09" + T.var_u64(u_max), b"\x09\x00"):
                    cols = [tikv_amd.Col(1),
                            tikv_amd.Col(2, flag=F.FLAG_UNSIGNED,
                                         default_val=dflt)]
                    req = count_req(cols, tikv_amd.cmp_col_const(
                        1, sig, c, unsigned_const=True))
                    res, _, _ = three_ways(engine, req, [rgn], raw)
                    assert res[0] == "ok", (sig, c, dflt)
    finally:
        rgn.close()


@pytest.mark.gpu
@pytest.mark.parametrize("default3", [None, b"\x08" + T.var_i64(-7)])
def test_missing_column_defaults(engine, default3):
    """column missing with a NULL default and with a value default: one
    cached plane serves both because ABSENT stays its own state"""
    raw = basic_raw(777)
    k, ko, v, vo, n, keep = raw
    rgn = engine.region_raw(k, ko, v, vo, n)
    try:
        builds = 0
        for d in (default3, None, b"\x08" + T.var_i64(20)):
            req = count_req(basic_cols(d),
                            tikv_amd.cmp_col_const(2, F.SIG_LT_INT, 0))
            res, _, b = three_ways(engine, req, [rgn], raw)
            assert res[0] == "ok"
            builds += b
        assert builds == 1
    finally:
        rgn.close()


@pytest.mark.gpu
def test_unsigned_column_unsigned_const(engine):
    sel = tikv_amd.cmp_col_const(3, F.SIG_GT_INT, U63 + 500, unsigned_const=True)
    res, _, _ = one_region(engine, count_req(basic_cols(), sel), basic_raw(777))
    assert res[0] == "ok"
    # signed constant against the unsigned column (mixed-sign compare)
    sel = tikv_amd.cmp_col_const(3, F.SIG_GT_INT, -1)
    one_region(engine, count_req(basic_cols(), sel), basic_raw(257))


@pytest.mark.gpu
def test_null_constant(engine):
    sel = tikv_amd.Expr().col(0).const_null().func(F.SIG_LT_INT, 2)
    res, _, _ = one_region(engine, count_req(basic_cols(), sel), basic_raw(257))
    assert res[0] == "ok"


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 2999])
def test_two_filters(engine, n):
    """two ANDed conjuncts on different columns, one of them with NULLs"""
    req = (tikv_amd.DagSelect(basic_cols())
           .where(tikv_amd.cmp_col_const(0, F.SIG_GT_INT, -20),
                  tikv_amd.cmp_col_const(1, F.SIG_LE_INT, 4000))
           .simple_agg([tikv_amd.count_star(), tikv_amd.sum_col(4)]).build())
    res, _, _ = one_region(engine, req, basic_raw(n))
    assert res[0] == "ok"


@pytest.mark.gpu
def test_real_filter_column(engine):
    xs = [None if i % 9 == 0 else (i % 41) * 0.75 - 12.5 for i in range(777)]
    raw = T.region_real(xs)
    cols = [tikv_amd.Col(1), tikv_amd.Col(2, tp=F.TP_DOUBLE)]
    for sig in (F.SIG_LT_REAL, F.SIG_GE_REAL, F.SIG_EQ_REAL):
        sel = tikv_amd.Expr().col(1).const_real(2.5).func(sig, 2)
        req = (tikv_amd.DagSelect(cols).where(sel)
               .simple_agg([tikv_amd.count_star(),
                            tikv_amd.count_col(1)]).build())
        res, _, _ = one_region(engine, req, raw)
        assert res[0] == "ok"


@pytest.mark.gpu
def test_type_mismatch_errors_like_the_scan(engine):
    """an int cell under a real comparer is an error at query time, on both
    paths, although the plane was built without knowing the comparer"""
    raw = basic_raw(257)
    cols = [tikv_amd.Col(1, tp=F.TP_DOUBLE), tikv_amd.Col(2)]
    sel = tikv_amd.Expr().col(0).const_real(2.5).func(F.SIG_LT_REAL, 2)
    req = (tikv_amd.DagSelect(cols).where(sel)
           .simple_agg([tikv_amd.count_star()]).build())
    res, _, _ = one_region(engine, req, raw)
    assert res[0] == "err" and "row parse error" in res[1]


AGGS = [tikv_amd.count_star(), tikv_amd.count_col(1), tikv_amd.sum_col(1),
        tikv_amd.min_col(2), tikv_amd.max_col(2),
        tikv_amd.max_col(3, flag=F.FLAG_UNSIGNED), tikv_amd.min_col(4)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("filtered", [False, True])
def test_aggregates(engine, n, filtered):
    """count(col), sum, min, max (signed and unsigned) over columns with
    NULL and missing cells, with and without a filter; 7 aggregates take
    the wide kernel instance"""
    ds = tikv_amd.DagSelect(basic_cols())
    if filtered:
        ds = ds.where(tikv_amd.cmp_col_const(0, F.SIG_GE_INT, 0))
    res, _, _ = one_region(engine, ds.simple_agg(AGGS).build(), basic_raw(n))
    assert res[0] == "ok"


@pytest.mark.gpu
@pytest.mark.parametrize("naggs", [1, 2, 3, 4])
def test_aggregate_counts_per_kernel_instance(engine, naggs):
    """every NAGGS instantiation of the plane kernel, no filter"""
    aggs = [tikv_amd.sum_col(4), tikv_amd.max_col(1), tikv_amd.count_col(2),
            tikv_amd.min_col(0)][:naggs]
    req = tikv_amd.DagSelect(basic_cols()).simple_agg(aggs).build()
    res, _, _ = one_region(engine, req, basic_raw(777))
    assert res[0] == "ok"


@pytest.mark.gpu
@pytest.mark.parametrize("sign", [1, -1])
def test_sum_reaches_i128_carry(engine, sign):
    """values near +-2^62: three rows already leave i64, 700 rows carry far
    into the high limb"""
    big = (1 << 62) - 3
    rows = [cell_int(1, i) + cell_int(2, sign * (big - i)) for i in range(700)]
    rows += [cell_int(1, 1000) + cell_int(2, -sign * 5)]
    raw = region_bytes(rows)
    cols = [tikv_amd.Col(1), tikv_amd.Col(2)]
    req = (tikv_amd.DagSelect(cols)
           .where(tikv_amd.cmp_col_const(0, F.SIG_NE_INT, 13))
           .simple_agg([tikv_amd.sum_col(1), tikv_amd.count_star()]).build())
    res, _, _ = one_region(engine, req, raw)
    assert res[0] == "ok"


# ---- rows the directory cannot express ---------------------------------
def odd_rows(n):
    """v1 rows mixed with row-v2 rows, empty rows, a row whose filter cell
    sits past byte 253 and rows carrying column ids above 16"""
    rows = []
    for i in range(n):
        m = i % 11
        if m == 0:      # v2; 200 in one byte is -56 for a signed column
            rows.append(bytes(v2_row([(1, i % 250), (3, 200), (5, i)])))
        elif m == 1:
            rows.append(b"")
        elif m == 2:
            rows.append(b"\x00")
        elif m == 3:    # long bytes cell first: later cells past offset 253
            rows.append(T.var_bytes_cell(9, b"x" * 300) + cell_int(1, i % 90)
                        + cell_int(3, i % 17) + cell_int(5, i))
        elif m == 4:    # ids above 16 around the columns of interest
            rows.append(cell_int(1, -i) + cell_int(20, i) + cell_int(3, 7)
                        + cell_int(40, -i) + cell_int(5, i))
        else:
            rows.append(cell_int(1, i % 90 - 45) + cell_int(3, i % 17)
                        + cell_int(5, i))
    return rows


def odd_cols(flag3=0):
    return [tikv_amd.Col(1), tikv_amd.Col(3, flag=flag3), tikv_amd.Col(5),
            tikv_amd.Col(20)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 2999])
@pytest.mark.parametrize("no_dir", [False, True])
def test_rowparse_and_walk_rows(engine, n, no_dir):
    """ROWPARSE rows (v2: the decode needs the request's signedness) and
    the sequential-walk fallback, with and without a cell directory"""
    raw = region_bytes(odd_rows(n))
    k, ko, v, vo, nkv, keep = raw
    with env(COPR_NO_DIR="1" if no_dir else None):
        rgn = engine.region_raw(k, ko, v, vo, nkv)
    try:
        builds = 0
        # signed, then unsigned view of column 3 over the same plane: the
        # v2 cell 200 reads as -56 or 200
        for flag3, const in ((0, 0), (F.FLAG_UNSIGNED, 100)):
            req = (tikv_amd.DagSelect(odd_cols(flag3))
                   .where(tikv_amd.cmp_col_const(1, F.SIG_LT_INT, const,
                                                 unsigned_const=bool(flag3)))
                   .simple_agg([tikv_amd.count_star(), tikv_amd.sum_col(0),
                                tikv_amd.max_col(2)]).build())
            res, _, b = three_ways(engine, req, [rgn], raw)
            assert res[0] == "ok"
            builds += b
        assert builds == 3          # columns 3, 1 and 5, each built once
        # column id 20: no directory plane. With a directory the scan path
        # walks for this request while planes follow the directory, so the
        # region stays on the scan path; without one the plane is built by
        # walking.
        req = (tikv_amd.DagSelect(odd_cols())
               .where(tikv_amd.cmp_col_const(3, F.SIG_GT_INT, 100))
               .simple_agg([tikv_amd.count_star()]).build())
        res, _, _ = three_ways(engine, req, [rgn], raw, plane=no_dir)
        assert res[0] == "ok"
    finally:
        rgn.close()


@pytest.mark.gpu
@pytest.mark.parametrize("no_dir", [False, True])
def test_malformed_row_same_error(engine, no_dir):
    """a row whose first cell carries an unknown datum flag: every path
    reports the same storage error"""
    rows = [basic_row(i, 300) for i in range(300)]
    rows[131] = b"\x08\x02\x0f\x01" + rows[131]
    raw = region_bytes(rows)
    k, ko, v, vo, n, keep = raw
    with env(COPR_NO_DIR="1" if no_dir else None):
        rgn = engine.region_raw(k, ko, v, vo, n)
    try:
        for off in (0, 4):
            req = count_req(basic_cols(),
                            tikv_amd.cmp_col_const(off, F.SIG_LT_INT, 3))
            res, _, _ = three_ways(engine, req, [rgn], raw)
            assert res[0] == "err" and "row parse error" in res[1]
    finally:
        rgn.close()


@pytest.mark.gpu
@pytest.mark.parametrize("no_dir", [False, True])
def test_malformed_cell_after_filter_column(engine, no_dir):
    """garbage after the last requested column is never parsed: all paths
    succeed with the same count; a request that must walk past it fails on
    all paths alike"""
    rows = [cell_int(1, i % 50) + cell_int(2, i) for i in range(300)]
    rows[77] += b"\x08\x06\x0f\x01"        # col 3, unknown datum flag
    raw = region_bytes(rows)
    k, ko, v, vo, n, keep = raw
    cols = [tikv_amd.Col(1), tikv_amd.Col(2), tikv_amd.Col(3)]
    with env(COPR_NO_DIR="1" if no_dir else None):
        rgn = engine.region_raw(k, ko, v, vo, n)
    try:
        req = count_req(cols[:2], tikv_amd.cmp_col_const(1, F.SIG_LT_INT, 100))
        res, _, _ = three_ways(engine, req, [rgn], raw)
        assert res[0] == "ok"
        req = count_req(cols, tikv_amd.cmp_col_const(2, F.SIG_LT_INT, 100))
        res, _, _ = three_ways(engine, req, [rgn], raw)
        assert res[0] == "err"
    finally:
        rgn.close()


# ---- caching, budget, lifetime -----------------------------------------
@pytest.mark.gpu
def test_plane_cached_across_requests(engine):
    raw = basic_raw(2999)
    k, ko, v, vo, n, keep = raw
    rgn = engine.region_raw(k, ko, v, vo, n)
    try:
        req = count_req(basic_cols(), tikv_amd.cmp_col_const(0, F.SIG_LT_INT, 3))
        _, launches, builds = three_ways(engine, req, [rgn], raw)
        assert (launches, builds) == (1, 1)
        # a different request on the same column: no rebuild
        req = (tikv_amd.DagSelect(basic_cols())
               .where(tikv_amd.cmp_col_const(0, F.SIG_GE_INT, -10))
               .simple_agg([tikv_amd.max_col(0)]).build())
        _, launches, builds = three_ways(engine, req, [rgn], raw)
        assert (launches, builds) == (1, 0)
        # another column: a second plane
        req = count_req(basic_cols(), tikv_amd.cmp_col_const(4, F.SIG_LT_INT, 3))
        _, launches, builds = three_ways(engine, req, [rgn], raw)
        assert (launches, builds) == (1, 1)
    finally:
        rgn.close()


@pytest.mark.gpu
def test_budget_zero_falls_back(engine):
    req = count_req(basic_cols(), tikv_amd.cmp_col_const(0, F.SIG_LT_INT, 3))
    res, _, builds = one_region(engine, req, basic_raw(777), plane=False,
                                budget_mb="0")
    assert res[0] == "ok" and builds == 0


def gen_raw(g):
    return (g.keys, g.key_offs, g.vals, g.val_offs, g.n_kv)


@pytest.mark.gpu
def test_default_budget_on_wide_rows(engine):
    """the default cap, half the region's value bytes, admits planes for a
    16-column generated region: the flagship shape, scaled down"""
    g = tikv_amd.GenRegion(config_index=1, n_rows=2999, table_id=1)
    try:
        rgn = engine.region(g)
        try:
            cols = [tikv_amd.Col(i) for i in range(1, 17)]
            req = count_req(cols, tikv_amd.cmp_col_const(3, F.SIG_LT_INT,
                                                         -800_000_000))
            res, _, builds = three_ways(engine, req, [rgn], gen_raw(g),
                                        budget_mb=None)
            assert res[0] == "ok" and builds == 1
        finally:
            rgn.close()
    finally:
        g.close()


@pytest.mark.gpu
def test_two_regions_one_eligible(engine):
    """region B is row-v2 throughout: its plane would be all ROWPARSE, so
    it stays on the scan path while region A uses its plane; one result"""
    na, nb = 777, 300
    rows_a = [cell_int(1, i % 90 - 45) + cell_int(3, i) for i in range(na)]
    rows_b = [bytes(v2_row([(1, i % 100), (3, i)])) for i in range(nb)]
    raw_a, raw_b = region_bytes(rows_a), region_bytes(rows_b)
    raw_all = region_bytes(rows_a + rows_b)
    cols = [tikv_amd.Col(1), tikv_amd.Col(3)]
    req = (tikv_amd.DagSelect(cols)
           .where(tikv_amd.cmp_col_const(0, F.SIG_LT_INT, 20))
           .simple_agg([tikv_amd.count_star(), tikv_amd.sum_col(1)]).build())
    ra = engine.region_raw(*raw_a[:5])
    rb = engine.region_raw(*raw_b[:5])
    try:
        res, _, _ = three_ways(engine, req, [ra, rb], raw_all, plane=1)
        assert res[0] == "ok"
        # the verdict on region B is remembered: no second build attempt
        _, _, builds = three_ways(engine, req, [ra, rb], raw_all, plane=1)
        assert builds == 0
    finally:
        ra.close()
        rb.close()


@pytest.mark.gpu
def test_mvcc_built_region(engine):
    g = tikv_amd.GenRegion(config_index=1, n_rows=3000, table_id=1, row_format=3)
    try:
        o_keys, o_ko, o_vals, o_vo, o_n = T._orc().mvcc_filter(
            g.keys, g.key_offs, g.vals, g.val_offs, g.n_kv, 1000)
        kb = (C.c_uint8 * max(len(o_keys), 1)).from_buffer_copy(o_keys or b"\0")
        vb = (C.c_uint8 * max(len(o_vals), 1)).from_buffer_copy(o_vals or b"\0")
        raw = (C.cast(kb, C.POINTER(C.c_uint8)), (C.c_uint64 * len(o_ko))(*o_ko),
               C.cast(vb, C.POINTER(C.c_uint8)), (C.c_uint64 * len(o_vo))(*o_vo),
               o_n)
        rgn = engine.region_mvcc(g, 1000)
        try:
            cols = [tikv_amd.Col(i) for i in range(1, 17)]
            req = (tikv_amd.DagSelect(cols)
                   .where(tikv_amd.cmp_col_const(3, F.SIG_LT_INT, 0))
                   .simple_agg([tikv_amd.count_star(),
                                tikv_amd.max_col(5)]).build())
            res, _, _ = three_ways(engine, req, [rgn], raw, budget_mb=None)
            assert res[0] == "ok"
        finally:
            rgn.close()
    finally:
        g.close()


@pytest.mark.gpu
def test_region_close_then_new_region(engine):
    """planes die with their region; a new region on the same engine
    builds its own and never sees the old values"""
    req = count_req(basic_cols(), tikv_amd.cmp_col_const(0, F.SIG_LT_INT, 3))
    for it, n in enumerate((777, 257, 777)):
        rows = [basic_row(i + 100 * it, 4000) for i in range(n)]
        res, launches, builds = one_region(engine, req, region_bytes(rows))
        assert res[0] == "ok" and (launches, builds) == (1, 1)


# ---- plans that must not take the plane path ---------------------------
@pytest.mark.gpu
def test_ineligible_plans_stay_on_scan_path(engine):
    raw = basic_raw(2999)
    cols = basic_cols()
    hash_req = (tikv_amd.DagSelect(cols)
                .where(tikv_amd.cmp_col_const(0, F.SIG_LT_INT, 3))
                .hash_agg([tikv_amd.count_star()], tikv_amd.Expr().col(2))
                .build())
    k, ko, v, vo, n, keep = raw
    rgn = engine.region_raw(k, ko, v, vo, n)
    try:
        l0, _ = engine.plane_stats()
        with env(COPR_NO_PLANES=None, COPR_PLANE_BUDGET_MB="64"):
            gd, gn, _ = engine.dag_run(hash_req, [rgn])
        od, on = T._orc().dag_run(hash_req, k, ko, v, vo, n)
        assert gn == on
        assert set(T.split_rows(gd, 2)) == set(T.split_rows(od, 2))
        assert engine.plane_stats()[0] == l0
        # RPN predicate: col0 < 3 OR col4 > 100
        rpn = (tikv_amd.Expr().col(0).const_int(3).func(F.SIG_LT_INT, 2)
               .col(4).const_int(100).func(F.SIG_GT_INT, 2)
               .func(F.SIG_LOGICAL_OR, 2))
        req = (tikv_amd.DagSelect(cols).where(rpn)
               .simple_agg([tikv_amd.count_star()]).build())
        res, _, _ = three_ways(engine, req, [rgn], raw, plane=False)
        assert res[0] == "ok"
        # no column referenced at all: nothing a plane could serve
        req = tikv_amd.DagSelect(cols).simple_agg([tikv_amd.count_star()]).build()
        res, _, _ = three_ways(engine, req, [rgn], raw, plane=False)
        assert res[0] == "ok"
    finally:
        rgn.close()
    # index scan + simple agg
    g = tikv_amd.GenRegion(config_index=4, n_rows=2999, table_id=1)
    try:
        rgn = engine.region(g)
        try:
            icols = [tikv_amd.Col(1), tikv_amd.Col(2),
                     tikv_amd.Col(-1, pk_handle=True)]
            req = (tikv_amd.DagSelect(icols, index=True)
                   .where(tikv_amd.cmp_col_const(1, F.SIG_GE_INT, 0))
                   .simple_agg([tikv_amd.count_star(),
                                tikv_amd.sum_col(1)]).build())
            res, _, _ = three_ways(engine, req, [rgn], gen_raw(g), plane=False)
            assert res[0] == "ok"
        finally:
            rgn.close()
    finally:
        g.close()
