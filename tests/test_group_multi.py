"""Hash aggregation over two to four int group-by columns on the GPU
(DESIGN.md §9j).

The oracle takes one group-by expression, so the references are (1) the
oracle on an equivalent single-key request, byte for byte, and (2) the Python
group-by of group_multi_util.py, itself pinned against the oracle by
test_group_multi_ref_cpu.py. Group order is not part of parity: rows compare
as multisets. Engine.hash_plane_launches() and Engine.group_stats() tell the
route (k_plane_hash or the sorted pipeline) and the key source (planes or row
bytes) a request took.
"""
import random

import pytest

import tikv_amd
from tikv_amd import _ffi as F

from group_multi_util import (Key, build_region, group_ref, orc,
                              region_of_bytes, row_v1, rows_of)
from test_col_planes import env
from test_hash_planes import split_datums
from test_topn_stream import cell_real, var_bytes_cell
from test_wide_decimal import cell, enc_decimal
from topn_multi_util import (INT64_MAX, INT64_MIN, U64, cell_int, int_datum,
                             uint_datum)

pytestmark = pytest.mark.gpu

UNSUP = "copr_dag_run: %d " % F.COPR_ERR_UNSUPPORTED
AGGS = [("count_star",), ("count", 5), ("max", 5), ("min", 5)]


def E(off):
    return tikv_amd.Expr().col(off)


def agg_defs(v_off=4):
    return [tikv_amd.count_star(), tikv_amd.count_col(v_off),
            tikv_amd.max_col(v_off), tikv_amd.min_col(v_off)]


def COLS(d=None, uns=()):
    """columns 1..4 are keys (offsets 0..3), column 5 the aggregated value"""
    d = d or {}
    return [tikv_amd.Col(c, flag=F.FLAG_UNSIGNED if c in uns else 0,
                         default_val=d.get(c)) for c in (1, 2, 3, 4, 5)]


class Rgn:
    def __init__(self, engine, rows, unsigned=(), v2=False, tail=None):
        self.host = build_region(rows, unsigned=unsigned, v2=v2, tail=tail)
        self.dev = engine.region_raw(*self.host[:5])

    def close(self):
        self.dev.close()


def genv(**kw):
    """the switches a request here runs under: planes on with a budget that
    admits these small regions' planes, the default dictionary size"""
    base = {"COPR_NO_PLANES": None, "COPR_GK_SLOTS": None,
            "COPR_PLANE_BUDGET_MB": "64"}
    base.update(kw)
    return env(**base)


def run(engine, req, rgn, n_cols, route=None, source=None, **envkw):
    """rows of one multi-key request, sorted. route: "plane" / "sorted";
    source: "plane" / "rows"; both asserted from the counters when given."""
    h0, g0 = engine.hash_plane_launches(), engine.group_stats()
    with genv(**envkw):
        data, n, _ = engine.dag_run(req, [rgn.dev])
    h1, g1 = engine.hash_plane_launches(), engine.group_stats()
    assert g1[0] == g0[0] + 1, "request did not take the multi-key path"
    if route == "plane":
        assert h1 > h0, "k_plane_hash did not run"
    elif route == "sorted":
        assert h1 == h0, "k_plane_hash ran on the sorted route"
    if source == "plane":
        assert g1[3] == g0[3], "a key was read from the row bytes"
    elif source == "rows":
        assert g1[3] > g0[3], "no key was read from the row bytes"
    rows = rows_of(data, n_cols)
    assert len(rows) == n
    return rows


def two_key_req(cols, keys=(0, 1), cond=None, aggs=None, slow=False, limit=None):
    ds = tikv_amd.DagSelect(cols)
    if cond is not None:
        ds = ds.where(cond)
    f = ds.slow_hash_agg if slow else ds.hash_agg
    ds = f(aggs or agg_defs(), [E(k) for k in keys])
    if limit is not None:
        ds = ds.limit(limit)
    return ds.build()


def mixed_rows(n, seed=1):
    rng = random.Random(seed)
    return [{1: rng.choice([None, 0, 1, 2, 3]), 2: rng.choice([None, 0, 5]),
             3: i % 4, 4: 7, 5: rng.choice([None, -3, 8, 10**11])}
            for i in range(n)]


# ---- sizes ------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 255, 257, 513, 1025])
def test_row_counts(engine, n):
    rows = mixed_rows(n, seed=n)
    rgn = Rgn(engine, rows)
    try:
        want = group_ref(rows, [Key(1), Key(2)], AGGS)
        got = run(engine, two_key_req(COLS()), rgn, 6, route="plane",
                  source="plane")
        assert got == want
        assert engine.group_stats()[1] == len(want)
    finally:
        rgn.close()


def test_empty_region_and_filter_dropping_every_row(engine):
    rgn = Rgn(engine, [])
    try:
        assert run(engine, two_key_req(COLS()), rgn, 6) == []
    finally:
        rgn.close()
    rows = mixed_rows(300)
    rgn = Rgn(engine, rows)
    try:
        cond = tikv_amd.cmp_col_const(2, F.SIG_GT_INT, 99)
        for kw in ({}, {"COPR_NO_PLANES": "1"}):
            assert run(engine, two_key_req(COLS(), cond=cond), rgn, 6, **kw) == []
        # the dropped rows' tuples still took dictionary slots
        assert engine.group_stats()[1] == len(
            group_ref(rows, [Key(1), Key(2)], AGGS))
    finally:
        rgn.close()


# ---- tuples -----------------------------------------------------------------
def test_tuple_edge_cases(engine):
    ab = [(1, 2), (2, 1), (1, 2), (0, None), (None, 0), (None, None), (0, 0),
          (INT64_MIN, -1), (-1, INT64_MIN), (INT64_MAX, 0), (0, INT64_MAX),
          (INT64_MIN, INT64_MIN), (INT64_MAX, INT64_MAX), (None, None),
          (0, None)]
    ab += [(9, b) for b in range(40)]        # many tuples share the first key
    rows = [{1: a, 2: b, 5: i} for i, (a, b) in enumerate(ab)]
    rgn = Rgn(engine, rows)
    try:
        want = group_ref(rows, [Key(1), Key(2)], AGGS)
        assert len(want) == 12 + 40
        for kw in ({}, {"COPR_NO_PLANES": "1"}):
            assert run(engine, two_key_req(COLS()), rgn, 6, **kw) == want
    finally:
        rgn.close()


def test_unsigned_keys_and_shared_bit_patterns(engine):
    # column 1 signed, column 2 unsigned: -1 and 2^64-1, INT64_MIN and 2^63
    # are the same 64 bits and must come back in their own column's form
    sv = [-1, INT64_MIN, 0, None]
    uv = [U64, 2**63, 0, 2**63 + 5, None]
    rows = [{1: sv[i % 4], 2: uv[(i // 4) % 5], 5: i} for i in range(257)]
    rgn = Rgn(engine, rows, unsigned={2})
    try:
        cols = COLS(uns={2})
        for order in ((0, 1), (1, 0)):
            keys = [Key(1), Key(2, True)]
            keys = [keys[o] for o in order]
            want = group_ref(rows, keys, AGGS)
            assert len(want) == 20
            for kw in ({}, {"COPR_NO_PLANES": "1"}):
                got = run(engine, two_key_req(cols, keys=order), rgn, 6, **kw)
                assert got == want
    finally:
        rgn.close()


@pytest.mark.parametrize("offs", [(0, 1, 2), (0, 1, 2, 3), (2, 0, 2), (1, 1),
                                  (3, 2, 1, 0)])
def test_three_four_keys_and_a_column_named_twice(engine, offs):
    rows = mixed_rows(513, seed=3)
    rgn = Rgn(engine, rows)
    try:
        want = group_ref(rows, [Key(o + 1) for o in offs], AGGS)
        for kw, route in (({}, "plane"), ({"COPR_NO_PLANES": "1"}, "sorted")):
            got = run(engine, two_key_req(COLS(), keys=offs), rgn,
                      4 + len(offs), route=route, **kw)
            assert got == want
    finally:
        rgn.close()


# ---- dictionary growth --------------------------------------------------------
def test_dictionary_grows_and_retries(engine):
    rows = [{1: i % 20, 2: i // 20 if i % 3 else None, 5: i} for i in range(450)]
    rgn = Rgn(engine, rows)
    try:
        want = group_ref(rows, [Key(1), Key(2)], AGGS)
        assert len(want) >= 300
        g0 = engine.group_stats()
        small = run(engine, two_key_req(COLS()), rgn, 6, COPR_GK_SLOTS="16")
        g1 = engine.group_stats()
        assert g1[2] > g0[2], "a 16-slot dictionary did not grow"
        assert g1[1] == len(want)
        dflt = run(engine, two_key_req(COLS()), rgn, 6)
        assert engine.group_stats()[2] == g1[2], "the default size grew"
        assert small == want and dflt == want
        # and through the row-bytes source
        assert run(engine, two_key_req(COLS()), rgn, 6, COPR_GK_SLOTS="16",
                   COPR_NO_PLANES="1", source="rows") == want
    finally:
        rgn.close()


# ---- routes and sources ---------------------------------------------------------
def test_routes_and_sources_agree(engine):
    rows = mixed_rows(777, seed=5)
    want = group_ref(rows, [Key(1), Key(2)], AGGS)
    cond = tikv_amd.cmp_col_const(4, F.SIG_GT_INT, 0)
    want_f = group_ref(rows, [Key(1), Key(2)], AGGS,
                       keep=lambda r: r[5] is not None and r[5] > 0)
    v1 = Rgn(engine, rows)
    v2 = Rgn(engine, rows, v2=True)
    try:
        for c, w in ((None, want), (cond, want_f)):
            req = two_key_req(COLS(), cond=c)
            assert run(engine, req, v1, 6, route="plane", source="plane") == w
            assert run(engine, req, v1, 6, route="sorted", source="rows",
                       COPR_NO_PLANES="1") == w
            # row-v2: every plane would be ROWPARSE, so no plane anywhere
            assert run(engine, req, v2, 6, route="sorted", source="rows") == w
    finally:
        v1.close()
        v2.close()


def test_first_and_bit_ops_take_the_sorted_route(engine):
    """FIRST and bit operations are not k_plane_hash kinds. Column 3 is
    constant inside every (a, b) group, so FIRST has one answer."""
    rows = [{1: i % 3, 2: (i // 3) % 4 if i % 5 else None, 3: 0, 5: i}
            for i in range(513)]
    for r in rows:
        r[3] = 100 + r[1] * 10 + (r[2] if r[2] is not None else 9)
    rgn = Rgn(engine, rows)
    try:
        aggs = [tikv_amd.count_star(), tikv_amd.first_col(2),
                tikv_amd.bit_op(F.AGG_BIT_OR, 4)]
        groups = {}
        for r in rows:
            groups.setdefault((r[1], r[2]), []).append(r)
        want = []
        for (a, b), rs in groups.items():
            bor = 0
            for r in rs:
                bor |= r[5]
            want.append(((3, len(rs)), (3, rs[0][3]), (4, bor), (3, a),
                         (0, None) if b is None else (3, b)))
        want = sorted(want, key=repr)
        for kw, src in (({}, "plane"), ({"COPR_NO_PLANES": "1"}, "rows")):
            got = run(engine, two_key_req(COLS(), aggs=aggs), rgn, 5,
                      route="sorted", source=src, **kw)
            assert got == want
    finally:
        rgn.close()


@pytest.mark.parametrize("with_default", [False, True])
def test_absent_key_cells_read_from_the_plane(engine, with_default):
    rows = mixed_rows(513, seed=8)
    for i, r in enumerate(rows):
        if i % 4 == 1:
            del r[1]
        if i % 6 == 2:
            del r[2]
    d = {1: int_datum(2), 2: uint_datum(2**63 + 1)} if with_default else {}
    keys = [Key(1, False, 2 if with_default else None),
            Key(2, True, 2**63 + 1 if with_default else None)]
    rgn = Rgn(engine, rows, unsigned={2})
    try:
        want = group_ref(rows, keys, AGGS)
        req = two_key_req(COLS(d, uns={2}))
        assert run(engine, req, rgn, 6, route="plane", source="plane") == want
        assert run(engine, req, rgn, 6, source="rows",
                   COPR_NO_PLANES="1") == want
    finally:
        rgn.close()


def test_plane_state_outside_the_three_reruns_on_row_bytes(engine):
    """a real cell in an int key column: the plane holds PST_REAL there, stage
    1 raises its fallback flag and reruns with every key from the row bytes,
    whose verdict on that cell, a row parse error, is the result, whether the
    filter keeps the row or not"""
    rows = mixed_rows(300, seed=9)
    rgn_rows = []
    for i, r in enumerate(rows):
        if i == 200:
            rgn_rows.append(cell_int(1, 1) + cell_real(2, 1.5)
                            + row_v1({3: 0, 4: 7, 5: -3}))
        else:
            rgn_rows.append(row_v1(r))
    host = region_of_bytes(rgn_rows)
    dev = engine.region_raw(*host[:5])
    try:
        for cond in (None, tikv_amd.cmp_col_const(4, F.SIG_GT_INT, 0)):
            for kw in ({}, {"COPR_NO_PLANES": "1"}):
                g0 = engine.group_stats()
                with genv(**kw):
                    with pytest.raises(RuntimeError, match="row parse error"):
                        engine.dag_run(two_key_req(COLS(), cond=cond), [dev])
                g1 = engine.group_stats()
                assert g1[3] == g0[3] + 1 and g1[0] == g0[0]
    finally:
        dev.close()


# ---- the oracle on an equivalent single-key request ---------------------------------
def cell_dec(col_id, scaled, frac):
    return cell(col_id, enc_decimal(scaled, frac))


def _dec_cols():
    return COLS() + [tikv_amd.Col(6, tp=F.TP_NEWDECIMAL, decimal=2)]


def _all_aggs():
    """count(*), count(col), sum(int), avg(int), sum(decimal), max, min: 8
    aggregate datums per row"""
    return [tikv_amd.count_star(), tikv_amd.count_col(4), tikv_amd.sum_col(4),
            tikv_amd.avg_col(4), tikv_amd.sum_col(5, decimal=2),
            tikv_amd.max_col(4), tikv_amd.min_col(4)]


@pytest.mark.parametrize("filtered", [False, True])
def test_packed_key_against_the_oracle(engine, filtered):
    o = orc()
    n = 1025
    rows = [{1: (i * 7) % 13 - 6, 2: (i * 5) % 17, 5: (i * 31) % 101 - 50 if i % 9 else None}
            for i in range(n)]
    for r in rows:
        r[3] = r[1] * 1000 + r[2]
    rgn = Rgn(engine, rows,
              tail=lambda i: cell_dec(6, (i * 7919) % 200_003 - 100_000, 2))
    try:
        cond = tikv_amd.cmp_col_const(4, F.SIG_LT_INT, 20) if filtered else None
        k, ko, v, vo, nn, _ = rgn.host
        ods = tikv_amd.DagSelect(_dec_cols())
        if cond is not None:
            ods = ods.where(cond)
        od, orows = o.dag_run(ods.hash_agg(_all_aggs(), E(2)).build(),
                              k, ko, v, vo, nn)
        want = {}
        for row in split_datums(od, 9):
            c = int.from_bytes(row[-8:], "big") ^ (1 << 63)
            c = c - (1 << 64) if c >= (1 << 63) else c
            want[c] = row[:-9]
        assert len(want) == orows
        for kw, route in (({}, "plane"), ({"COPR_NO_PLANES": "1"}, "sorted")):
            h0 = engine.hash_plane_launches()
            with genv(**kw):
                gd, grows, _ = engine.dag_run(
                    two_key_req(_dec_cols(), cond=cond, aggs=_all_aggs()),
                    [rgn.dev])
            assert (engine.hash_plane_launches() > h0) == (route == "plane")
            got = {}
            for row in split_datums(gd, 10):
                a = int.from_bytes(row[-17:-9], "big") ^ (1 << 63)
                b = int.from_bytes(row[-8:], "big") ^ (1 << 63)
                a = a - (1 << 64) if a >= (1 << 63) else a
                assert row[-18] == 3 and row[-9] == 3
                got[a * 1000 + b] = row[:-18]
            assert grows == orows and got == want
    finally:
        rgn.close()


@pytest.mark.parametrize("k_null", [False, True])
@pytest.mark.parametrize("filtered", [False, True])
def test_constant_second_key_against_the_oracle(engine, filtered, k_null):
    o = orc()
    n = 777
    rows = []
    for i in range(n):
        r = {1: (i * 7) % 13 - 6 if i % 11 else None, 2: None if k_null else 7,
             5: (i * 31) % 101 - 50 if i % 9 else None}
        if i % 10 == 3:
            del r[1]
        rows.append(r)
    rgn = Rgn(engine, rows,
              tail=lambda i: cell_dec(6, (i * 7919) % 200_003 - 100_000, 2))
    try:
        cond = tikv_amd.cmp_col_const(4, F.SIG_LT_INT, 20) if filtered else None
        k, ko, v, vo, nn, _ = rgn.host
        ods = tikv_amd.DagSelect(_dec_cols())
        if cond is not None:
            ods = ods.where(cond)
        od, orows = o.dag_run(ods.hash_agg(_all_aggs(), E(0)).build(),
                              k, ko, v, vo, nn)
        kd = b"\x00" if k_null else b"\x03" + (7 ^ (1 << 63)).to_bytes(8, "big")
        want = sorted(r + kd for r in split_datums(od, 9))
        for kw in ({}, {"COPR_NO_PLANES": "1"}):
            with genv(**kw):
                gd, grows, _ = engine.dag_run(
                    two_key_req(_dec_cols(), cond=cond, aggs=_all_aggs()),
                    [rgn.dev])
            assert grows == orows
            assert split_datums(gd, 10) == want
    finally:
        rgn.close()


# ---- executor kinds, LIMIT, counters ----------------------------------------------
def test_slow_and_fast_hash_agg(engine):
    o = orc()
    rows = mixed_rows(513, seed=12)
    rgn = Rgn(engine, rows)
    try:
        fast = run(engine, two_key_req(COLS()), rgn, 6)
        slow = run(engine, two_key_req(COLS(), slow=True), rgn, 6)
        assert fast == slow == group_ref(rows, [Key(1), Key(2)], AGGS)
        # one key under SLOW_HASH_AGG plans as FAST_HASH_AGG: the oracle's
        # bytes as a multiset of rows, and no multi-key counter moves
        k, ko, v, vo, n, _ = rgn.host
        oreq = tikv_amd.DagSelect(COLS()).hash_agg(agg_defs(), E(0)).build()
        od, orows = o.dag_run(oreq, k, ko, v, vo, n)
        g0 = engine.group_stats()
        sreq = tikv_amd.DagSelect(COLS()).slow_hash_agg(agg_defs(), E(0)).build()
        freq = tikv_amd.DagSelect(COLS()).hash_agg(agg_defs(), E(0)).build()
        with genv():
            gd, grows, _ = engine.dag_run(sreq, [rgn.dev])
            fd, frows, _ = engine.dag_run(freq, [rgn.dev])
        assert engine.group_stats() == g0
        assert grows == orows == frows
        assert rows_of(gd, 5) == rows_of(od, 5) == rows_of(fd, 5)
        assert gd == fd
    finally:
        rgn.close()


def test_limit_below_the_group_count(engine):
    rows = mixed_rows(513, seed=13)
    rgn = Rgn(engine, rows)
    try:
        want = group_ref(rows, [Key(1), Key(2)], AGGS)
        assert len(want) > 4
        for kw in ({}, {"COPR_NO_PLANES": "1"}):
            got = run(engine, two_key_req(COLS(), limit=4), rgn, 6, **kw)
            assert len(got) == 4 and len(set(got)) == 4
            assert all(g in want for g in got)
        assert run(engine, two_key_req(COLS(), limit=10**6), rgn, 6) == want
    finally:
        rgn.close()


def test_counters(engine):
    rows = [{1: i % 6, 2: i % 4, 5: i} for i in range(300)]
    rgn = Rgn(engine, rows)
    try:
        g0 = engine.group_stats()
        run(engine, two_key_req(COLS()), rgn, 6, route="plane", source="plane")
        g1 = engine.group_stats()
        assert g1 == (g0[0] + 1, 12, g0[2], g0[3])
        run(engine, two_key_req(COLS()), rgn, 6, COPR_NO_PLANES="1")
        g2 = engine.group_stats()
        assert g2 == (g0[0] + 2, 12, g0[2], g0[3] + 1)
    finally:
        rgn.close()


# ---- refusals ---------------------------------------------------------------------
def _refused(engine, req, rgns, reason):
    with pytest.raises(RuntimeError) as ei, genv():
        engine.dag_run(req, rgns)
    assert str(ei.value).startswith(UNSUP), str(ei.value)
    assert reason in str(ei.value), str(ei.value)


def test_refused_shapes(engine):
    rows = [{1: i % 3, 2: i % 2, 3: 1, 4: 1, 5: i} for i in range(20)]
    tail = lambda i: (cell_dec(6, i, 2) + cell_real(7, 1.0 * i)  # noqa: E731
                      + var_bytes_cell(8, b"x%d" % (i % 3)))
    rgn = Rgn(engine, rows, tail=tail)
    rgn2 = Rgn(engine, rows, tail=tail)
    cols = COLS() + [tikv_amd.Col(6, tp=F.TP_NEWDECIMAL, decimal=2),
                     tikv_amd.Col(7, tp=F.TP_DOUBLE),
                     tikv_amd.Col(8, tp=F.TP_VARCHAR),
                     tikv_amd.Col(9, pk_handle=True)]
    aggs = [tikv_amd.count_star()]

    def req(keys, cond=None, kind="hash", index=False):
        ds = tikv_amd.DagSelect(cols, index=index)
        if cond is not None:
            ds = ds.where(cond)
        f = {"hash": ds.hash_agg, "slow": ds.slow_hash_agg,
             "stream": ds.stream_agg}[kind]
        return f(aggs, keys).build()

    try:
        one = [rgn.dev]
        _refused(engine, req([E(0), E(1), E(2), E(3), E(4)]), one, "at most 4")
        _refused(engine, req([E(0), E(8)]), one, "handle column")
        _refused(engine, req([E(0), E(7)], kind="slow"), one, "type not yet native")
        _refused(engine, req([E(5), E(0)]), one, "type not yet native")
        _refused(engine, req([E(0), E(6)]), one, "type not yet native")
        plus = tikv_amd.Expr().col(0).const_int(1).func(F.SIG_PLUS_INT, 2)
        _refused(engine, req([plus, E(1)]), one, "must be a column")
        _refused(engine, req([E(0), E(1)], index=True), one, "index scan")
        rpn = tikv_amd.Expr().col(0).col(1).func(F.SIG_LT_INT, 2)
        _refused(engine, req([E(0), E(1)], cond=rpn), one, "predicates")
        _refused(engine, req([E(0), E(1)]), [rgn.dev, rgn2.dev], "one region")
        _refused(engine, req([E(0), E(1)], kind="stream"), one, "stream agg")
    finally:
        rgn.close()
        rgn2.close()
