"""TopN over several order-by columns on the GPU, bit-for-bit
against the oracle (pinned by tests/test_topn_multi_oracle.py).

Every request with more than one order-by expression must go through the
multi-key pipeline (Engine.topn_stats()[0] advances) and return the oracle's
bytes and row count: lexicographic order with a direction per key, NULL first
within a key (last under desc), source order under full ties, every order
column emitted decoded, absent cells filled from the column default. The
candidate counts asserted below follow from the cut rule
(tikv_amd/csrc/topn_keys.h topn_cut): they are exact, not measured.
"""
import functools
import itertools
import random

import pytest

import tikv_amd
from tikv_amd import _ffi as F

from topn_multi_util import (INT64_MAX, INT64_MIN, U64, int_datum, orc,
                             region_of, uint_datum)

pytestmark = pytest.mark.gpu

BIG = 2**63 + 5
UNSUP = "copr_dag_run: %d " % F.COPR_ERR_UNSUPPORTED


def E(off):
    return tikv_amd.Expr().col(off)


class Rgn:
    """a hand-built region on both sides: host arrays for the oracle, a
    device region for the engine"""

    def __init__(self, engine, rows, unsigned=()):
        self.host = region_of(rows, unsigned=unsigned)
        k, ko, v, vo, n, _ = self.host
        self.dev = engine.region_raw(k, ko, v, vo, n)
        self.n = n

    def close(self):
        self.dev.close()


def check(engine, o, req, rgn, multi=True):
    """engine bytes == oracle bytes, row counts equal; returns the row count
    and the engine's topn_stats() after the request"""
    k, ko, v, vo, n, _ = rgn.host
    od, orows = o.dag_run(req, k, ko, v, vo, n)
    s0 = engine.topn_stats()
    gd, grows, _ = engine.dag_run(req, [rgn.dev])
    s1 = engine.topn_stats()
    assert grows == orows
    assert gd == od
    if multi:
        assert s1[0] == s0[0] + 1, "request did not take the multi-key path"
    else:
        assert s1 == s0, "single-key request moved the multi-key counters"
    return grows, s1


# ---- two keys, tie-heavy primary ----------------------------------------
@functools.lru_cache(maxsize=None)
def _tie_rows(n_rows):
    rng = random.Random(1000 + n_rows)
    return tuple((rng.choice([None, -2, 0, 3]), rng.choice([None, 1, 7, BIG]))
                 for _ in range(n_rows))


@pytest.mark.parametrize("n_rows", [300, 4097])
def test_two_keys_tie_heavy(engine, n_rows):
    o = orc()
    rows = [{1: a, 2: b, 3: i} for i, (a, b) in enumerate(_tie_rows(n_rows))]
    rgn = Rgn(engine, rows, unsigned={2})
    cols = [tikv_amd.Col(1), tikv_amd.Col(2, flag=F.FLAG_UNSIGNED),
            tikv_amd.Col(3)]
    try:
        for d0, d1 in itertools.product((False, True), repeat=2):
            for n in (1, 40, 300, 10000):
                req = (tikv_amd.DagSelect(cols)
                       .topn([(E(0), d0), (E(1), d1)], n).build())
                got, st = check(engine, o, req, rgn)
                assert got == min(n, n_rows)
                assert st[1] == n_rows and n_rows >= st[2] >= got
        # LIMIT below and above n
        for lim in (7, 55):
            req = (tikv_amd.DagSelect(cols)
                   .topn([(E(0), False), (E(1), True)], 40).limit(lim).build())
            got, _ = check(engine, o, req, rgn)
            assert got == min(40, lim)
    finally:
        rgn.close()


# ---- the candidate cut ----------------------------------------------------
def _cut_case(engine, primaries, n):
    o = orc()
    rng = random.Random(5)
    rows = [{1: a, 2: rng.randrange(-50, 50), 3: i}
            for i, a in enumerate(primaries)]
    rgn = Rgn(engine, rows)
    cols = [tikv_amd.Col(1), tikv_amd.Col(2), tikv_amd.Col(3)]
    try:
        req = (tikv_amd.DagSelect(cols)
               .topn([(E(0), False), (E(1), False)], n).build())
        _, st = check(engine, o, req, rgn)
        return st
    finally:
        rgn.close()


def test_cut_inside_a_tie_run(engine):
    # sorted primaries: 30 distinct, a run of exactly 50 equal values at
    # positions 30..79, then distinct ones. n = 40 cuts inside the run, so
    # the whole run is a candidate: 30 + 50.
    m = 1000
    prim = list(range(30)) + [100] * 50 + list(range(200, 200 + m - 80))
    random.Random(9).shuffle(prim)
    st = _cut_case(engine, prim, 40)
    assert (st[1], st[2]) == (m, 80)


def test_cut_distinct_primaries(engine):
    prim = list(range(-500, 500))
    random.Random(10).shuffle(prim)
    st = _cut_case(engine, prim, 40)
    assert (st[1], st[2]) == (1000, 40)


def test_cut_constant_primary(engine):
    st = _cut_case(engine, [7] * 777, 40)
    assert (st[1], st[2]) == (777, 777)


# ---- extremes -------------------------------------------------------------
def test_extreme_values_both_directions(engine):
    o = orc()
    sv = [INT64_MIN, INT64_MAX, -1, 0, 1, None, INT64_MIN + 1, INT64_MAX - 1]
    uv = [0, U64, 1, 2**63, 2**63 - 1, None, U64 - 1]
    rng = random.Random(3)
    rows = [{1: rng.choice(sv), 2: rng.choice(uv), 3: i} for i in range(513)]
    rgn = Rgn(engine, rows, unsigned={2})
    cols = [tikv_amd.Col(1), tikv_amd.Col(2, flag=F.FLAG_UNSIGNED),
            tikv_amd.Col(3)]
    try:
        for d0, d1 in itertools.product((False, True), repeat=2):
            for order in ([(E(0), d0), (E(1), d1)], [(E(1), d1), (E(0), d0)]):
                req = tikv_amd.DagSelect(cols).topn(order, 200).build()
                check(engine, o, req, rgn)
    finally:
        rgn.close()


def test_primary_null_in_every_row(engine):
    o = orc()
    rng = random.Random(4)
    rows = [{1: None, 2: rng.choice([None, 5, -5, 9]), 3: i}
            for i in range(700)]
    rgn = Rgn(engine, rows)
    cols = [tikv_amd.Col(1), tikv_amd.Col(2), tikv_amd.Col(3)]
    try:
        for d0, d1 in itertools.product((False, True), repeat=2):
            req = (tikv_amd.DagSelect(cols)
                   .topn([(E(0), d0), (E(1), d1)], 33).build())
            _, st = check(engine, o, req, rgn)
            assert (st[1], st[2]) == (700, 700)
    finally:
        rgn.close()


def test_filter_keeps_none_and_one(engine):
    o = orc()
    rows = [{1: i % 5, 2: i % 3, 3: i} for i in range(600)]
    rgn = Rgn(engine, rows)
    cols = [tikv_amd.Col(1), tikv_amd.Col(2), tikv_amd.Col(3)]
    try:
        none = tikv_amd.cmp_col_const(2, F.SIG_GT_INT, 10**6)
        req = (tikv_amd.DagSelect(cols).where(none)
               .topn([(E(0), False), (E(1), True)], 10).build())
        got, st = check(engine, o, req, rgn)
        assert got == 0 and (st[1], st[2]) == (0, 0)
        one = tikv_amd.cmp_col_const(2, F.SIG_EQ_INT, 417)
        req = (tikv_amd.DagSelect(cols).where(one)
               .topn([(E(0), False), (E(1), True)], 10).build())
        got, st = check(engine, o, req, rgn)
        assert got == 1 and (st[1], st[2]) == (1, 1)
    finally:
        rgn.close()


# ---- three and four keys --------------------------------------------------
def test_three_and_four_keys(engine):
    o = orc()
    rng = random.Random(6)
    dom = [[None, -1, 4], [0, 9, 2**63 + 1], [None, 3, 5], [-7, 0, 7]]
    rows = [{1: rng.choice(dom[0]), 2: rng.choice(dom[1]),
             3: rng.choice(dom[2]), 4: rng.choice(dom[3]), 5: i}
            for i in range(2000)]
    rgn = Rgn(engine, rows, unsigned={2})
    cols = [tikv_amd.Col(1), tikv_amd.Col(2, flag=F.FLAG_UNSIGNED),
            tikv_amd.Col(3), tikv_amd.Col(4), tikv_amd.Col(5)]
    try:
        orders = [
            [(E(0), False), (E(1), True), (E(2), False)],
            [(E(2), True), (E(0), True), (E(3), False)],
            [(E(0), False), (E(1), True), (E(2), True), (E(3), False)],
            [(E(3), True), (E(2), False), (E(1), False), (E(0), True)],
        ]
        for order in orders:
            for n in (50, 1500):
                req = tikv_amd.DagSelect(cols).topn(order, n).build()
                check(engine, o, req, rgn)
    finally:
        rgn.close()


def test_repeated_column(engine):
    o = orc()
    rng = random.Random(7)
    rows = [{1: rng.choice([None, 1, 2, 3]), 2: rng.choice([None, 10, 20]),
             3: i} for i in range(900)]
    rgn = Rgn(engine, rows)
    cols = [tikv_amd.Col(1), tikv_amd.Col(2), tikv_amd.Col(3)]
    try:
        req = (tikv_amd.DagSelect(cols)
               .topn([(E(0), False), (E(1), True), (E(0), True)], 120).build())
        check(engine, o, req, rgn)
        # every expression names the same column: one key is left
        req = (tikv_amd.DagSelect(cols)
               .topn([(E(1), True), (E(1), False)], 120).build())
        check(engine, o, req, rgn)
    finally:
        rgn.close()


# ---- absent cells ---------------------------------------------------------
@pytest.mark.parametrize("with_default", [True, False])
def test_absent_key_cells(engine, with_default):
    o = orc()
    rng = random.Random(8)
    rows = []
    for i in range(1500):
        r = {1: rng.choice([None, -3, 0, 6]), 2: rng.choice([None, 2, 8]),
             3: i}
        if i % 3 == 0:
            del r[1]
        if i % 3 == 1:
            del r[2]
        rows.append(r)
    rgn = Rgn(engine, rows, unsigned={2})
    cols = [tikv_amd.Col(1, default_val=int_datum(0) if with_default else None),
            tikv_amd.Col(2, flag=F.FLAG_UNSIGNED,
                         default_val=uint_datum(5) if with_default else None),
            tikv_amd.Col(3)]
    try:
        for d0, d1 in itertools.product((False, True), repeat=2):
            req = (tikv_amd.DagSelect(cols)
                   .topn([(E(0), d0), (E(1), d1)], 400).build())
            check(engine, o, req, rgn)
        # one order-by expression: today's path, whatever it returns
        s0 = engine.topn_stats()
        req = tikv_amd.DagSelect(cols).topn(E(0), 400).build()
        gd, grows, _ = engine.dag_run(req, [rgn.dev])
        assert grows == 400
        assert engine.topn_stats() == s0
    finally:
        rgn.close()


# ---- predicates -----------------------------------------------------------
def test_predicates_with_columns_in_output(engine):
    o = orc()
    rng = random.Random(11)
    rows = [{1: rng.choice([None, -2, 0, 3]), 2: rng.choice([None, 1, 7, BIG]),
             3: rng.randrange(-100, 100), 4: rng.choice([None, 5, 6, 7, 8]),
             5: i} for i in range(3000)]
    rgn = Rgn(engine, rows, unsigned={2})
    cols = [tikv_amd.Col(1), tikv_amd.Col(2, flag=F.FLAG_UNSIGNED),
            tikv_amd.Col(3), tikv_amd.Col(4), tikv_amd.Col(5)]
    order = [(E(0), False), (E(1), True)]
    try:
        c3 = tikv_amd.cmp_col_const(2, F.SIG_GT_INT, -40)
        c4 = tikv_amd.cmp_col_const(3, F.SIG_NE_INT, 6)
        c1 = tikv_amd.cmp_col_const(0, F.SIG_GE_INT, -2)   # an order column
        for conds in ([c3], [c3, c4], [c1], [c1, c4], [c4, c1]):
            for n in (60, 5000):
                req = (tikv_amd.DagSelect(cols).where(*conds)
                       .topn(order, n).build())          # all five columns out
                check(engine, o, req, rgn)
        req = (tikv_amd.DagSelect(cols).where(c3, c4)
               .topn(order, 60).output([4, 3, 2, 0]).build())
        check(engine, o, req, rgn)
    finally:
        rgn.close()


# ---- generated regions ----------------------------------------------------
@pytest.mark.parametrize("row_format", [1, 2])
def test_generated_region(engine, row_format):
    o = orc()
    g = tikv_amd.GenRegion(config_index=1, n_rows=200001, table_id=5,
                           row_format=row_format)
    try:
        rgn = engine.region(g)
        try:
            cols = [tikv_amd.Col(i) for i in range(1, 17)]
            for d0, d1, chunked in ((False, True, False), (True, False, False),
                                    (False, True, row_format == 2)):
                sel = (tikv_amd.DagSelect(cols)
                       .topn([(E(4), d0), (E(7), d1)], 100).output([0, 4, 7]))
                if chunked:
                    sel = sel.chunked()
                req = sel.build()
                s0 = engine.topn_stats()
                gd, gr, _ = engine.dag_run(req, [rgn])
                od, orows = o.dag_run(req, g.keys, g.key_offs, g.vals,
                                      g.val_offs, g.n_kv)
                st = engine.topn_stats()
                assert st[0] == s0[0] + 1
                assert gr == orows == 100
                assert gd == od
                assert st[1] == 200001 and 100 <= st[2] <= 200001
        finally:
            rgn.close()
    finally:
        g.close()


# ---- shapes that stay loud ------------------------------------------------
def test_unsupported_shapes_stay_loud(engine):
    o = orc()
    rng = random.Random(12)
    rows = [{c: rng.randrange(-9, 9) for c in range(1, 7)} for _ in range(400)]
    rgn = Rgn(engine, rows)
    rgn2 = Rgn(engine, rows)
    cols = [tikv_amd.Col(i) for i in range(1, 7)]
    hcols = cols + [tikv_amd.Col(-1, pk_handle=True)]
    try:
        def single_key_still_matches():
            sel = tikv_amd.cmp_col_const(1, F.SIG_GT_INT, -5)
            req = (tikv_amd.DagSelect(cols).where(sel)
                   .topn(E(0), 25, desc=True).output([1, 0, 3]).build())
            check(engine, o, req, rgn, multi=False)

        def loud(req, regions):
            s0 = engine.topn_stats()
            with pytest.raises(RuntimeError) as ei:
                engine.dag_run(req, regions)
            assert UNSUP in str(ei.value), str(ei.value)
            assert engine.topn_stats() == s0
            single_key_still_matches()

        two = [(E(0), False), (E(1), True)]
        # five keys
        loud(tikv_amd.DagSelect(cols)
             .topn([(E(i), False) for i in range(5)], 10).build(), [rgn.dev])
        # a handle column as a key
        loud(tikv_amd.DagSelect(hcols)
             .topn([(E(0), False), (E(6), False)], 10).build(), [rgn.dev])
        # two regions
        loud(tikv_amd.DagSelect(cols).topn(two, 10).build(),
             [rgn.dev, rgn2.dev])
        # an RPN predicate
        rpn = (tikv_amd.Expr().col(2).col(3).func(F.SIG_PLUS_INT)
               .const_int(0).func(F.SIG_GT_INT))
        loud(tikv_amd.DagSelect(cols).where(rpn).topn(two, 10).build(),
             [rgn.dev])
    finally:
        rgn.close()
        rgn2.close()


# ---- single key unchanged -------------------------------------------------
def test_single_key_path_untouched(engine):
    o = orc()
    g = tikv_amd.GenRegion(config_index=1, n_rows=200001, table_id=5)
    try:
        rgn = engine.region(g)
        try:
            cols = [tikv_amd.Col(i) for i in range(1, 17)]
            sel = tikv_amd.cmp_col_const(3, F.SIG_GT_INT, 0)
            req = (tikv_amd.DagSelect(cols).where(sel)
                   .topn(E(4), 100).output([0, 4, 7]).build())
            s0 = engine.topn_stats()
            gd, gr, _ = engine.dag_run(req, [rgn])
            od, orows = o.dag_run(req, g.keys, g.key_offs, g.vals,
                                  g.val_offs, g.n_kv)
            assert (gr, gd) == (orows, od)
            assert engine.topn_stats() == s0
        finally:
            rgn.close()
    finally:
        g.close()
