"""col IN (c1 .. cn) and NOT IN against a plain Python
reference over the generated rows: exact integers, three-valued result.
Regions of the plane kernels hold two full grid-stride steps at COPR_IN_GRID=1
plus one row; their results also equal the scan path's bytes."""
import random

import pytest

import tikv_amd
from tikv_amd import _ffi as F
from tikv_amd import in_col_consts as IN

from group_multi_util import Key, group_ref, rows_of
from selection_ref import ColSpec, gen_rows, out_datum, region_for
from topn_multi_util import INT64_MAX, U64, split_int_rows

pytestmark = pytest.mark.gpu

AGGS = [("count_star",), ("count", 6), ("max", 6), ("min", 6)]
NO_ROWS = [((3, 0), (3, 0), (0, None), (0, None))]


def in_value(v, items, negate=False):
    """the node on one cell: None (NULL), 1 or 0. Cells and items are exact
    integers, an unsigned item (x, True) the integer x."""
    if v is None:
        return None
    exact = {i[0] if isinstance(i, tuple) else i for i in items if i is not None}
    r = 1 if v in exact else None if None in items else 0
    return r if r is None or not negate else 1 - r


def true(v):
    return v is not None and v != 0


def agg_defs(off):
    return [tikv_amd.count_star(), tikv_amd.count_col(off),
            tikv_amd.max_col(off), tikv_amd.min_col(off)]


def split_sum_first(data):
    # first datum sum(int), a decimal of frac 0 or NULL -> (int or None, rest)
    if data[0] == 0:
        return None, data[1:]
    assert data[0] == 6 and data[2] == 0
    lead, words = [0, 1, 1, 2, 2, 3, 3, 4, 4][data[1] % 9], data[1] // 9
    raw = bytes([data[3] ^ 0x80]) + data[4:3 + lead + 4 * words]
    neg = not data[3] & 0x80
    if neg:
        raw = bytes(b ^ 0xFF for b in raw)
    v = int.from_bytes(raw[:lead], "big")
    for k in range(words):
        v = v * 10**9 + int.from_bytes(raw[lead + 4 * k:lead + 4 * k + 4], "big")
    return (-v if neg else v), data[3 + len(raw):]


N_A = 2 * 1024 + 261
SCHEMA_A = [ColSpec(1, False, -7), ColSpec(2, True), ColSpec(3, False),
            ColSpec(4), ColSpec(5), ColSpec(6)]
C1, C2, C3 = SCHEMA_A[:3]
SIGNED = [-20, -7, 3, 5, 11, (U64, True), (3, True)]


def rows_a():
    rows = gen_rows(random.Random(11), SCHEMA_A, N_A, n_pred_cols=3)
    rows[5][1], rows[6][1] = -1, INT64_MAX      # -1 is not (2^64-1, True)
    rows[5][2], rows[6][2] = U64, 2**63         # 2^64-1 is not -1
    for i, r in enumerate(rows):
        r[5] = None if i // 37 % 5 == 4 else i // 37 % 5 - 1
        r[6] = (i * 7919) % N_A * 3 - N_A
    return rows


ROWS_A = rows_a()


def gt3(r):                  # column 3 > 3 is true; NULL > 3 is not
    return (C3.cell(r) or 0) > 3


# name -> (condition builders, the selection's value on a row, offsets it names)
CASES_A = {
    "in": ([lambda: IN(0, SIGNED)], lambda r: in_value(C1.cell(r), SIGNED), {0}),
    "in_null": ([lambda: IN(0, SIGNED + [None])],
                lambda r: in_value(C1.cell(r), SIGNED + [None]), {0}),
    "not_in": ([lambda: IN(0, SIGNED, negate=True)],
               lambda r: in_value(C1.cell(r), SIGNED, True), {0}),
    "not_in_null": ([lambda: IN(0, [None] + SIGNED, True)], lambda r: None, {0}),
    "unsigned": ([lambda: IN(1, [-1, 4, (9, True), (2**63, True), -(2**63)])],
                 lambda r: in_value(C2.cell(r), [4, 9, 2**63]), {1}),
    "and_cmp": ([lambda: IN(0, SIGNED, negate=True),
                 lambda: tikv_amd.cmp_col_const(2, F.SIG_GT_INT, 3)],
                lambda r: true(in_value(C1.cell(r), SIGNED, True)) and gt3(r),
                {0, 2}),
    "or_cmp": ([lambda: IN(0, SIGNED + [None]).col(2).const_int(3)
                .func(F.SIG_GT_INT, 2).func(F.SIG_LOGICAL_OR, 2)],
               lambda r: true(in_value(C1.cell(r), SIGNED + [None])) or gt3(r),
               {0, 2}),
}


@pytest.mark.parametrize("case", sorted(CASES_A))
@pytest.mark.parametrize("site", ["simple", "hash", "project"])
def test_evaluator_sites(engine, monkeypatch, site, case):
    monkeypatch.setenv("COPR_NO_IN_PLANES", "1")
    conds, value, named = CASES_A[case]
    kept = [r for r in ROWS_A if true(value(r))]
    assert case == "not_in_null" or 0 < len(kept) < N_A
    ds = (tikv_amd.DagSelect([c.col() for c in SCHEMA_A])
          .where(*[c() for c in conds]))
    rgn = engine.region_raw(*region_for(ROWS_A, SCHEMA_A)[:5])
    try:
        if site == "simple":
            data = engine.dag_run(ds.simple_agg(agg_defs(5)).build(), [rgn])[0]
            assert split_int_rows(data, 4) == (group_ref(kept, [], AGGS) or NO_ROWS)
        elif site == "hash":
            req = ds.hash_agg(agg_defs(5), tikv_amd.Expr().col(4)).build()
            assert rows_of(engine.dag_run(req, [rgn])[0], 5) == \
                group_ref(kept, [Key(5)], AGGS)
        else:
            data = engine.dag_run(ds.output(list(range(6))).build(), [rgn])[0]
            assert split_int_rows(data, 6) == [
                tuple(out_datum(cs, r, off in named)
                      for off, cs in enumerate(SCHEMA_A)) for r in kept]
    finally:
        rgn.close()


def check_planes(engine, monkeypatch, schema, rows, items, negate, stat, full):
    """count(*) alone and, with `full`, sum / count(*) / count / max / min of
    column 6: the reference, the kernel in_stats()[stat] counts, the scan path"""
    kept = [r for r in rows if true(in_value(schema[0].cell(r), items, negate))]
    monkeypatch.setenv("COPR_IN_GRID", "1")
    monkeypatch.setenv("COPR_PLANE_BUDGET_MB", "64")
    rgn = engine.region_raw(*region_for(rows, schema)[:5])
    try:
        for aggs in ([tikv_amd.count_star()],
                     [tikv_amd.sum_col(1)] + agg_defs(1))[:2 if full else 1]:
            req = (tikv_amd.DagSelect([c.col() for c in schema])
                   .where(IN(0, items, negate))
                   .simple_agg(aggs).build())
            monkeypatch.delenv("COPR_NO_IN_PLANES", raising=False)
            before = engine.in_stats()[stat]
            data = engine.dag_run(req, [rgn])[0]
            assert engine.in_stats()[stat] == before + 1
            monkeypatch.setenv("COPR_NO_IN_PLANES", "1")
            assert engine.dag_run(req, [rgn])[0] == data
            assert engine.in_stats()[stat] == before + 1
            if len(aggs) == 1:
                assert split_int_rows(data, 1) == [((3, len(kept)),)]
                continue
            total, rest = split_sum_first(data)
            vals = [r[6] for r in kept if r.get(6) is not None]
            assert total == (sum(vals) if vals else None)
            assert split_int_rows(rest, 4) == (group_ref(kept, [], AGGS) or NO_ROWS)
    finally:
        rgn.close()


N_B = 2 * (256 * 4 * 2) + 1      # block x COPR_PLANE_IN_UNR x rows per 16 B


def rows_b(unsigned):
    rng = random.Random(5 + unsigned)
    rows = []
    for i in range(N_B):
        r = {6: None if i % 13 == 0 else (i * 7919) % N_B * 5 - 9000}
        x = rng.random()
        if x >= 0.08:                         # else: absent, takes the default
            v = rng.randrange(-600, 700)
            r[1] = None if x < 0.16 else v % 2**64 if unsigned else v
        rows.append(r)
    for i, v in enumerate([0, 1, 523, 524, 525, -1]):   # each list's `empty`
        rows[10 + i][1] = v % 2**64 if unsigned else v
    return rows


ROWS_B = {False: rows_b(False), True: rows_b(True)}


@pytest.mark.parametrize("dflt_in", [False, True])
@pytest.mark.parametrize("with_null", [False, True])
@pytest.mark.parametrize("negate", [False, True])
@pytest.mark.parametrize("size", [1, 1024, "unsigned"])
def test_plane_in(engine, monkeypatch, size, negate, with_null, dflt_in):
    """the default inside and outside the list; some row's value is the
    image's `empty`, the smallest of 0, 1, 2 ... that is no key. Unsigned
    cells reach 2^64-1: -1 and -600 match none, (2^64-300, True) its cell."""
    uns = size == "unsigned"
    base = list(range(-500, 525))
    base.remove(524 if dflt_in else -7)
    items = base if size == 1024 else [-7 if dflt_in else 3]
    if uns:
        items = [-1, -600, (2**64 - 300, True), (77, True), 5 if dflt_in else 6]
    if with_null:
        items = items[:-1] + [None]
    empty = min(set(range(1026)) - {i for i in items if isinstance(i, int)})
    assert uns or len(items) == size
    assert any(r.get(1) == empty for r in ROWS_B[uns])
    check_planes(engine, monkeypatch,
                 [ColSpec(1, uns, 5 if uns else -7), ColSpec(6)], ROWS_B[uns],
                 items, negate, 0, full=True)


@pytest.mark.parametrize("negate", [False, True])
@pytest.mark.parametrize("base", [-3, INT64_MAX - 70000])
@pytest.mark.parametrize("width", [1, 2])
def test_plane_in_bitmap(engine, monkeypatch, width, base, negate):
    """every row an int in [base, base + span]: a `width`-byte plane; keys
    around both ends of the range and at the bitmap's word boundaries"""
    span = 200 if width == 1 else 60000
    n = 2 * 256 * 4 * (16 // width) + 1   # block x COPR_PLANE_INB_UNR x rows
    rng = random.Random(width)
    rows = [{1: base + rng.randrange(span + 1)} for _ in range(n)]
    rows[0][1], rows[n - 1][1] = base, base + span
    items = [base + d for d in (-1, 0, 1, 31, 32, 33, 63, 64, 95, 96, 127, 128,
                                span - 1, span, span + 1, span + 300)]
    items += [(base + 150, True)] if base > 0 else [-(2**63), (2**63, True)]
    check_planes(engine, monkeypatch, [ColSpec(1)], rows, items, negate, 1,
                 full=False)


@pytest.mark.parametrize("conds", [
    lambda: [IN(0, list(range(1025)))],
    lambda: [IN(0, [1, 2]), IN(2, [3])],
    lambda: [tikv_amd.Expr().const_int(1).const_int(2).func(F.SIG_IN_INT, 2)],
], ids=["1025_items", "two_in_nodes", "const_probe"])
def test_limits_are_unsupported(engine, conds):
    """the plan is refused before any region is looked at"""
    req = (tikv_amd.DagSelect([c.col() for c in SCHEMA_A]).where(*conds())
           .simple_agg([tikv_amd.count_star()]).build())
    with pytest.raises(RuntimeError, match=r"copr_dag_run: 3 \("):
        engine.dag_run(req, [])
