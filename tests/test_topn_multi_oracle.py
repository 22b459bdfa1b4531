"""Multi-key TopN through the oracle, against hand-computed answers: pins
what tests/test_topn_multi.py compares the engine with.

Comparator (top_n_executor.rs): lexicographic over the order keys; within a
key NULL sorts before every value, values in signed or unsigned order per the
column's UNSIGNED flag; desc reverses that key alone, NULL placement included;
full ties keep source-row order. Every order column comes back decoded
(flag 3 signed, 4 unsigned, 0 NULL); other columns come back raw."""
import tikv_amd
from tikv_amd import _ffi as F

from topn_multi_util import int_datum, orc, region_of, split_int_rows, uint_datum

BIG = 2**63 + 5

# (a signed col 1, b unsigned col 2); col 3 = the row index
AB = [(3, 7), (None, 1), (-2, None), (3, BIG), (-2, 7), (None, None), (0, 1),
      (3, 7)]


def _cols(**kw):
    return [tikv_amd.Col(1, default_val=kw.get("d1")),
            tikv_amd.Col(2, flag=F.FLAG_UNSIGNED, default_val=kw.get("d2")),
            tikv_amd.Col(3)]


def test_topn_two_keys_asc_desc_oracle():
    o = orc()
    rows = [{1: a, 2: b, 3: i} for i, (a, b) in enumerate(AB)]
    k, ko, v, vo, n, keep = region_of(rows, unsigned={2})
    req = (tikv_amd.DagSelect(_cols())
           .topn([(tikv_amd.Expr().col(0), False),
                  (tikv_amd.Expr().col(1), True)], 5).build())
    data, nrows = o.dag_run(req, k, ko, v, vo, n)
    assert nrows == 5
    # a asc: NULLs (rows 1, 5), then -2 (rows 2, 4), then 0 (row 6).
    # b desc inside: values descending, NULL last.
    assert split_int_rows(data, 3) == [
        ((0, None), (4, 1), (8, 1)),
        ((0, None), (0, None), (8, 5)),
        ((3, -2), (4, 7), (8, 4)),
        ((3, -2), (0, None), (8, 2)),
        ((3, 0), (4, 1), (8, 6)),
    ]


def test_topn_two_keys_desc_asc_defaults_oracle():
    o = orc()
    rows = [{1: a, 2: b, 3: i} for i, (a, b) in enumerate(AB)]
    del rows[7][1]        # a absent -> default 3
    del rows[0][2]        # b absent -> default 7
    k, ko, v, vo, n, keep = region_of(rows, unsigned={2})
    req = (tikv_amd.DagSelect(_cols(d1=int_datum(3), d2=uint_datum(7)))
           .topn([(tikv_amd.Expr().col(0), True),
                  (tikv_amd.Expr().col(1), False)], 4).build())
    data, nrows = o.dag_run(req, k, ko, v, vo, n)
    assert nrows == 4
    # a desc: 3 (rows 0, 3, 7), then 0 (row 6). b asc (unsigned) inside:
    # 7, 7 (rows 0 and 7 tie: arrival order), then 2^63+5 (row 3).
    assert split_int_rows(data, 3) == [
        ((3, 3), (4, 7), (8, 0)),
        ((3, 3), (4, 7), (8, 7)),
        ((3, 3), (4, BIG), (8, 3)),
        ((3, 0), (4, 1), (8, 6)),
    ]
