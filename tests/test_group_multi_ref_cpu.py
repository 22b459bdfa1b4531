"""Pins the Python group-by of tests/group_multi_util.py, the reference of
test_group_multi.py, against the oracle with one group-by column, on the kind
of hand-built region those tests use: NULL and absent key cells with and
without a column default, an unsigned key above 2^63, row-v1 and row-v2, with
and without a filter. Needs no GPU."""
import random

import pytest

import tikv_amd
from tikv_amd import _ffi as F

from group_multi_util import (Key, build_region, group_ref, orc, rows_of)
from topn_multi_util import INT64_MAX, INT64_MIN, U64, int_datum, uint_datum

AGGS = [("count_star",), ("count", 5), ("max", 5), ("min", 5)]


def _req(cols, key_off, cond=None):
    ds = tikv_amd.DagSelect(cols)
    if cond is not None:
        ds = ds.where(cond)
    return ds.hash_agg([tikv_amd.count_star(), tikv_amd.count_col(2),
                        tikv_amd.max_col(2), tikv_amd.min_col(2)],
                       tikv_amd.Expr().col(key_off)).build()


def _rows(n):
    rng = random.Random(77)
    sv = [None, INT64_MIN, -1, 0, 1, INT64_MAX]
    uv = [None, 0, 1, 2**63, U64]
    rows = []
    for i in range(n):
        r = {1: rng.choice(sv), 2: rng.choice(uv),
             5: rng.choice([None, -9, 4, 10**12])}
        if i % 7 == 3:
            del r[1]
        if i % 5 == 2:
            del r[2]
        rows.append(r)
    return rows


@pytest.mark.parametrize("v2", [False, True])
@pytest.mark.parametrize("defaults", [False, True])
def test_python_group_by_matches_oracle_single_key(v2, defaults):
    o = orc()
    rows = _rows(300)
    k, ko, v, vo, n, keep = build_region(rows, unsigned={2}, v2=v2)
    d1 = int_datum(-5) if defaults else None
    d2 = uint_datum(2**63 + 9) if defaults else None
    cols = [tikv_amd.Col(1, default_val=d1),
            tikv_amd.Col(2, flag=F.FLAG_UNSIGNED, default_val=d2),
            tikv_amd.Col(5)]
    keys = [Key(1, False, -5 if defaults else None),
            Key(2, True, 2**63 + 9 if defaults else None)]
    for off, key in enumerate(keys):
        for cond, kf in ((None, None),
                         (tikv_amd.cmp_col_const(2, F.SIG_GT_INT, 0),
                          lambda r: r.get(5) is not None and r[5] > 0)):
            data, nrows = o.dag_run(_req(cols, off, cond), k, ko, v, vo, n)
            want = group_ref(rows, [key], AGGS, keep=kf)
            assert nrows == len(want)
            assert rows_of(data, 5) == want
