"""The CPU oracle's int selection predicates against the exact Python
reference of selection_ref.py. The device evaluator was
written after the oracle's, so a mistake shared by the two passes every
engine-against-oracle test; this file pins the oracle, test_selection_ref.py
pins the engine, both against the same independent model."""
import random

import pytest

import tikv_amd

from selection_ref import (EDGE_SHARES, ColSpec, Gen, RefAmbiguous,
                           RefOverflow, gen_rows, gen_schema, project_ref,
                           region_for, select, to_expr)
from topn_multi_util import INT64_MAX, U64, orc, split_int_rows

N_PROGRAMS = 320
N_ROWS = 257


def oracle_count(o, conds, rows, schema, v2=False):
    """count(*) the oracle returns under the selection, or "error\""""
    host = region_for(rows, schema, v2=v2)
    req = (tikv_amd.DagSelect([c.col() for c in schema])
           .where(*[to_expr(c, schema) for c in conds])
           .simple_agg([tikv_amd.count_star()]).build())
    try:
        data, n = o.dag_run(req, *host[:5])
    except RuntimeError as e:
        assert "out of range" in str(e), str(e)
        return "error"
    assert n == 1
    return split_int_rows(data, 1)[0][0][1]


def ref_count(conds, rows, schema):
    try:
        return len(select(conds, rows, schema))
    except RefOverflow:
        return "error"
    except RefAmbiguous:
        return "ambiguous"


def generated_cases():
    """(seed, schema, rows, conds, v2) for every seeded program"""
    for seed in range(N_PROGRAMS):
        rng = random.Random(1000 + seed)
        schema = gen_schema(rng)
        rows = gen_rows(rng, schema, N_ROWS, p_edge=rng.choice(EDGE_SHARES))
        conds = Gen(seed, schema).selection()
        yield seed, schema, rows, conds, seed % 4 == 3


def test_generated_programs_and_generator_caps():
    o = orc()
    raised = ambiguous = informative = 0
    wrong = []
    for seed, schema, rows, conds, v2 in generated_cases():
        want = ref_count(conds, rows, schema)
        if want == "ambiguous":
            ambiguous += 1
            continue
        if want == "error":
            raised += 1
        elif 1 <= want <= N_ROWS - 1:
            informative += 1
        got = oracle_count(o, conds, rows, schema, v2=v2)
        if got != want:
            wrong.append((seed, conds, want, got))
    assert not wrong, "%d programs differ, first: %r" % (len(wrong), wrong[0])
    # the generator's caps, from the reference alone
    quiet = N_PROGRAMS - raised - ambiguous
    print("raised %d, ambiguous %d, informative %d of %d quiet"
          % (raised, ambiguous, informative, quiet))
    assert N_PROGRAMS / 10 <= raised <= N_PROGRAMS / 3
    assert informative * 2 >= quiet
    assert ambiguous * 20 <= N_PROGRAMS


U_SCHEMA = [ColSpec(1, unsigned=True)]


def _ucol_op_const(op, k):
    return ("cmp", "gt", ("arith", op, ("col", 0), ("const", k, True)),
            ("const", 0, False))


@pytest.mark.parametrize("op,k,cell,want", [
    ("plus", 1, U64, "error"),            # 2^64: BIGINT UNSIGNED overflow
    ("plus", 1, INT64_MAX, 1),            # 2^63 fits BIGINT UNSIGNED
    ("mul", 2**31, 2**32, 1),             # 2^63 again
    ("minus", 1, 0, "error"),             # -1 is no BIGINT UNSIGNED
])
def test_unsigned_arithmetic_cases(op, k, cell, want):
    conds = [_ucol_op_const(op, k)]
    rows = [{1: cell}]
    assert ref_count(conds, rows, U_SCHEMA) == want
    assert oracle_count(orc(), conds, rows, U_SCHEMA) == want


@pytest.mark.parametrize("op,l,lu,r,ru,want", [
    # every variant at its two edges: (signed, unsigned) operand pairs
    ("plus", -1, False, 0, True, "error"),
    ("plus", -1, False, 1, True, 0),
    ("plus", 1, False, U64, True, "error"),
    ("plus", U64, True, -1, False, 1),
    ("plus", INT64_MAX, False, INT64_MAX, True, 1),
    ("plus", -2**63, False, 2**63, True, 0),
    ("plus", -2**63, False, 2**63 - 1, True, "error"),
    ("minus", -1, False, 0, True, "error"),
    ("minus", 5, False, 5, True, 0),
    ("minus", 5, False, 6, True, "error"),
    ("minus", 0, True, -2**63, False, 1),
    ("minus", 2**63, True, -2**63, False, "error"),
    ("minus", 2**63 - 1, True, -2**63, False, 1),
    ("minus", 2**63, True, INT64_MAX, False, 1),
    ("minus", 3, True, 4, False, "error"),
    ("minus", 3, True, 4, True, "error"),
    ("mul", -1, False, 1, True, "error"),
    ("mul", 1, True, -1, False, "error"),
    ("mul", 2, False, 2**63, True, "error"),
    ("mul", 2**32, True, 2**32, True, "error"),
    ("mul", 2**32, True, 2**32 - 1, True, 1),
    ("mul", 2**32, False, 2**31, False, "error"),
    ("mul", -2**32, False, 2**31, False, 1),
    ("minus", -2**63, False, 1, False, "error"),
])
def test_arithmetic_variants_at_their_edges(op, l, lu, r, ru, want):
    """l OP r <> 0 on one row; l is a column, r a constant"""
    schema = [ColSpec(1, unsigned=lu)]
    conds = [("cmp", "ne", ("arith", op, ("col", 0), ("const", r, ru)),
              ("const", 0, False))]
    rows = [{1: l}]
    assert ref_count(conds, rows, schema) == want
    assert oracle_count(orc(), conds, rows, schema) == want


def test_conditions_apply_in_order():
    """WHERE c1 < 10 AND c1 + INT64_MAX > 0: the second condition would
    overflow on the row the first one drops, and never sees it. The other
    way round the overflow comes first and fails the request."""
    schema = [ColSpec(1)]
    lt = ("cmp", "lt", ("col", 0), ("const", 10, False))
    ovf = ("cmp", "gt", ("arith", "plus", ("col", 0),
                         ("const", INT64_MAX, False)), ("const", 0, False))
    rows = [{1: 100}, {1: 0}, {1: -5}, {1: None}]
    o = orc()
    assert ref_count([lt, ovf], rows, schema) == 2
    assert oracle_count(o, [lt, ovf], rows, schema) == 2
    assert ref_count([ovf, lt], rows, schema) == "error"
    assert oracle_count(o, [ovf, lt], rows, schema) == "error"
    # one AND inside one condition evaluates both sides on every row
    both = [("and", lt, ovf)]
    assert ref_count(both, rows, schema) == "error"
    assert oracle_count(o, both, rows, schema) == "error"


def test_project_datum_forms_follow_the_reference_model():
    """columns a predicate names come back decoded (flags 3 / 4), the others
    as their cells were written (8 / 9), a default as its datum: the model
    test_selection_ref.py holds the engine's project to"""
    rng = random.Random(5)
    schema = [ColSpec(1, False, -7), ColSpec(2, True, 2**63 + 1),
              ColSpec(3, False), ColSpec(4, True)]
    rows = gen_rows(rng, schema, N_ROWS, p_edge=0.3)
    conds = [("cmp", "lt", ("col", 0), ("col", 1))]
    host = region_for(rows, schema)
    req = (tikv_amd.DagSelect([c.col() for c in schema])
           .where(*[to_expr(c, schema) for c in conds])
           .output([0, 1, 2, 3]).build())
    data, n = orc().dag_run(req, *host[:5])
    want = project_ref(conds, rows, schema, [0, 1, 2, 3])
    assert 0 < len(want) < N_ROWS
    assert split_int_rows(data, 4) == want and n == len(want)
