"""count(*) WHERE col IN (...) over a split 32-bit plane (DESIGN.md §9p,
k_plane_ins) and the one-dispatch finish of the narrow IN kernels, against a
plain Python reference over exact integers. A region holds two full
grid-stride steps at COPR_IN_GRID=1 plus one row (the clamped last vector)."""
import random

import pytest

import tikv_amd
from tikv_amd import in_col_consts as IN

from selection_ref import ColSpec, region_for
from topn_multi_util import INT64_MAX, split_int_rows

pytestmark = pytest.mark.gpu

N = 2 * 256 * 4 * 8 + 1          # block x loads per lane x rows per 16 B
SCHEMA = [ColSpec(1)]
UNMATCHABLE = (2**63 + 5, True)
_RAW = {}


def kept(rows, items, negate):
    """rows the selection keeps: exact integers, three-valued IN"""
    exact = {i[0] if isinstance(i, tuple) else i for i in items if i is not None}
    if negate and None in items:
        return 0
    return sum((r[1] in exact) != negate for r in rows if r[1] is not None)


def plane(shape, base):
    """(rows, items) of one split-plane region"""
    span = 70000 if shape == "dense" else 2 * 10**9
    rng = random.Random(len(shape))
    vals = [base + rng.randrange(span + 1) for _ in range(N)]
    if shape == "hull":          # sorted: whole waves lie outside the hull
        vals.sort()
    vals[0], vals[N - 1] = base, base + span
    picks = [vals[i] for i in (1, 300, 5000, N // 2, N // 2 + 1, 8191, 8192, N - 2)]
    if shape == "dense":         # keys in both buckets: every row is open
        items = picks + [base + d for d in (0, 1, 0xFFFF, 0x10000, 69999, span)]
    elif shape == "none":        # every key outside [base, base + span]
        items = [base - 1, base - 65536, base + span + 1]
    elif shape == "hull":
        items = [v + d for v in picks[3:5] for d in (-1, 0, 1)]
    else:
        items = [v + d for v in picks for d in (0, 1, -1, 65536, -65536)]
        items += [base + d for d in (0xFFFF, 0x10000, -1, 0, span, span + 1)]
    items = [i for i in items if -2**63 <= i <= INT64_MAX] + [UNMATCHABLE]
    return [{1: v} for v in vals], items


def raw_of(key, rows):
    if key not in _RAW:
        _RAW[key] = region_for(rows, SCHEMA)[:5]
    return _RAW[key]


def count_req(items, negate):
    return (tikv_amd.DagSelect([c.col() for c in SCHEMA])
            .where(IN(0, items, negate))
            .simple_agg([tikv_amd.count_star()]).build())


def run(engine, monkeypatch, req, rgns, **env):
    """one request under the switches given; (bytes, in_split launches,
    one-dispatch waits, fallbacks) it added"""
    for k in ("COPR_NO_IN_SPLIT", "COPR_NO_IN_PLANES", "COPR_FC_POLL_US",
              "COPR_NARROW_NO_FINALIZE", "COPR_NO_NARROW", "COPR_NO_PLANES"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("COPR_IN_GRID", "1")
    monkeypatch.setenv("COPR_PLANE_BUDGET_MB", "64")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s0, w0 = engine.in_split_launches(), engine.fc_wait_stats()
    data = engine.dag_run(req, rgns)[0]
    w1 = engine.fc_wait_stats()
    return (data, engine.in_split_launches() - s0, sum(w1) - sum(w0),
            w1[1] - w0[1])


CASES = [(s, b, n, False) for s in ("sparse", "dense", "none", "hull")
         for b in (-10**9, INT64_MAX - 2 * 10**9 - 5) for n in (False, True)]
CASES.append(("sparse", -10**9, True, True))       # NOT IN with a NULL: never


@pytest.mark.parametrize("shape,base,negate,with_null", CASES)
def test_split_plane_in(engine, monkeypatch, shape, base, negate, with_null):
    rows, items = plane(shape, base)
    if with_null:
        items = items + [None]
    want = kept(rows, items, negate)
    if shape != "none" and not with_null:
        assert 0 < want < N
    req = count_req(items, negate)
    rgn = engine.region_raw(*raw_of((shape, base), rows))
    try:
        data, split, waits, fell = run(engine, monkeypatch, req, [rgn])
        assert split_int_rows(data, 1) == [((3, want),)]
        assert (split, waits) == (1, 1)
        assert run(engine, monkeypatch, req, [rgn], COPR_FC_POLL_US="0") == \
            (data, 1, 1, 1)
        assert run(engine, monkeypatch, req, [rgn], COPR_NO_IN_SPLIT="1") == \
            (data, 0, 0, 0)
        assert run(engine, monkeypatch, req, [rgn], COPR_NO_IN_PLANES="1") == \
            (data, 0, 0, 0)
    finally:
        rgn.close()


@pytest.mark.parametrize("parts,one_dispatch", [
    (("split", "w2"), True), (("split", "w2", "null"), False),
    (("w1", "w2"), True)])
def test_regions(engine, monkeypatch, parts, one_dispatch):
    """first launch stamps, last finalizes, whichever kernel each takes; a
    region without a narrow plane sends the request down the ordinary
    sequence"""
    base, spans = -10**9, {"split": 2 * 10**9, "w2": 60000, "w1": 200,
                           "null": 2 * 10**9}
    rng = random.Random(3)
    regions = {k: [{1: base + rng.randrange(s + 1)} for _ in range(N)]
               for k, s in spans.items()}
    regions["null"][7][1] = None
    items = [regions[k][i][1] + d for k in ("split", "w2", "w1")
             for i in (0, 4097, N - 1) for d in (0, 1)]
    req = count_req(items, False)
    rgns = [engine.region_raw(*raw_of(k, regions[k])) for k in parts]
    try:
        want = sum(kept(regions[k], items, False) for k in parts)
        data, split, waits, _ = run(engine, monkeypatch, req, rgns)
        assert split_int_rows(data, 1) == [((3, want),)]
        assert split == sum(k == "split" for k in parts)
        assert waits == (1 if one_dispatch else 0)
        assert run(engine, monkeypatch, req, rgns, COPR_NO_IN_PLANES="1")[0] \
            == data
    finally:
        for rgn in rgns:
            rgn.close()
