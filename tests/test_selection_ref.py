"""The engine's int selection predicates against the exact Python reference
of selection_ref.py, at every site that evaluates a predicate on the device
(DESIGN.md §9k): the accumulate step of k_scan_agg and k_scan_agg_pipe
(simple and hash aggregation), k_scan_project, and k_scan_extract (TopN,
stream aggregation), with the predicate's third and fourth column arriving
through the extra-capture channels. The oracle is not consulted here;
test_selection_ref_cpu.py holds it to the same reference.

Regions have 2 * 1024 + 261 rows: two full scan tiles and a ragged tail."""
import copy
import itertools
import random
import zlib

import pytest

import tikv_amd

from group_multi_util import Key, group_ref, rows_of
from selection_ref import (ColSpec, Gen, RefAmbiguous, RefOverflow, columns_of,
                           gen_rows, node_unsigned, out_datum, project_ref, region_for, select,
                           to_expr)
from topn_multi_util import INT64_MAX, U64, split_int_rows

pytestmark = pytest.mark.gpu

N = 2 * 1024 + 261
N_PROGRAMS = 30                  # per region; two regions per site
G_OFF, V_OFF = 4, 5              # group column (id 5), value column (id 6)
AGGS = [("count_star",), ("count", 5), ("max", 6), ("min", 6)]
SALT = "a"                       # part of every program seed
OVERFLOW = "row parse error on device"


def schema_of(edge_default=False):
    """columns 1..4 feed predicates: 2 and 4 unsigned, 1 and 4 with a default.
    Column 5 is a low-cardinality group key with NULLs, column 6 a value that
    is unique per row: neither is ever absent."""
    return [ColSpec(1, False, -7), ColSpec(2, True), ColSpec(3, False),
            ColSpec(4, True, 2**63 + 1 if edge_default else 9),
            ColSpec(5), ColSpec(6)]


class Data:
    """one region's rows with the reference's verdict per program, computed
    once and shared by the sites"""

    def __init__(self, p_edge, v2=False):
        rng = random.Random(int(p_edge * 1000) + (7 if v2 else 0))
        self.schema = schema_of(edge_default=v2)
        self.v2 = v2
        self.p_edge = p_edge
        self.rows = gen_rows(rng, self.schema, N, p_edge=p_edge)
        vs = list(range(-N // 2, N - N // 2))
        rng.shuffle(vs)
        for i, r in enumerate(self.rows):
            g = (i // 37) % 5
            r[5] = None if g == 4 else g - 1
            r[6] = vs[i] * 3
        self._memo = {}

    def region(self, engine):
        self.host = region_for(self.rows, self.schema, v2=self.v2)
        return engine.region_raw(*self.host[:5])

    def programs(self, tag, max_cols=4):
        """(conds, kept row indices or "error"), ambiguous programs left out.
        The seed takes in the site's tag and the region, so a site sees
        2 * N_PROGRAMS distinct programs over its two regions and no two
        sites share any; every other program names at least 3 columns when
        it may."""
        key = tag
        if key not in self._memo:
            out = []
            for k in range(N_PROGRAMS):
                seed = zlib.crc32(("%s%s/%s/%s/%d" % (SALT, tag, self.p_edge, self.v2,
                                                    k)).encode())
                g = Gen(seed, self.schema, max_cols=max_cols)
                conds = g.selection(
                    min_cols=3 if max_cols >= 3 and k % 2 == 0 else 1)
                try:
                    out.append((conds, select(conds, self.rows, self.schema)))
                except RefOverflow:
                    out.append((conds, "error"))
                except RefAmbiguous:
                    pass
            self._memo[key] = out
        return self._memo[key]


_DATA = {}


def data(p_edge, v2=False):
    if (p_edge, v2) not in _DATA:
        _DATA[(p_edge, v2)] = Data(p_edge, v2)
    return _DATA[(p_edge, v2)]


P_EDGE = [0.0, 0.004]


def agg_defs():
    return [tikv_amd.count_star(), tikv_amd.count_col(G_OFF),
            tikv_amd.max_col(V_OFF), tikv_amd.min_col(V_OFF)]


def select_req(schema, conds):
    return (tikv_amd.DagSelect([c.col() for c in schema])
            .where(*[to_expr(c, schema) for c in conds]))


# ---- what each site returns for a set of kept rows -------------------------
def simple_want(rows):
    got = group_ref(rows, [], AGGS)
    return got if got else [((3, 0), (3, 0), (0, None), (0, None))]


def hash_want(rows):
    return group_ref(rows, [Key(5)], AGGS)


def stream_want(rows):
    out = []
    for _, run in itertools.groupby(rows, key=lambda r: r[5]):
        out += group_ref(list(run), [Key(5)], AGGS)
    return out


def topn_want(d, conds, kept, n, desc):
    """ORDER BY column 6 LIMIT n over all six columns: the order column and
    the columns the predicate names come back decoded"""
    named = set([V_OFF])
    for c in conds:
        columns_of(c, named)
    rows = sorted((d.rows[i] for i in kept), key=lambda r: r[6], reverse=desc)
    return [tuple(out_datum(cs, r, off in named, d.v2)
                  for off, cs in enumerate(d.schema)) for r in rows[:n]]


class Site:
    """one evaluation site: the request it sends and its reference"""

    def __init__(self, name, max_cols=4):
        self.name = name
        self.max_cols = max_cols

    def req(self, d, conds, k=0):
        ds = select_req(d.schema, conds)
        if self.name == "simple":
            return ds.simple_agg(agg_defs()).build()
        if self.name == "hash":
            return ds.hash_agg(agg_defs(), tikv_amd.Expr().col(G_OFF)).build()
        if self.name == "stream":
            return ds.stream_agg(agg_defs(), tikv_amd.Expr().col(G_OFF)).build()
        if self.name == "topn":
            return ds.topn(tikv_amd.Expr().col(V_OFF), 50, desc=k % 2 == 1).build()
        return ds.output(list(range(6))).build()

    def got(self, data, n):
        if self.name == "hash":
            rows = rows_of(data, 5)
        else:
            rows = split_int_rows(data, 6 if self.name in ("topn", "project") else
                                  4 if self.name == "simple" else 5)
        assert len(rows) == n
        return rows

    def want(self, d, conds, kept, k=0):
        rows = [d.rows[i] for i in kept]
        if self.name == "simple":
            return simple_want(rows)
        if self.name == "hash":
            return hash_want(rows)
        if self.name == "stream":
            return stream_want(rows)
        if self.name == "topn":
            return topn_want(d, conds, kept, 50, k % 2 == 1)
        return project_ref(conds, d.rows, d.schema, list(range(6)), d.v2)


def unsigned_arith(t, schema):
    """does the tree hold arithmetic with an unsigned operand"""
    if t[0] == "arith" and node_unsigned(t, schema):
        return True
    return any(unsigned_arith(c, schema) for c in t[1:] if isinstance(c, tuple))


def check_site(engine, site, d, tag=None):
    rgn = d.region(engine)
    try:
        n_err = n_some = n_uarith = n_xcap = 0
        for k, (conds, kept) in enumerate(d.programs(tag or site.name,
                                                     site.max_cols)):
            req = site.req(d, conds, k)
            n_uarith += any(unsigned_arith(c, d.schema) for c in conds)
            named = set()
            for c in conds:
                columns_of(c, named)
            n_xcap += len(named) >= 3
            if kept == "error":
                n_err += 1
                with pytest.raises(RuntimeError, match=OVERFLOW):
                    engine.dag_run(req, [rgn])
                continue
            n_some += 0 < len(kept) < N
            data, n, _ = engine.dag_run(req, [rgn])
            assert site.got(data, n) == site.want(d, conds, kept, k), \
                "program %d: %r" % (k, conds)
        assert n_some >= 5, "the programs say too little"
        assert n_err >= 1, "no program raises"
        assert n_uarith >= 3, "too little unsigned arithmetic"
        assert site.max_cols < 3 or n_xcap >= 10, "too few 3- and 4-column programs"
    finally:
        rgn.close()


# ---- generated programs at every site -----------------------------------------
@pytest.mark.parametrize("no_pipe", [False, True])
@pytest.mark.parametrize("p_edge", P_EDGE)
def test_simple_agg(engine, monkeypatch, p_edge, no_pipe):
    """k_scan_agg_pipe by default, k_scan_agg under COPR_NO_PIPE=1"""
    if no_pipe:
        monkeypatch.setenv("COPR_NO_PIPE", "1")
    else:
        monkeypatch.delenv("COPR_NO_PIPE", raising=False)
    check_site(engine, Site("simple"), data(p_edge),
               "simple_nopipe" if no_pipe else "simple")


@pytest.mark.parametrize("p_edge", P_EDGE)
def test_hash_agg(engine, p_edge):
    check_site(engine, Site("hash"), data(p_edge))


@pytest.mark.parametrize("p_edge", P_EDGE)
def test_project(engine, p_edge):
    check_site(engine, Site("project", max_cols=2), data(p_edge))


@pytest.mark.parametrize("p_edge", P_EDGE)
def test_topn(engine, p_edge):
    check_site(engine, Site("topn"), data(p_edge))


@pytest.mark.parametrize("p_edge", P_EDGE)
def test_stream_agg(engine, p_edge):
    check_site(engine, Site("stream"), data(p_edge))


@pytest.mark.parametrize("site", ["simple", "topn"])
def test_row_v2(engine, site):
    check_site(engine, Site(site), data(0.004, v2=True))


# ---- TopN behind the fused comparers ---------------------------------------------
def test_topn_two_fused_comparers_decode_both_columns(engine):
    """two cmp(col, const) conditions on different columns take the fused
    fast path, not the RPN evaluator; the selection decoded both columns, so
    TopN returns both in decoded form, like the order column"""
    d = data(0.0)
    conds = [("cmp", "gt", ("col", 0), ("const", -20, False)),
             ("cmp", "lt", ("col", 1), ("const", 30, True))]
    kept = select(conds, d.rows, d.schema)
    assert 50 < len(kept) < N
    s = Site("topn")
    rgn = d.region(engine)
    try:
        for k in (0, 1):
            data_, n, _ = engine.dag_run(s.req(d, conds, k), [rgn])
            assert s.got(data_, n) == s.want(d, conds, kept, k)
    finally:
        rgn.close()


# ---- one overflowing row, placed -------------------------------------------------
C1, C2, C3, C4 = (("col", i) for i in range(4))
# c1 < c3 OR c2 + c4 > 5: the sum's operands are the third and fourth column
# the program names, so they arrive through the extra-capture channels
PLACED4 = [("or", ("cmp", "lt", C1, C3),
            ("cmp", "gt", ("arith", "plus", C2, C4), ("const", 5, False)))]
PLACED2 = [("cmp", "gt", ("arith", "plus", C2, C4), ("const", 5, False))]


@pytest.mark.parametrize("site", ["simple", "simple_nopipe", "hash", "project",
                                  "topn", "stream"])
def test_one_overflowing_row(engine, monkeypatch, site):
    """column 2 = 2^64-1 and column 4 = 1 in exactly one row, at the first
    row, either side of a tile boundary, and the last row: the request fails.
    With column 2 = 7 there it equals the reference."""
    if site == "simple_nopipe":
        monkeypatch.setenv("COPR_NO_PIPE", "1")
        site = "simple"
    else:
        monkeypatch.delenv("COPR_NO_PIPE", raising=False)
    s = Site(site)
    conds = PLACED2 if site == "project" else PLACED4
    base = data(0.0)
    for idx in (0, 1023, 1024, N - 1):
        d = copy.copy(base)
        d.rows = list(base.rows)
        d.rows[idx] = {**base.rows[idx], 1: 1, 2: U64, 3: 5, 4: 1}
        with pytest.raises(RefOverflow):
            select(conds, d.rows, d.schema)
        rgn = d.region(engine)
        try:
            with pytest.raises(RuntimeError, match=OVERFLOW):
                engine.dag_run(s.req(d, conds), [rgn])
        finally:
            rgn.close()
        d.rows[idx] = {**d.rows[idx], 2: 7}
        kept = select(conds, d.rows, d.schema)
        assert idx in kept and 0 < len(kept) < N
        rgn = d.region(engine)
        try:
            data_, n, _ = engine.dag_run(s.req(d, conds), [rgn])
            assert s.got(data_, n) == s.want(d, conds, kept)
        finally:
            rgn.close()


# ---- conditions apply in order -----------------------------------------------------
FIRST = ("cmp", "lt", C1, ("const", 10, False))
# overflows for c1 > 10, rows FIRST drops
SECOND = ("cmp", "gt", ("arith", "plus", C1, ("const", INT64_MAX - 10, False)),
          ("const", 0, False))
THIRD4 = ("cmp", "ge", ("arith", "mul", C2, C4), C3)
THIRD2 = ("cmp", "gt", C2, ("const", 3, False))


@pytest.mark.parametrize("site", ["simple", "simple_nopipe", "hash", "project",
                                  "topn", "stream"])
def test_later_condition_sees_only_kept_rows(engine, monkeypatch, site):
    if site == "simple_nopipe":
        monkeypatch.setenv("COPR_NO_PIPE", "1")
        site = "simple"
    else:
        monkeypatch.delenv("COPR_NO_PIPE", raising=False)
    s = Site(site)
    d = data(0.0)
    third = THIRD2 if site == "project" else THIRD4
    conds = [FIRST, SECOND, third]
    kept = select(conds, d.rows, d.schema)
    assert 0 < len(kept) < N
    assert any(r.get(1, -7) is not None and r.get(1, -7) > 10 for r in d.rows)
    for wrong in ([SECOND, FIRST, third], [("and", FIRST, SECOND), third]):
        with pytest.raises(RefOverflow):
            select(wrong, d.rows, d.schema)
    rgn = d.region(engine)
    try:
        data_, n, _ = engine.dag_run(s.req(d, conds), [rgn])
        assert s.got(data_, n) == s.want(d, conds, kept)
        for wrong in ([SECOND, FIRST, third], [("and", FIRST, SECOND), third]):
            with pytest.raises(RuntimeError, match=OVERFLOW):
                engine.dag_run(s.req(d, wrong), [rgn])
    finally:
        rgn.close()
