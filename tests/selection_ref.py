"""An exact reference for the native int selection predicates, independent
of the oracle, and a seeded generator of programs and rows.

The evaluator works on dict rows {col_id: int-or-None} with Python integers,
so nothing wraps: an arithmetic result is computed exactly and then checked
against the range of its type, which is BIGINT UNSIGNED when either operand's
field type is unsigned and BIGINT otherwise (map_int_sig picks the IntInt /
IntUint / UintInt / UintUint variant from the same flags). A signed cell is
an int in [-2^63, 2^63-1], an unsigned one an int in [0, 2^64-1].

A predicate is a tree of tuples:
  ("col", offset)            ("const", value, unsigned)        ("null",)
  ("cmp", "lt|le|gt|ge|eq|ne", l, r)      ("arith", "plus|minus|mul", l, r)
  ("and", l, r)  ("or", l, r)  ("not", x)
  ("isnull", x)  ("istrue", x)  ("isfalse", x)
A selection is a list of such trees, applied in order.
"""
import random

import tikv_amd
from tikv_amd import _ffi as F

from group_multi_util import build_region
from topn_multi_util import INT64_MAX, INT64_MIN, U64, int_datum, uint_datum

MAX_NODES = 16      # COPR_MAX_RPN
MAX_DEPTH = 4       # the device evaluator's stack


class RefOverflow(Exception):
    """an arithmetic result outside the range of its type"""


class RefAmbiguous(Exception):
    """negative signed factor times unsigned 0: exact arithmetic gives 0, the
    Int x Uint multiply variants are believed to fail; not pinned"""


class ColSpec:
    """one scan column: an absent cell takes `default` (None = NULL)"""

    def __init__(self, col_id, unsigned=False, default=None):
        self.col_id = col_id
        self.unsigned = unsigned
        self.default = default

    def cell(self, row):
        return row[self.col_id] if self.col_id in row else self.default

    def col(self):
        dv = None
        if self.default is not None:
            dv = (uint_datum if self.unsigned else int_datum)(self.default)
        return tikv_amd.Col(self.col_id,
                            flag=F.FLAG_UNSIGNED if self.unsigned else 0,
                            default_val=dv)


# ---- the evaluator ----------------------------------------------------------
_CMP = {"lt": lambda a, b: a < b, "le": lambda a, b: a <= b,
        "gt": lambda a, b: a > b, "ge": lambda a, b: a >= b,
        "eq": lambda a, b: a == b, "ne": lambda a, b: a != b}


def node_unsigned(t, schema):
    """the UNSIGNED flag of a node's field type"""
    k = t[0]
    if k == "col":
        return schema[t[1]].unsigned
    if k == "const":
        return t[2]
    if k == "arith":
        return node_unsigned(t[2], schema) or node_unsigned(t[3], schema)
    return False


def evaluate(t, row, schema):
    """value of one node on one row: None (NULL) or an exact int"""
    k = t[0]
    if k == "col":
        return schema[t[1]].cell(row)
    if k == "const":
        return t[1]
    if k == "null":
        return None
    if k == "cmp":
        a, b = evaluate(t[2], row, schema), evaluate(t[3], row, schema)
        if a is None or b is None:
            return None
        return 1 if _CMP[t[1]](a, b) else 0
    if k == "arith":
        a, b = evaluate(t[2], row, schema), evaluate(t[3], row, schema)
        if a is None or b is None:
            return None
        lu, ru = node_unsigned(t[2], schema), node_unsigned(t[3], schema)
        r = a + b if t[1] == "plus" else a - b if t[1] == "minus" else a * b
        if t[1] == "mul" and lu != ru:
            s, u = (b, a) if lu else (a, b)
            if s < 0 and u == 0:
                raise RefAmbiguous()
        lo, hi = (0, U64) if lu or ru else (INT64_MIN, INT64_MAX)
        if r < lo or r > hi:
            raise RefOverflow()
        return r
    if k == "and":          # impl_op.rs logical_and
        a, b = evaluate(t[1], row, schema), evaluate(t[2], row, schema)
        if a == 0 or b == 0:
            return 0
        return None if a is None or b is None else 1
    if k == "or":
        a, b = evaluate(t[1], row, schema), evaluate(t[2], row, schema)
        if (a is not None and a != 0) or (b is not None and b != 0):
            return 1
        return None if a is None or b is None else 0
    a = evaluate(t[1], row, schema)
    if k == "not":
        return None if a is None else 1 if a == 0 else 0
    if k == "isnull":
        return 1 if a is None else 0
    if k == "istrue":
        return 1 if a is not None and a != 0 else 0
    if k == "isfalse":
        return 1 if a is not None and a == 0 else 0
    raise AssertionError("unknown node %r" % (k,))


def select(conds, rows, schema):
    """indices of the rows a selection keeps. Conditions apply in order and a
    later one sees only the rows every earlier one kept. Raises RefAmbiguous
    if any evaluated row is ambiguous, else RefOverflow if any overflows."""
    live = list(range(len(rows)))
    overflow = False
    for c in conds:
        kept = []
        for i in live:
            try:
                v = evaluate(c, rows[i], schema)
            except RefOverflow:
                overflow = True
                continue
            if v is not None and v != 0:
                kept.append(i)
        live = kept
    if overflow:
        raise RefOverflow()
    return live


def out_datum(cs, row, decoded, v2=False):
    """one response cell in split_int_rows form. A column an expression
    decoded comes back as flag 3, or 4 when unsigned; any other as it was
    stored: a row-v1 cell or a default datum as 8 / 9, a row-v2 cell, which
    has no datum form of its own, as 3 / 4."""
    v = cs.cell(row)
    if v is None:
        return (0, None)
    if decoded or (v2 and cs.col_id in row):
        return (4 if cs.unsigned else 3, v)
    return (9 if cs.unsigned else 8, v)


def project_ref(conds, rows, schema, out_offs, v2=False):
    """the kept rows of a plain project in split_int_rows form; the columns
    the conditions name are the decoded ones"""
    named = set()
    for c in conds:
        columns_of(c, named)
    return [tuple(out_datum(schema[off], rows[i], off in named, v2)
                  for off in out_offs)
            for i in select(conds, rows, schema)]


# ---- trees as requests ------------------------------------------------------
_SIG = {"lt": F.SIG_LT_INT, "le": F.SIG_LE_INT, "gt": F.SIG_GT_INT,
        "ge": F.SIG_GE_INT, "eq": F.SIG_EQ_INT, "ne": F.SIG_NE_INT,
        "plus": F.SIG_PLUS_INT, "minus": F.SIG_MINUS_INT,
        "mul": F.SIG_MULTIPLY_INT, "and": F.SIG_LOGICAL_AND,
        "or": F.SIG_LOGICAL_OR, "not": F.SIG_UNARY_NOT,
        "isnull": F.SIG_INT_IS_NULL, "istrue": F.SIG_INT_IS_TRUE,
        "isfalse": F.SIG_INT_IS_FALSE}


def _emit(t, schema, e):
    k = t[0]
    if k == "col":
        e.col(t[1])
    elif k == "const":
        e.const_int(t[1], unsigned=t[2])
    elif k == "null":
        e.const_null()
    elif k in ("cmp", "arith"):
        _emit(t[2], schema, e)
        _emit(t[3], schema, e)
        uns = k == "arith" and node_unsigned(t, schema)
        e.func(_SIG[t[1]], 2, ft=tikv_amd.field_type(
            F.TP_LONGLONG, F.FLAG_UNSIGNED if uns else 0))
    elif k in ("and", "or"):
        _emit(t[1], schema, e)
        _emit(t[2], schema, e)
        e.func(_SIG[k], 2)
    else:
        _emit(t[1], schema, e)
        e.func(_SIG[k], 1)


def to_expr(t, schema):
    e = tikv_amd.Expr()
    _emit(t, schema, e)
    return e


def n_nodes(t):
    return 1 + sum(n_nodes(c) for c in t[1:] if isinstance(c, tuple))


def depth(t):
    """stack slots the postfix form of the tree needs"""
    kids = [c for c in t[1:] if isinstance(c, tuple)]
    if not kids:
        return 1
    return max(depth(c) + i for i, c in enumerate(kids))


def columns_of(t, out=None):
    out = set() if out is None else out
    if t[0] == "col":
        out.add(t[1])
    for c in t[1:]:
        if isinstance(c, tuple):
            columns_of(c, out)
    return out


def device_nodes(conds):
    """nodes of the flattened device program: one gate between conditions"""
    return sum(n_nodes(c) for c in conds) + len(conds) - 1


# ---- the generator ----------------------------------------------------------
EDGE_SIGNED = [INT64_MIN, INT64_MIN + 1, -1, 0, 1, 2**31, 2**32,
               INT64_MAX - 1, INT64_MAX]
EDGE_UNSIGNED = [0, 1, 2**31, 2**32, INT64_MAX - 1, INT64_MAX,
                 2**63, 2**63 + 1, U64 - 1, U64]
SMALL = 40          # modest cell values and small constants lie in +-SMALL


class Gen:
    """random selections over the first `n_cols` columns of `schema`, of at
    most `max_cols` distinct columns each"""

    def __init__(self, seed, schema, n_cols=4, max_cols=4, p_arith=0.25,
                 p_edge_const=0.08, p_null_const=0.03):
        self.rng = random.Random(seed)
        self.schema = schema
        self.n_cols = n_cols
        self.max_cols = max_cols
        self.p_arith = p_arith
        self.p_edge_const = p_edge_const
        self.p_null_const = p_null_const

    def _leaf(self, cols):
        r = self.rng
        x = r.random()
        if x < 0.55:
            return ("col", r.choice(cols))
        x = r.random()
        uns = r.random() < 0.4
        if x < self.p_null_const:
            return ("null",)
        if x < self.p_null_const + self.p_edge_const:
            return ("const", r.choice(EDGE_UNSIGNED if uns else EDGE_SIGNED), uns)
        return ("const", r.randrange(0 if uns else -SMALL, SMALL), uns)

    def _val(self, cols, budget):
        r = self.rng
        if budget >= 3 and r.random() < self.p_arith:
            op = r.choice(["plus", "minus", "mul"])
            return ("arith", op, self._val(cols, budget - 2),
                    self._val(cols, (budget - 1) // 2))
        return self._leaf(cols)

    def _bool(self, cols, budget):
        r = self.rng
        x = r.random()
        if budget >= 7 and x < 0.25:
            half = (budget - 1) // 2
            return (r.choice(["and", "or"]), self._bool(cols, half),
                    self._bool(cols, half))
        if budget >= 4 and x < 0.35:
            return ("not", self._bool(cols, budget - 1))
        if x < 0.45:
            return (r.choice(["isnull", "istrue", "isfalse"]),
                    self._val(cols, budget - 1))
        if x < 0.48:
            return self._val(cols, budget)      # a bare value: as_mysql_bool
        return ("cmp", r.choice(sorted(_CMP)), self._val(cols, budget - 2),
                self._val(cols, (budget - 1) // 2))

    def selection(self, min_cols=1):
        """a list of 1..3 condition trees within the device limits that names
        min_cols..max_cols distinct columns"""
        r = self.rng
        while True:
            n_conds = r.choice([1, 1, 1, 2, 2, 3])
            cols = r.sample(range(self.n_cols),
                            r.randint(min_cols, min(self.max_cols, self.n_cols)))
            budget = (MAX_NODES - (n_conds - 1)) // n_conds
            conds = [self._bool(cols, budget) for _ in range(n_conds)]
            used = set()
            for c in conds:
                columns_of(c, used)
            if (min_cols <= len(used) <= self.max_cols
                    and device_nodes(conds) <= MAX_NODES
                    and all(depth(c) <= MAX_DEPTH for c in conds)):
                return conds


def gen_rows(rng, schema, n, p_edge=0.0, p_null=0.08, p_absent=0.08,
             n_pred_cols=4):
    """n dict rows over the first n_pred_cols columns of schema: modest
    values, a share of edge values, NULL cells and absent cells"""
    rows = []
    for _ in range(n):
        row = {}
        for cs in schema[:n_pred_cols]:
            x = rng.random()
            if x < p_absent:
                continue
            if x < p_absent + p_null:
                row[cs.col_id] = None
            elif rng.random() < p_edge:
                row[cs.col_id] = rng.choice(
                    EDGE_UNSIGNED if cs.unsigned else EDGE_SIGNED)
            else:
                row[cs.col_id] = rng.randrange(0 if cs.unsigned else -SMALL,
                                               SMALL)
        rows.append(row)
    return rows


def gen_schema(rng, n_cols=4):
    """columns 1..n_cols, each unsigned with probability 0.4 and with a
    default (modest or edge) with probability 0.5"""
    out = []
    for c in range(1, n_cols + 1):
        uns = rng.random() < 0.4
        d = None
        if rng.random() < 0.5:
            d = (rng.choice(EDGE_UNSIGNED if uns else EDGE_SIGNED)
                 if rng.random() < 0.1
                 else rng.randrange(0 if uns else -SMALL, SMALL))
        out.append(ColSpec(c, uns, d))
    return out


EDGE_SHARES = [0, 0, 0, 0.002, 0.3]


def region_for(rows, schema, v2=False):
    """the region arrays of dict rows under a schema"""
    return build_region(rows, unsigned={c.col_id for c in schema if c.unsigned},
                        v2=v2)
