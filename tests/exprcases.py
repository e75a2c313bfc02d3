"""Expressions, tables and a plain integer model for tests/test_expr_edges_host.py and tests/test_gpu_expr_edges.py: the scalar
expression language at its value edges - 64-bit wraps, truncating division, rescaling casts that wrap, INT -> BIGINT sign extension,
signed comparisons after rescaling, CASE with the reference's super type, the division error word - and every typed form of the
register aggregation's range-typed arithmetic (codegen_internal.h ExprGen::emitTyped / arithTV) at the ends of its envelope.

Expressions are nested tuples: ("col", name), ("const", text, category), ("add" | "sub" | "mul" | "div", a, b), ("cast", type, a),
("lt" | "le" | "gt" | "ge" | "eq" | "neq", a, b), ("and" | "or", a, b), ("case", ((when, then), ...), else or None).  `derive` types
a tuple tree the way expr.cpp's Deriver does (implicit casts become nodes of their own), `evaluate` computes it over Python integers;
neither knows anything of the engine.  Every table is 300 rows - two 128-row tiles and a 44-row tail - with the interesting values in
rows 0-7 in all pairings of the operands' ends, again at rows 126-129 and in the last two rows."""
import os
import sys

import numpy as np

from resql_amd import plan as P

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import narrowcases as N  # noqa: E402

T = P.TypeInit
ROWS = 300
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
M31 = I32_MAX
BIGINT, INTT, DATE, BOOL = T.BIGINT(), T.INT(), T.DATE(), T.BOOL()
ARITH = ("add", "sub", "mul", "div")
COMPARE = ("lt", "le", "gt", "ge", "eq", "neq")


def col(name): return ("col", name)
def dec(text): return ("const", text, P.DECIMAL)
def big(text): return ("const", str(text), P.BIGINT)
def date(text): return ("const", text, P.DATE)
def add(a, b): return ("add", a, b)
def sub(a, b): return ("sub", a, b)
def mul(a, b): return ("mul", a, b)
def div(a, b): return ("div", a, b)
def cast(type_, a): return ("cast", type_, a)
def case(whens, else_=None): return ("case", tuple(whens), else_)
def cmp(op, a, b): return (op, a, b)
def flag(cond): return case([(cond, big(1))], big(0))          # a comparison as a CASE condition: case when <cond> then 1 else 0 end


class Trap(Exception):
    """what the reference's generated code dies of: a zero divisor, INT64_MIN / -1"""


class Refused(Exception):
    """a statement the type derivation or the code generator refuses (RSQ_ERR_TYPE), with the engine's message"""


def wrap64(v): return (v + (1 << 63)) % (1 << 64) - (1 << 63)
def wrap32(v): return (v + (1 << 31)) % (1 << 32) - (1 << 31)
def wrap16(v): return (v + (1 << 15)) % (1 << 16) - (1 << 15)


def tdiv(a, b):
    """cqo + idiv: the quotient truncated towards zero"""
    if b == 0 or (a == I64_MIN and b == -1):
        raise Trap(f"{a} / {b}")
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


# ---- type derivation (expr.cpp Deriver) ---------------------------------------------------------------------------------------
class Node:
    """a typed expression node: kind, type, children; `value` of a constant, `name` of a column"""
    def __init__(self, kind, type_, kids=(), value=None, name=None):
        self.kind, self.type, self.kids, self.value, self.name = kind, type_, list(kids), value, name


def constant(text, category):
    """parseConstant: (raw value, type) of a literal"""
    if category == P.DECIMAL:
        digits = text.replace(".", "", 1)
        scale = len(text) - text.index(".") - 1 if "." in text else 0
        return int(digits), T.DECIMAL(len(digits), scale)
    if category == P.BIGINT:                                  # parsed through an int32_t: '4294967297' is 1
        return wrap32(max(I64_MIN, min(I64_MAX, int(text)))), BIGINT
    if category == P.INT:
        return int(text), INTT
    if category == P.DATE:
        y, m, d = text.replace("/", "-").split("-")
        return int(y) * 10000 + int(m) * 100 + int(d), DATE
    raise ValueError(category)


def _cast_node(to, child):
    """insertTypecast: a cast towards DECIMAL starts as DECIMAL(19, 0); sameScale gives it its scale later"""
    return Node("cast", T.DECIMAL(19, 0) if to.tag == P.DECIMAL else to, [child])


def _precedence(kids):
    """the operand of the lower type category is cast to the other's (the categories' enum order decides)"""
    l, r = kids
    if l.type.tag > r.type.tag:
        kids[1] = _cast_node(l.type, r)
    elif l.type.tag < r.type.tag:
        kids[0] = _cast_node(r.type, l)


def _scale_to(spec, other):
    d = other.scale - spec.scale
    return T.DECIMAL(min(19, (spec.precision + d) & 255), (spec.scale + d) & 255)


def _same_scale(kids):
    """the operand of smaller scale is cast to the larger; an operand that IS a cast is retargeted instead"""
    for i, j in ((0, 1), (1, 0)):
        if kids[i].type.scale < kids[j].type.scale:
            t = _scale_to(kids[i].type, kids[j].type)
            if kids[i].kind == "cast":
                kids[i].type = t
            else:
                kids[i] = Node("cast", t, [kids[i]])


def _numeric(op, n):
    if n.type.tag not in (P.DECIMAL, P.BIGINT, P.INT):
        raise Refused(f"Incompatible types: {op.upper()} expression requires a numeric operand")


def super_type(a, b):
    """Deriver::superType: for BIGINT / INT against DECIMAL it returns its SECOND argument, whichever that is"""
    if a.tag == b.tag:
        return T.DECIMAL(max(a.precision, b.precision), max(a.scale, b.scale)) if a.tag == P.DECIMAL else a
    if (a.tag in (P.BIGINT, P.INT) and b.tag == P.DECIMAL) or (b.tag in (P.BIGINT, P.INT) and a.tag == P.DECIMAL):
        return b
    raise Refused("Incompatible or unimplemented type combination in getCommonSuperType(..)")


def derive(e, schema):
    k = e[0]
    if k == "col":
        return Node("col", schema[e[1]], name=e[1])
    if k == "const":
        v, t = constant(e[1], e[2])
        return Node("const", t, value=v)
    if k == "cast":
        return Node("cast", e[1], [derive(e[2], schema)])
    if k in ARITH:
        kids = [derive(e[1], schema), derive(e[2], schema)]
        _numeric(k, kids[0]); _numeric(k, kids[1])
        _precedence(kids)
        t = kids[0].type
        if t.tag == P.DECIMAL:
            if k == "div":
                raise Refused("Decimal division not yet implemented")
            if k != "mul":
                _same_scale(kids)
            l, r = kids[0].type, kids[1].type
            t = (T.DECIMAL(min(19, (l.precision + r.precision) & 255), (l.scale + r.scale) & 255) if k == "mul"
                 else T.DECIMAL(min(19, (max(l.precision, r.precision) + 1) & 255), l.scale))
        return Node(k, t, kids)
    if k in COMPARE:
        kids = [derive(e[1], schema), derive(e[2], schema)]
        _precedence(kids)
        if kids[0].type.tag == P.DECIMAL:
            _same_scale(kids)
        return Node(k, BOOL, kids)
    if k in ("and", "or"):
        kids = [derive(e[1], schema), derive(e[2], schema)]
        if any(x.type.tag != P.BOOL for x in kids):
            raise Refused(f"Incompatible types: {k.upper()} expression requires bool operand")
        return Node(k, BOOL, kids)
    if k == "case":
        whens = [[derive(w, schema), derive(t, schema)] for w, t in e[1]]
        other = derive(e[2], schema) if e[2] is not None else None
        rt = whens[0][1].type
        for _, t in whens[1:]:
            rt = super_type(rt, t.type)
        if other is not None:
            rt = super_type(rt, other.type)
        same = lambda t: (t.tag, t.precision, t.scale) == (rt.tag, rt.precision, rt.scale) if t.tag == P.DECIMAL else t.tag == rt.tag
        for wt in whens:
            if not same(wt[1].type):
                wt[1] = _cast_node(rt, wt[1])
        if other is not None and not same(other.type):
            other = _cast_node(rt, other)
        n = Node("case", rt, [x for wt in whens for x in wt] + ([other] if other is not None else []))
        n.has_else = other is not None
        return n
    raise ValueError(k)


def check(n):
    """what the code generator refuses (ExprGen::emitUnary / emitBinary), with its message"""
    for c in n.kids:
        check(c)
    if n.kind == "cast":
        f, t = n.kids[0].type, n.type
        if t.tag == P.DECIMAL and f.tag == P.DECIMAL:
            if abs(t.scale - f.scale) > 8:
                raise Refused("typecast beyond the supported scale difference")
        elif t.tag == P.DECIMAL and f.tag == P.BIGINT:
            if t.scale > 8:
                raise Refused("typecast beyond the supported scale")
        elif t.tag == P.DECIMAL:
            raise Refused("emitTypecastToDECIMAL(..) code generation not implemented for datatype")
        elif t.tag == P.BIGINT and f.tag == P.DECIMAL:
            if f.scale > 8:
                raise Refused("typecast beyond the supported scale")
        elif t.tag == P.BIGINT and f.tag in (P.INT, P.BIGINT):
            pass
        elif t.tag == P.BIGINT:
            raise Refused("emitTypecastToBIGINT(..) code generation not implemented for datatype")
        else:
            raise Refused("emitTypecast(..) code generation not implemented for datatype")
    if n.kind in ARITH and n.type.tag not in (P.DECIMAL, P.BIGINT):
        raise Refused(f"{n.kind.upper()} code generation not implemented for datatype")
    if n.kind in ("lt", "le", "gt", "ge") and n.kids[0].type.tag not in (P.DECIMAL, P.DATE, P.BIGINT):
        name = {"lt": "LESS_THAN", "gt": "ADD", "le": "LE", "ge": "GE"}[n.kind]      # (the reference's own words)
        raise Refused(f"{name} code generation not implemented for datatype")
    return n


def typed(e, schema):
    return check(derive(e, schema))


def _signed(v, t):
    """the value as the comparison sees it: INT and DATE compare as signed 32-bit integers"""
    return wrap32(v) if t.tag in (P.INT, P.DATE) else v


def compute(n, row, int16=False):
    """the raw integer of a typed node over one row"""
    k = n.kind
    if k == "col":
        return row[n.name]
    if k == "const":
        return n.value
    if k == "cast":
        v, f, t = compute(n.kids[0], row, int16), n.kids[0].type, n.type
        if t.tag == P.DECIMAL:
            d = t.scale - (f.scale if f.tag == P.DECIMAL else 0)
            return wrap64(v * 10 ** d) if d >= 0 else tdiv(v, 10 ** -d)
        if f.tag == P.INT:
            return wrap16(v) if int16 else wrap32(v)
        return tdiv(v, 10 ** f.scale) if f.tag == P.DECIMAL else v
    if k == "case":                                              # (the first true WHEN; what lies behind it is not evaluated, and cannot trap)
        pairs = n.kids[:-1] if n.has_else else n.kids
        for i in range(0, len(pairs), 2):
            if compute(pairs[i], row, int16):
                return compute(pairs[i + 1], row, int16)
        return compute(n.kids[-1], row, int16) if n.has_else else 0
    a, b = compute(n.kids[0], row, int16), compute(n.kids[1], row, int16)
    if k == "add": return wrap64(a + b)
    if k == "sub": return wrap64(a - b)
    if k == "mul": return wrap64(a * b)
    if k == "div": return tdiv(a, b)
    if k == "and": return a & b
    if k == "or": return a | b
    a, b = _signed(a, n.kids[0].type), _signed(b, n.kids[1].type)
    return int({"lt": a < b, "le": a <= b, "gt": a > b, "ge": a >= b, "eq": a == b, "neq": a != b}[k])


def schema_of(t):
    return {c.name: c.type for c in t.columns}


def evaluate(e, row, schema, int16=False):
    """(raw integer, type) of the expression over one row (a dict of raw integers)"""
    n = typed(e, schema)
    return compute(n, row, int16), n.type


def functions(n, out=None):
    """the rsq:: functions the row function of a typed node calls: add / sub / mul / div, and mul for every cast that scales up"""
    out = set() if out is None else out
    for c in n.kids:
        functions(c, out)
    if n.kind in ARITH:
        out.add(f"rsq::{n.kind}(")
    if n.kind == "cast" and n.type.tag == P.DECIMAL:
        f = n.kids[0].type
        if f.tag == P.BIGINT or n.type.scale > f.scale:
            out.add("rsq::mul(")
    return out


def has_open_case(e):
    """a CASE without ELSE somewhere in the tuple tree: 0 here; the reference leaves its result register as it was (undefined)"""
    if not isinstance(e, tuple):
        return False
    if e and e[0] == "case":
        return e[2] is None or any(has_open_case(w) or has_open_case(t) for w, t in e[1]) or has_open_case(e[2])
    return any(has_open_case(x) for x in e[1:])


def rows_of(t):
    cols = {c.name: [int(v) for v in c.data] for c in t.columns}
    return [{k: v[r] for k, v in cols.items()} for r in range(t.n_rows)]


def same_type(a, b):
    return a.tag == b.tag and (a.tag != P.DECIMAL or (a.precision, a.scale) == (b.precision, b.scale))


# ---- plans --------------------------------------------------------------------------------------------------------------------
class Builder:
    """fresh plan nodes for every use of a tuple; a node that would get a second parent expression is refused"""
    def __init__(self, p):
        self.p, self.parent = p, {}

    def _own(self, parent, *kids):
        for c in kids:
            if c in self.parent:
                raise ValueError(f"expression node {c} is already the child of node {self.parent[c]}: build it again")
            self.parent[c] = parent
        return parent

    def node(self, e):
        p, k = self.p, e[0]
        if k == "col":
            return p.attr(e[1])
        if k == "const":
            return p.constant(e[1], e[2])
        if k == "cast":
            c = self.node(e[2])
            return self._own(p.typecast(e[1], c), c)
        if k == "case":
            kids = []
            for w, t in e[1]:
                wn, tn = self.node(w), self.node(t)
                kids.append(self._own(p.when_then(wn, tn), wn, tn))
            if e[2] is not None:
                kids.append(self.node(e[2]))
            return self._own(p.case(*kids), *kids)
        a, b = self.node(e[1]), self.node(e[2])
        make = {"and": p.and_, "or": p.or_}.get(k) or getattr(p, k)
        return self._own(make(a, b), a, b)

    def wrap(self, make, *kids):
        """an aggregate or AS over built nodes"""
        return self._own(make(*kids), *kids)


def projection_plan(exprs, t, where=None):
    """select k, e0 as x0, ... from t [where <where>]"""
    p = P.Plan([t])
    b = Builder(p)
    node = p.scan(t.name)
    if where is not None:
        node = p.selection(b.node(where), node)
    outs = [p.attr("k")]
    for i, e in enumerate(exprs):
        outs.append(b.wrap(lambda c, i=i: p.as_(f"x{i}", c), b.node(e)))
    return p.set_root(p.materialize(p.projection(outs, node)))


def selection_plan(cond, t):
    """select k from t where <cond>"""
    return projection_plan([], t, where=cond)


def aggregation_plan(exprs, t, sums_only=False, group="g"):
    """select g, sum(e), min(e), max(e) for e in exprs, count(*) from t group by g"""
    p = P.Plan([t])
    b = Builder(p)
    g = p.attr(group)
    aggs = []
    for e in exprs:
        for f in (("sum",) if sums_only else ("sum", "min", "max")):
            aggs.append(b.wrap(getattr(p, f), b.node(e)))
    aggs.append(p.count(p.star()))
    node = p.aggregation(aggs, [g], p.scan(t.name))
    node = p.projection([g] + [p.as_(f"x{i}", a) for i, a in enumerate(aggs)], node)
    return p.set_root(p.materialize(node))


def keyed_plan(key, t):
    """select <key> as key, count(*), sum(k) from t group by <key>: the generic hash aggregation over a computed key"""
    p = P.Plan([t])
    b = Builder(p)
    kn = b.node(key)
    cnt, sk = p.count(p.star()), p.sum(p.attr("k"))
    node = p.aggregation([cnt, sk], [kn], p.scan(t.name))
    node = p.projection([p.as_("key", kn), p.as_("n", cnt), p.as_("sk", sk)], node)
    return p.set_root(p.materialize(node))


def project_model(exprs, t, where=None, int16=False):
    """(rows as tuples of raw integers, result types) of projection_plan; Trap where a row that is evaluated traps"""
    s = schema_of(t)
    nodes = [typed(e, s) for e in exprs]
    w = typed(where, s) if where is not None else None
    out = []
    for row in rows_of(t):
        if w is not None and not compute(w, row, int16):
            continue
        out.append((row["k"],) + tuple(compute(n, row, int16) for n in nodes))
    return out, [s["k"]] + [n.type for n in nodes]


def sum_type(t):
    return T.DECIMAL(19, t.scale) if t.tag == P.DECIMAL else t


def aggregate_model(exprs, t, sums_only=False, group="g"):
    s = schema_of(t)
    nodes = [typed(e, s) for e in exprs]
    per = 1 if sums_only else 3
    groups = {}
    for row in rows_of(t):
        acc = groups.setdefault(row[group], [None] * (per * len(nodes)) + [0])
        for i, n in enumerate(nodes):
            v = compute(n, row)
            acc[per * i] = wrap64((acc[per * i] or 0) + v)
            if not sums_only:
                acc[per * i + 1] = v if acc[per * i + 1] is None else min(acc[per * i + 1], v)
                acc[per * i + 2] = v if acc[per * i + 2] is None else max(acc[per * i + 2], v)
        acc[-1] += 1
    types = [s[group]]
    for n in nodes:
        types += [sum_type(n.type)] + ([] if sums_only else [n.type, n.type])
    return sorted((g,) + tuple(a) for g, a in groups.items()), types + [BIGINT]


def keyed_model(key, t):
    s = schema_of(t)
    n = typed(key, s)
    groups = {}
    for row in rows_of(t):
        acc = groups.setdefault(compute(n, row), [0, 0])
        acc[0] += 1
        acc[1] = wrap64(acc[1] + row["k"])
    return sorted((g, a[0], a[1]) for g, a in groups.items()), [n.type, BIGINT, BIGINT]


# ---- tables -------------------------------------------------------------------------------------------------------------------
def _column(name, type_, values):
    dt = type_.np_dtype
    if type_.tag == P.DATE:
        values = [v & 0xFFFFFFFF for v in values]
    return P.Column(name, type_, np.array([int(v) for v in values], dtype=dt))


def place(n, ends, cells, stride, phase, corner_bit):
    """`n` values: rows 0-7 hold the two ends (`corner_bit` of the row number decides which, so three columns with bits 1, 2, 4 meet in
    all pairings), rows 126-129 and the last two rows hold them again (alternating, offset by `phase`), the others walk `cells`"""
    lo, hi = ends
    m = len(cells)
    v = [cells[(i * stride + phase) % m] for i in range(n)]
    for i in range(min(8, n)):
        v[i] = hi if i & corner_bit else lo
    for j, i in enumerate([126, 127, 128, 129, n - 2, n - 1]):
        if 8 <= i < n:
            v[i] = hi if ((j >> (corner_bit >> 1)) + phase) & 1 else lo
    return v


def _keys(n, seed):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 3, n).astype(np.int64)
    g[:3] = [0, 1, 2][:n]
    return [P.Column("k", BIGINT, np.arange(n, dtype=np.int64)), P.Column("g", BIGINT, g)]


# family A: 64-bit semantics
CELLS64 = sorted({0, 1, -1, 1 << 31, -(1 << 31), 1 << 32, -(1 << 32), 1 << 62, -(1 << 62), I64_MIN, I64_MIN + 1, I64_MAX}
                 | {s * (10 ** k + d) for k in range(19) for d in (-1, 0, 1) for s in (1, -1)})
DEC18 = T.DECIMAL(18, 2)


def table_a(n=ROWS):
    ends = (I64_MIN, I64_MAX)
    cols = _keys(n, 41)
    for name, ty, stride, phase, bit in (("a", BIGINT, 1, 0, 1), ("b", BIGINT, 7, 3, 2), ("c", BIGINT, 13, 5, 4),
                                         ("da", DEC18, 1, 0, 1), ("db", DEC18, 11, 2, 2), ("dc", DEC18, 17, 7, 4)):
        cols.append(_column(name, ty, place(n, ends, CELLS64, stride, phase, bit)))
    return P.Table("t", cols, n)


A_EXPRS = [
    add(col("a"), col("b")), sub(col("a"), col("b")), mul(col("a"), col("b")), mul(mul(col("a"), col("b")), col("c")),
    add(col("a"), big(2147483647)), sub(col("a"), big(-2147483648)), mul(col("a"), big(1000000007)), sub(big(-1), col("a")),
    add(col("da"), col("db")), sub(col("da"), col("db")), mul(col("da"), col("db")), mul(mul(col("da"), col("db")), col("dc")),
    add(col("da"), dec("92233720368547758.07")), mul(col("da"), dec("1000000000.01")), sub(dec("0.01"), col("da")),
    add(col("a"), col("da")),                                                       # BIGINT beside DECIMAL: cast by x 100, wrapping
]
A_CONST = [add(big(2147483647), big(2147483647)), mul(big(-2147483648), big(-2147483648)), mul(mul(big(2147483647), big(2147483647)), big(5)),
           add(dec("9223372036854775807"), dec("1")), mul(dec("3037000500.0"), dec("3037000500.0")), sub(dec("-9223372036854775807"), dec("2")),
           add(big("4294967297"), big(0)), mul(big("4294967297"), col("a"))]        # ('4294967297' is 1)
A_AGG = [add(col("a"), col("b")), mul(col("a"), col("b")), sub(col("da"), col("db"))]
A_KEY = mul(col("a"), col("b"))                                                      # 2^32 x 2^32, 2^62 x 4 ... and 0 x anything: one group


# family B: division
DIVIDENDS = [I64_MIN, I64_MIN + 1, -7, -1, 0, 1, 7, I64_MAX]
DIVISORS = [-I64_MAX, -7, -3, -1, 1, 2, 3, 7, 100, I64_MAX]
CONST_DIVISORS = [-7, -3, 1, 2, 3, 7, 100]     # (a BIGINT literal is an int32; -1 is left out: the dividends hold INT64_MIN)


def table_b(n=ROWS):
    """every dividend over every divisor (80 pairings, INT64_MIN / -1 replaced by INT64_MIN / 1), the ends' pairings where `place` puts them"""
    a = place(n, (I64_MIN, I64_MAX), [DIVIDENDS[i % 8] for i in range(80)], 1, 0, 1)
    b = place(n, (-I64_MAX, I64_MAX), [DIVISORS[i // 8] for i in range(80)], 1, 0, 2)
    b = [1 if (x, y) == (I64_MIN, -1) else y for x, y in zip(a, b)]
    return P.Table("t", _keys(n, 42) + [_column("a", BIGINT, a), _column("b", BIGINT, b)], n)


B_EXPRS = ([div(col("a"), col("b"))] + [div(col("a"), big(c)) for c in CONST_DIVISORS] + [div(big(7), col("b")), div(big(-2147483648), col("b")),
           div(big(-7), big(2)), div(big(7), big(-2)), div(col("a"), big("4294967297")), div(sub(col("a"), col("b")), big(3))])
B_PREDICATES = [cmp("gt", div(col("a"), col("b")), big(1)), cmp("eq", div(col("a"), big(-7)), big(0)), cmp("lt", div(col("a"), col("b")), big(0))]
B_AGG = [div(col("a"), col("b")), div(col("a"), big(-7))]
B_KEY = div(col("a"), big(7))


def error_table(n, at, kind):
    """a BIGINT / BIGINT table of n rows whose only trapping row is row `at`: a zero divisor ("zero") or INT64_MIN / -1 ("min")"""
    a = [(-1) ** i * (3 * i + 5) for i in range(n)]
    b = [(-1) ** (i // 2) * (i % 7 + 2) for i in range(n)]
    a[at], b[at] = (5, 0) if kind == "zero" else (I64_MIN, -1)
    return P.Table("t", _keys(n, 43) + [_column("a", BIGINT, a), _column("b", BIGINT, b)], n)


ERROR_N = [1, 127, 128, 129, ROWS]
ERROR_AT = [0, 127, 128, -1]
ERR_DIV = div(col("a"), col("b"))
ERR_GUARD = cmp("neq", col("b"), big(0))
ERR_GUARD_MIN = cmp("neq", col("b"), big(-1))
ERR_UNGUARDED = ("and", ERR_GUARD, cmp("gt", ERR_DIV, big(1)))       # AND has no short circuit: this one does fail


def error_cases():
    """(n, row, kind) of every error table: the trapping row first, at both sides of the tile seam, last"""
    out = []
    for n in ERROR_N:
        for at in ERROR_AT:
            r = n - 1 if at < 0 else at
            if r < n and (n, r) not in [(x[0], x[1]) for x in out]:
                out += [(n, r, kind) for kind in (("zero", "min") if n == ROWS else ("zero",))]
    return out


# family C: casts
DEC18_8, DEC18_9 = T.DECIMAL(18, 8), T.DECIMAL(18, 9)
INT_CELLS = [I32_MIN, -65537, -65536, -32769, -32768, -1, 0, 32767, 32768, 65535, 65536, I32_MAX]
DOWN_CELLS = sorted({s * (b + d) for b in (0, 100, 200, 10 ** 8, 2 * 10 ** 8, 10 ** 17) for d in (-1, 0, 1) for s in (1, -1)}
                    | {s * v for v in (9, 10, 11, 99, 101, 99999999, 100000001, 5 * 10 ** 7) for s in (1, -1)})


def table_c(n=ROWS):
    cols = _keys(n, 44)
    cols.append(_column("w", DEC18, place(n, (I64_MIN, I64_MAX), CELLS64, 1, 0, 1)))
    cols.append(_column("x", DEC18_8, place(n, (-(10 ** 18 - 1), 10 ** 18 - 1), DOWN_CELLS, 1, 0, 2)))
    cols.append(_column("x9", DEC18_9, place(n, (-(10 ** 18 - 1), 10 ** 18 - 1), DOWN_CELLS, 3, 1, 2)))
    cols.append(_column("a", BIGINT, place(n, (I64_MIN, I64_MAX), CELLS64, 5, 2, 4)))
    cols.append(_column("i", INTT, place(n, (I32_MIN, I32_MAX), INT_CELLS, 1, 0, 1)))
    cols.append(_column("j", INTT, place(n, (I32_MIN, I32_MAX), INT_CELLS, 5, 3, 2)))
    return P.Table("t", cols, n)


C_EXPRS = ([cast(T.DECIMAL(19, 2 + d), col("w")) for d in (1, 2, 8)] + [cast(T.DECIMAL(18, 8 - d), col("x")) for d in (1, 2, 8)]
           + [cast(BIGINT, col("x")), cast(BIGINT, col("w")), cast(T.DECIMAL(12, 2), col("a")),
              add(cast(T.DECIMAL(12, 2), col("a")), col("w")),
              add(col("x"), col("w")),                                                # the implicit cast up by 6, wrapping
              add(cast(T.DECIMAL(18, 0), col("x")), col("w"))])                       # an explicit cast beside a larger scale is retargeted
C_INT = [cast(BIGINT, col("i")), add(col("i"), col("a")), mul(col("j"), big(65536)), sub(cast(BIGINT, col("i")), cast(BIGINT, col("j")))]
C_AGG = [cast(T.DECIMAL(19, 10), col("w")), cast(T.DECIMAL(18, 6), col("x")), cast(BIGINT, col("i"))]
C_KEY = cast(T.DECIMAL(18, 0), col("x"))                                           # -0.99999999 .. 0.99999999 are one group
C_REFUSED = [                                                                     # (expression, is a predicate, the engine's message)
    (cast(T.DECIMAL(18, 0), col("x9")), False, "typecast beyond the supported scale difference"),
    (add(col("i"), col("j")), False, "ADD code generation not implemented for datatype"),
    (cmp("lt", col("i"), col("j")), True, "LESS_THAN code generation not implemented for datatype"),
    (div(col("w"), col("w")), False, "Decimal division not yet implemented"),
]


# family D: comparisons
DEC15_2, DEC15_4, DEC18_6 = T.DECIMAL(15, 2), T.DECIMAL(15, 4), T.DECIMAL(18, 6)
DATE_CELLS = [0, 19920101, 19981201, 99991231, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]
D15 = 10 ** 15 - 1
# c2 x 10^4 wraps from 922 337 203 685 478 on: both sides of that, and values whose images are equal after the rescaling
CELLS_D2 = sorted({s * v for v in (0, 1, 99, 100, 101, 12345, 922337203685477, 922337203685478, D15 - 1, D15) for s in (1, -1)})
CELLS_D4 = sorted({s * v for v in (0, 1, 99, 100, 101, 9900, 10000, 10100, 1234500, D15) for s in (1, -1)})
CELLS_D6 = sorted({s * v for v in (0, 1, 990000, 1000000, 1010000, 123450000, 10 ** 18 - 1, 776627963145224192) for s in (1, -1)})


def table_d(n=ROWS):
    cols = _keys(n, 45)
    cols.append(_column("c2", DEC15_2, place(n, (-D15, D15), CELLS_D2, 1, 0, 1)))
    cols.append(_column("c4", DEC15_4, place(n, (-D15, D15), CELLS_D4, 3, 1, 2)))
    cols.append(_column("c6", DEC18_6, place(n, (-(10 ** 18 - 1), 10 ** 18 - 1), CELLS_D6, 5, 2, 2)))
    cols.append(_column("a", BIGINT, place(n, (I64_MIN, I64_MAX), sorted(set(INT_CELLS) | {I32_MIN - 1, I32_MAX + 1, 1 << 32}), 1, 0, 1)))
    cols.append(_column("i", INTT, place(n, (I32_MIN, I32_MAX), INT_CELLS, 5, 0, 2)))
    cols.append(_column("d", DATE, place(n, (0x80000000, 0x7FFFFFFF), DATE_CELLS, 1, 0, 1)))
    cols.append(_column("e", DATE, place(n, (0x80000000, 0x7FFFFFFF), DATE_CELLS, 3, 1, 2)))
    return P.Table("t", cols, n)


D_PAIRS = {"c2_c4": (col("c2"), col("c4")), "c2_c6": (col("c2"), col("c6")), "a_i": (col("a"), col("i")), "c2_const": (col("c2"), big(1)),
           "d_const": (col("d"), date("1998-12-01")), "d_e": (col("d"), col("e"))}
D_MORE = [cmp("lt", col("d"), date("9999-12-31")),
          ("and", cmp("ge", col("d"), date("1992-01-01")), cmp("le", col("d"), date("1998-12-01"))),
          ("or", cmp("lt", col("c2"), col("c6")), cmp("gt", col("a"), col("i")))]
D_COMPARISONS = [cmp(op, l, r) for (l, r) in D_PAIRS.values() for op in COMPARE] + D_MORE
D_AGG = [flag(D_COMPARISONS[0]), flag(D_COMPARISONS[8]), flag(D_COMPARISONS[33])]
D_KEY = flag(cmp("le", col("c2"), col("c6")))


# family E: CASE
DEC12_2 = T.DECIMAL(12, 2)


def table_e(n=ROWS):
    cols = _keys(n, 46)
    cells = sorted({s * v for v in (0, 1, 50, 99, 100, 101, 199, 250, 10 ** 11, 10 ** 12 - 1) for s in (1, -1)})
    cols.append(_column("p", DEC12_2, place(n, (-(10 ** 12 - 1), 10 ** 12 - 1), cells, 1, 0, 1)))
    cols.append(_column("q", BIGINT, place(n, (I64_MIN, I64_MAX), CELLS64, 3, 1, 2)))
    cols.append(_column("s", BIGINT, place(n, (-2, 2), [-2, -1, 0, 1, 2], 1, 0, 4)))
    return P.Table("t", cols, n)


_pos, _neg, _big = cmp("gt", col("s"), big(0)), cmp("lt", col("s"), big(0)), cmp("gt", col("q"), big(1000))
E_EXPRS = [
    case([(_pos, col("p"))], col("q")),                          # THEN DECIMAL(12,2) / ELSE BIGINT: BIGINT, the THEN value cast down
    case([(_pos, col("q"))], col("p")),                          # the reverse: DECIMAL(12,2), the THEN value cast by 1
    case([(_pos, col("p"))]), case([(_neg, col("q"))]),          # no ELSE: 0
    case([(_pos, big(1)), (cmp("ge", col("s"), big(0)), big(2)), (cmp("ge", col("s"), big(-1)), big(3))], big(4)),      # two or three are true
    case([(_pos, case([(_big, col("q"))], big(-1)))], case([(_neg, big(-2))])),                                      # a CASE inside a CASE
    case([(_pos, col("p"))], dec("0.001")),                      # DECIMAL(12,2) / DECIMAL(4,3): the super type's scale, both cast through (19,0)
    add(case([(_pos, col("q"))], big(0)), col("p")),
]
E_PREDICATES = [cmp("gt", case([(_pos, col("p"))], col("q")), big(0)), cmp("eq", case([(_neg, col("q"))]), big(0))]
# (below an aggregate the types are derived twice, the aggregation's pass and the projection's, and a CASE whose branches were cast by
# the first pass gets another type from the second - in the reference as well: the model follows branches of ONE type, the mixed ones
# are the oracle's and the reference's to judge)
E_AGG = [case([(_pos, col("q"))], col("s")), case([(_neg, col("p"))]), case([(_big, col("p")), (_neg, col("p"))])]
E_AGG_MIXED = [case([(_pos, col("p"))], col("q")), case([(_pos, col("q"))], col("p"))]
E_KEY = case([(_pos, col("q"))], mul(col("s"), big(0)))


FAMILIES = {
    "A": dict(table=table_a, projections=[A_EXPRS, A_CONST], predicates=[], agg=A_AGG, key=A_KEY),
    "B": dict(table=table_b, projections=[B_EXPRS], predicates=B_PREDICATES, agg=B_AGG, key=B_KEY),
    "C": dict(table=table_c, projections=[C_EXPRS, C_INT], predicates=[], agg=C_AGG, key=C_KEY),
    "D": dict(table=table_d, projections=[[flag(c) for c in D_COMPARISONS[i:i + 14]] for i in range(0, len(D_COMPARISONS), 14)],
              predicates=D_COMPARISONS, agg=D_AGG, key=D_KEY),
    "E": dict(table=table_e, projections=[E_EXPRS], predicates=E_PREDICATES, agg=E_AGG, key=E_KEY),
}


# ---- family F: the typed forms of the register aggregation -----------------------------------------------------------------------
def _env(bits, signed):
    m = (1 << bits) - 1
    return (-m if signed else 0, m)


class Form:
    """one row of the issue's table: operand columns with their (lo, hi) and types, the expression, the text the source must hold,
    the class one too narrow (`narrow`), and texts the source must not hold"""
    def __init__(self, id_, cols, expr, text, narrow=None, absent=()):
        self.id, self.cols, self.expr, self.text, self.narrow, self.absent = id_, cols, expr, text, narrow, absent


def _cd(c, d, tc=DEC15_2, td=DEC15_2):
    return [("c", tc, c), ("d", td, d)]


_MUL, _ADD, _SUB = mul(col("c"), col("d")), add(col("c"), col("d")), sub(col("c"), col("d"))
UMUL24, MUL24 = "((i32)__umul24((u32)(n_1), (u32)(n_2)))", "__mul24(n_1, n_2)"
UWIDE, SWIDE = "((i64)((u64)(u32)(n_1) * (u64)(u32)(n_2)))", "((i64)(n_1) * (i64)(n_2))"
FORMS = [
    Form("umul24_24x7", _cd(_env(24, 0), _env(7, 0)), _MUL, UMUL24, "mask23"),
    Form("plain_25x6", _cd(_env(25, 0), _env(6, 0)), _MUL, "((i64)((n_1 * n_2)))", "mask24u", absent=("__umul24",)),
    Form("uwide_16x16", _cd(_env(16, 0), _env(16, 0)), _MUL, UWIDE, "s32"),
    Form("uwide_31x31", _cd(_env(31, 0), _env(31, 0)), _MUL, UWIDE, "s32"),
    Form("mul24_23x7", _cd(_env(23, 1), _env(7, 1)), _MUL, MUL24, "mask22"),
    Form("mul24_23x8", _cd(_env(23, 1), _env(8, 1)), _MUL, MUL24, "mask22"),
    Form("plain_24x7_signed", _cd(_env(24, 1), _env(7, 1)), _MUL, "((i64)((n_1 * n_2)))", "mask23s", absent=("__mul24",)),
    Form("swide_23x9", _cd(_env(23, 1), _env(9, 1)), _MUL, SWIDE, "s32"),
    Form("swide_31x31", _cd(_env(31, 1), _env(31, 1)), _MUL, SWIDE, "s32"),
    Form("add32_30p30", _cd(_env(30, 0), _env(30, 0)), _ADD, "((i64)((n_1 + n_2)))"),
    Form("addwide_31p31", _cd(_env(31, 0), _env(31, 0)), _ADD, "((i64)(n_1) + (i64)(n_2))", "s32"),
    Form("sub32_31m31", _cd(_env(31, 0), _env(31, 0)), _SUB, "((i64)((n_1 - n_2)))"),
    Form("subwide_31m31_signed", _cd(_env(31, 1), _env(31, 1)), _SUB, "((i64)(n_1) - (i64)(n_2))", "s32"),
    Form("cast32_24", _cd(_env(24, 0), _env(7, 0), td=DEC15_4), _ADD, "((i32)__umul24((u32)(n_1), (u32)(((i32)100))))", "mask23"),
    Form("castwide_25", _cd(_env(25, 0), _env(7, 0), td=DEC15_4), _ADD, "((i64)((u64)(u32)(n_1) * (u64)(u32)(((i32)100))))", "s32"),
    # (20 bits x 100 is far from any class boundary: the case is about the BIGINT -> DECIMAL cast being typed at all)
    Form("bigint_cast_20", _cd(_env(20, 0), _env(7, 0), tc=BIGINT), _ADD, "((i32)__umul24((u32)(n_1), (u32)(((i32)100))))"),
    Form("bigint_times_decimal", _cd(_env(23, 1), _env(7, 1), tc=BIGINT), _MUL, MUL24, "mask22"),
    Form("constant_folded", _cd(_env(20, 0), _env(7, 0)), mul(col("c"), sub(dec("1"), dec("0.25"))), "((i32)75)"),
    Form("decode_i32_top", [("c", DEC15_2, (M31 - 200, M31))], col("c"), "rsq::dec<i32>(a.c1[r], a.fb1)"),
    Form("decode_i32_bottom", [("c", DEC15_2, (-M31, -M31 + 200))], col("c"), "rsq::dec<i32>(a.c1[r], a.fb1)"),
    Form("decode_i64_top", [("c", DEC15_2, (M31 - 199, M31 + 1))], col("c"), "rsq::dec<i64>(a.c1[r], a.fb1)", absent=("n_1",)),
    Form("decode_i64_bottom", [("c", DEC15_2, (-M31 - 1, -M31 + 199))], col("c"), "rsq::dec<i64>(a.c1[r], a.fb1)", absent=("n_1",)),
]
FORM = {f.id: f for f in FORMS}
EDGE_ROWS = (list(range(8)), [126, 127, 128, 129, ROWS - 2, ROWS - 1])


def form_table(f, n=ROWS, seed=5):
    """g: three dense groups; the operand columns between their (lo, hi) by narrowcases.edge_values, every pairing of the ends in rows
    0-7 and again in rows 126-129 and the last two"""
    rng = np.random.default_rng(seed)
    cols = [P.Column("g", BIGINT, rng.integers(0, 3, n).astype(np.int64))]
    for j, (name, ty, (lo, hi)) in enumerate(f.cols):
        v = N.edge_values(n, lo, hi - lo, seed=seed + j)
        for i in range(8):
            v[i] = hi if (i >> j) & 1 else lo
        for r, i in enumerate(EDGE_ROWS[1]):
            v[i] = hi if ((r + 1) >> j) & 1 else lo                 # (c, d): hi lo, lo hi, hi hi, lo lo, hi lo, lo hi
        cols.append(_column(name, ty, v))
    return P.Table("t", cols, n)


def form_plan(f, t):
    return aggregation_plan([f.expr], t, sums_only=True)


def form_model(f, t):
    return aggregate_model([f.expr], t, sums_only=True)


def narrower(f, t):
    """per row: (the exact value, the value of an emission one class too narrow) of the case's expression"""
    top = typed(f.expr, schema_of(t))
    n = top
    if f.id in ("cast32_24", "castwide_25"):       # the form under test is the rescaling cast: c x 100
        n = top.kids[0]
        assert n.kind == "cast"
    out = []
    for row in rows_of(t):
        exact = compute(top, row)
        if n.kind == "cast":
            a, b, op = compute(n.kids[0], row), 100, "mul"
        else:
            a, b, op = compute(n.kids[0], row), compute(n.kids[1], row), n.kind
        mask = {"mask23": lambda v: v & ((1 << 23) - 1), "mask24u": lambda v: v & ((1 << 24) - 1),
                "mask22": lambda v: (v + (1 << 22)) % (1 << 23) - (1 << 22), "mask23s": lambda v: (v + (1 << 23)) % (1 << 24) - (1 << 23)}
        if f.narrow == "s32":
            low = wrap32(a * b if op == "mul" else a + b if op == "add" else a - b)
        else:
            low = mask[f.narrow](a) * mask[f.narrow](b)
        if n is not top:
            low = wrap64(low + compute(top.kids[1], row))
        out.append((exact, low))
    return out


# ---- the finishing evaluators ---------------------------------------------------------------------------------------------------
def table_finish(n=ROWS):
    """three groups: 0 is one row; 1 sums to a negative number that its count does not divide; 2's sum x 100 wraps"""
    g = [0] + [1 + (i & 1) for i in range(1, n)]
    a = [7] + [(-1001 if i % 3 else 500) if g[i] == 1 else (1 << 50) + i for i in range(1, n)]
    b = [I64_MAX if i in (1, 2) else 3 * i for i in range(n)]
    d4 = [(-1) ** i * (10 ** 14 + i) for i in range(n)]
    z = [(-1) ** (i // 2) * (10 ** 6 + 7 * i) - 5 for i in range(n)]
    cols = [P.Column("k", BIGINT, np.arange(n, dtype=np.int64)), _column("g", BIGINT, g), _column("a", DEC15_2, a), _column("b", DEC15_2, b),
            _column("d4", DEC15_4, d4), _column("z", BIGINT, z)]
    return P.Table("t", cols, n)


FINISH = {                       # name -> (aggregates as (function, column), the projected expression over them by position or None)
    "sum_plus_sum": ([("sum", "a"), ("sum", "b")], ("add", 0, 1)),
    "sum_minus_sum_scales": ([("sum", "a"), ("sum", "d4")], ("sub", 0, 1)),
    "sum_div_count": ([("sum", "z"), ("count", None)], ("div", 0, 1)),
    "avg": ([("avg", "a"), ("avg", "z"), ("sum", "a"), ("count", None)], None),
}


def finish_plan(name, t, computed_key=False):
    """select g, <expression over the aggregates> | <the aggregates> from t group by g; computed_key: grouped by g + 0 instead, the
    generic hash aggregation"""
    aggs_, e = FINISH[name]
    p = P.Plan([t])
    g = p.add(p.attr("g"), p.constant("0", P.BIGINT)) if computed_key else p.attr("g")
    aggs = [p.count(p.star()) if f == "count" else getattr(p, f)(p.attr(c)) for f, c in aggs_]
    node = p.aggregation(aggs, [g], p.scan(t.name))
    if e is None:
        outs = [p.as_(f"x{i}", a) for i, a in enumerate(aggs)]
    else:
        outs = [p.as_("r", getattr(p, e[0])(aggs[e[1]], aggs[e[2]]))]
    return p.set_root(p.materialize(p.projection([p.as_("gk", g) if computed_key else g] + outs, node)))


def finish_model(name, t):
    """(sorted rows, types): the aggregates over Python integers, then the projected expression through `derive` over their types"""
    aggs_, e = FINISH[name]
    s = schema_of(t)
    groups = {}
    for row in rows_of(t):
        acc = groups.setdefault(row["g"], [0] * len(aggs_) + [0])
        for i, (f, c) in enumerate(aggs_):
            if f != "count":
                acc[i] = wrap64(acc[i] + row[c])
        acc[-1] += 1
    types, rows = [], []
    for f, c in aggs_:
        ct = s[c] if c else None
        types.append(BIGINT if f == "count" else sum_type(ct) if f == "sum" else
                     T.DECIMAL(min(ct.precision + 2, 19), ct.scale + 2) if ct.tag == P.DECIMAL else T.DECIMAL(19, 2))
    for g, acc in sorted(groups.items()):
        vals = [acc[-1] if f == "count" else tdiv(wrap64(acc[i] * 100), acc[-1]) if f == "avg" else acc[i] for i, (f, c) in enumerate(aggs_)]
        if e is None:
            rows.append((g,) + tuple(vals))
        else:
            sch = {f"v{i}": ty for i, ty in enumerate(types)}
            n = typed((e[0], col(f"v{e[1]}"), col(f"v{e[2]}")), sch)
            rows.append((g, compute(n, {f"v{i}": v for i, v in enumerate(vals)})))
            out_types = [n.type]
    return rows, [s["g"]] + (types if e is None else out_types)


# ---- the build's warm-up ------------------------------------------------------------------------------------------------------
FEW = {"RSQ_AGG_MODE": "3"}      # the workgroup's LDS table: what the device tail reads (a register-mode table it does not)


def warm_plans():
    """the plan shapes tests/test_gpu_expr_edges.py compiles, as (plan, environment) pairs (each is compiled with narrow scans and
    without).  Left to their tests: the error tables of 1 and 127-129 rows (other statistics, other texts), the mixed CASE below an
    aggregate and the statement of the context with the compat flag."""
    for fam in FAMILIES.values():
        t = fam["table"]()
        for exprs in fam["projections"]:
            yield projection_plan(exprs, t), {}
        yield aggregation_plan(fam["agg"], t), {}
        yield keyed_plan(fam["key"], t), {}
        for c in fam["predicates"]:
            yield selection_plan(c, t), {}
    t = error_table(ROWS, 0, "zero")
    yield projection_plan([ERR_DIV], t), {}
    yield projection_plan([ERR_DIV], t, where=ERR_GUARD), {}
    yield selection_plan(ERR_UNGUARDED, t), {}
    t = error_table(ROWS, 0, "min")
    yield projection_plan([ERR_DIV], t), {}
    yield projection_plan([ERR_DIV], t, where=ERR_GUARD_MIN), {}
    for f in FORMS:
        yield form_plan(f, form_table(f)), {}
    t = table_finish()
    for name in FINISH:
        yield finish_plan(name, t), {}
    yield finish_plan("avg", t), dict(FEW)
    yield finish_plan("avg", t, computed_key=True), {}
