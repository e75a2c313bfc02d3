"""Tables, statements and an exact reference for tests/test_narrow_edges_host.py and tests/test_gpu_narrow_edges.py: narrow images
(frame of reference, rsq_device.h ld2n / dec) and 32-bit partial sums (codegen_agg.cpp) at the edges of their value ranges - image
values with the top bit set, ranges that end exactly on 255 / 256 / 65535 / 65536 / 2^32 - 1 / 2^32, negative and huge bases, the
column's min and max in both halves of a lane's two-row load, on both sides of a tile boundary and in the tail rows, and sums of
+-(2^24 - 1) over more tiles per wave than the partial sums may hold between two folds.

The reference (`reference`) computes every statement over Python integers, sums wrapped to int64 the way rsq::add wraps; the host
test proves it against the oracle before a kernel is involved."""
import datetime
import re

import numpy as np

from resql_amd import plan as P

T = P.TypeInit

TILE = 128
EDGE_N = TILE * 9 + 50
SMALL_N = [1, 2, 127, 128, 129, 257]
SPANS = [255, 256, 65535, 65536, (1 << 32) - 1, 1 << 32]
SMALL_BASES = [0, -1000, -(1 << 40)]                    # sum(c) of EDGE_N rows stays far inside int64
HUGE_BASES = [(1 << 62) - (1 << 33), -(1 << 62)]        # ... here it would not: these run without the sum
P32_MAX = (1 << 24) - 1                                 # the largest |value| a 32-bit partial sum takes
FOLD_TILES = [31, 32, 33, 64, 65, 80, 200]              # whole tiles per wave: around one fold period, around two, several
FOLD_TAILS = [0, 77]
FOLD_WAVES = 8                                          # waves of a register aggregation's launch under RSQ_MAX_GRID=1: one 512-thread workgroup


def width_type(span):
    """the C type a column whose max - min is `span` is scanned at"""
    return "u8" if span <= 255 else "u16" if span <= 65535 else "u32" if span < (1 << 32) else "i64"


def scan_types(source):
    """kernel argument types of the scanned columns of a generated source, by column number: {2: 'u8', ...}"""
    return {int(k): t for t, k in re.findall(r"const (u8|u16|u32|i32|i64)\* c(\d+);", source)}


def scanned_type(source, st, t, col):
    """the type column `col` of table `t` is scanned at by statement `st` (the scan numbers the columns it reads in table order)"""
    used = {c for _, c in st.aggs if c} | set(st.groups) | {c for c, _, _ in st.where}
    order = [c.name for c in t.columns if c.name in used]
    return scan_types(source)[order.index(col)]


def block_threads(source):
    return int(re.search(r"#define RSQ_BLOCK_THREADS (\d+)", source).group(1))


def waves_per_launch(source, max_grid):
    """waves of a launch under RSQ_MAX_GRID=max_grid: max_grid * 256 threads in workgroups of the kernel's size, at least one workgroup"""
    b = block_threads(source)
    return max(1, max_grid * 256 // b) * (b // 64)


# ---- tables ---------------------------------------------------------------------------------------------------------------------
def _np(type_, values):
    return np.array([int(v) for v in values], dtype=type_.np_dtype)


def edge_values(n, lo, span, seed=11, pool=None):
    """`n` values of [lo, lo + span] as Python integers: rows 0 / 1 hold lo / lo + span (the low and the high half of lane 0's packed
    load), rows 2 / 3 the same swapped, 4 / 5 the values next to the ends, 127 / 128 the two ends on both sides of a tile boundary, the
    last two rows (tail rows unless n is a multiple of 128) the ends again; the others are random, every other one from the top half of
    the range (image values with the top bit set).  `pool`: the values the random rows may take (sorted; DATE columns: real dates)."""
    rng = np.random.default_rng(seed)
    hi, mid = lo + span, lo + (span + 1) // 2
    if pool is None:
        low = [lo + int(x) for x in rng.integers(0, span + 1, n, dtype=np.uint64)]
        top = [mid + int(x) for x in rng.integers(0, hi - mid + 1, n, dtype=np.uint64)]
    else:
        upper = [v for v in pool if v >= mid]
        low = [pool[int(i)] for i in rng.integers(0, len(pool), n)]
        top = [upper[int(i)] for i in rng.integers(0, len(upper), n)]
    vals = [top[i] if i % 2 else low[i] for i in range(n)]
    fixed = {0: lo, 1: hi, 2: hi, 3: lo, 4: lo + 1, 5: hi - 1, 127: hi, 128: lo, 129: hi, 126: lo}
    for i, v in fixed.items():
        if i < n:
            vals[i] = v
    if n >= 2:
        vals[n - 2], vals[n - 1] = lo, hi
    elif n == 1:
        vals[0] = hi
    return vals


def date_pool(first, last):
    """every calendar day from `first` to `last` (yyyymmdd integers, the engine's DATE values)"""
    d = datetime.date(first // 10000, first // 100 % 100, first % 100)
    end = datetime.date(last // 10000, last // 100 % 100, last % 100)
    out = []
    while d <= end:
        out.append(d.year * 10000 + d.month * 100 + d.day)
        d += datetime.timedelta(days=1)
    return out


def edge_table(c_type, n, lo, span, seed=11, pool=None):
    """a: 0..999; b: four groups; c: the column under test (edge_values)"""
    rng = np.random.default_rng(seed + 1)
    return P.Table("t", [P.Column("a", T.BIGINT(), rng.integers(0, 1000, n).astype(np.int64)),
                         P.Column("b", T.BIGINT(), rng.integers(0, 4, n).astype(np.int64)),
                         P.Column("c", c_type, _np(c_type, edge_values(n, lo, span, seed, pool)))], n)


# (id, type, lo, span, random-row pool) of the typed cases next to the BIGINT / DECIMAL grid
DATE_LO = 19920102
TYPED_CASES = [
    ("date_200_days", T.DATE(), DATE_LO, 19920720 - DATE_LO, date_pool(DATE_LO, 19920720)),        # 200 days: 618 as yyyymmdd, two bytes
    ("date_one_byte", T.DATE(), DATE_LO, 200, date_pool(DATE_LO, DATE_LO + 200)),                    # ... and a range of 200: one byte
    ("date_1992_1998", T.DATE(), DATE_LO, 19981201 - DATE_LO, date_pool(DATE_LO, 19981201)),         # the whole TPC-H span: two bytes
    ("int_pm100", T.INT(), -100, 200, None),
    ("int_m128_127", T.INT(), -128, 255, None),
]


def grid_cases():
    """(id, type, lo, span, with_sum) over BIGINT and DECIMAL(12,2), every span at every base"""
    out = []
    for tn, ty in (("bigint", T.BIGINT()), ("decimal", T.DECIMAL(12, 2))):
        for lo in SMALL_BASES + HUGE_BASES:
            for span in SPANS:
                out.append((f"{tn}_lo{lo}_span{span}", ty, lo, span, lo in SMALL_BASES))
    return out


# the small tables (SMALL_N rows): one case per image width
SMALL_CASES = [(T.BIGINT(), -1000, 255), (T.BIGINT(), -(1 << 40), 65535), (T.DECIMAL(12, 2), 0, (1 << 32) - 1)]


def late_table(n=300_000, lo=-(1 << 40), span=65535, seed=21):
    """c: the narrow edge column, leading and selective (the predicate passes its top 300 values); d: a second narrow column, loaded late
    (DECIMAL, one byte, negative base, its ends next to each other in the rows that pass)"""
    t = edge_table(T.BIGINT(), n, lo, span, seed)
    d = edge_values(n, -200, 255, seed + 5)
    t.columns.append(P.Column("d", T.DECIMAL(12, 2), _np(T.DECIMAL(12, 2), d)))
    return t


def join_tables(n=6000, seed=31):
    """t.k: the probe key, a narrow BIGINT with a negative base (two bytes, every edge of edge_values); r: one row per key of the upper
    half of the range and a few outside it, rp a narrow DECIMAL payload (four bytes, negative base)"""
    lo, span = -70_000, 65535
    rng = np.random.default_rng(seed)
    pool = [lo, lo + 1] + list(range(lo + 32768 - 500, lo + 32768 + 3500)) + [lo + span - 1, lo + span]      # (most probes near the build keys)
    t = P.Table("t", [P.Column("k", T.BIGINT(), _np(T.BIGINT(), edge_values(n, lo, span, seed, pool))),
                      P.Column("a", T.BIGINT(), rng.integers(0, 1000, n).astype(np.int64))], n)
    keys = [lo, lo + 1, lo + span - 1, lo + span] + list(range(lo + 32768, lo + 32768 + 3000)) + [lo - 1, lo + span + 1]
    pay = edge_values(len(keys), -(1 << 31), (1 << 32) - 1, seed + 1)
    r = P.Table("r", [P.Column("rk", T.BIGINT(), _np(T.BIGINT(), keys)),
                      P.Column("rp", T.DECIMAL(12, 2), _np(T.DECIMAL(12, 2), pay))], len(keys))
    return t, r


FOLD_KINDS = ["pos", "neg", "alt", "alt_lanes"]


def _fold_sign(n, kind):
    row = np.arange(n, dtype=np.int64)
    return {"pos": np.ones(n, np.int64), "neg": -np.ones(n, np.int64), "alt": 1 - 2 * (row % 2), "alt_lanes": 1 - 2 * ((row // 2) % 2)}[kind]


def fold_reference(st, n, kind, groups):
    """the rows of FOLD / FOLD_GROUPED / FOLD_MIXED over fold_table(n, kind, groups) in closed form: per group a count and a sum of
    signs (small integers), multiplied out as Python integers - the loop of `reference` over 200 000 rows without the loop
    (tests/test_narrow_edges_host.py holds the two against each other)"""
    sign = _fold_sign(n, kind)
    b = (np.arange(n, dtype=np.int64) % TILE) // 2 % groups
    rows = []
    for g in range(groups):
        m = b == g
        if not m.any():
            continue
        cnt, sgn = int(m.sum()), sign[m]
        val = {("sum", "c"): int(sgn.sum()) * P32_MAX, ("sum", "e"): cnt << 24, ("count", None): cnt,
               ("min", "c"): int(sgn.min()) * P32_MAX, ("max", "c"): int(sgn.max()) * P32_MAX}
        rows.append(((g,) if st.groups else ()) + tuple(_wrap64(val[a]) for a in st.aggs))
    return sorted(rows)


def fold_table(n, kind, groups):
    """c: +(2^24 - 1) in every row ('pos'), -(2^24 - 1) ('neg'), the signs alternating with the row ('alt') or every lane's two rows
    alike and the lanes alternating ('alt_lanes': a lane's partial sum only ever grows or only ever falls); e: 2^24 in every row - one
    too many for a partial sum.  b: the group - `groups` = 1: one group; 3: a function of the lane ((row % 128) / 2 % 3), so that one
    group meets every row of its lanes."""
    sign = _fold_sign(n, kind)
    b = (np.arange(n, dtype=np.int64) % TILE) // 2 % groups
    return P.Table("t", [P.Column("b", T.BIGINT(), b.astype(np.int64)),
                         P.Column("c", T.BIGINT(), sign * P32_MAX),
                         P.Column("e", T.BIGINT(), np.full(n, 1 << 24, dtype=np.int64))], n)


def p32_table(c_min, c_max, n=4096, seed=5):
    """a, b, c as edge_table; c between c_min and c_max with both present (what decides whether sum(c) gets a 32-bit partial sum)"""
    rng = np.random.default_rng(seed)
    c = rng.integers(c_min, c_max + 1, n).astype(np.int64)
    c[0], c[1] = c_min, c_max
    return P.Table("t", [P.Column("a", T.BIGINT(), rng.integers(0, 1000, n).astype(np.int64)),
                         P.Column("b", T.BIGINT(), rng.integers(0, 4, n).astype(np.int64)),
                         P.Column("c", T.BIGINT(), c)], n)


# ---- statements: a description the plan builder and the reference both read -------------------------------------------------------
class Statement:
    """select <groups>, <aggs> from t [where <col> <op> <value> [and ...]] [group by <groups>]: aggs are (function, column) pairs with
    function in sum / min / max / count (count: column None), where is a list of (column, op, value) with op in lt / le / ge / gt"""

    def __init__(self, aggs, groups=(), where=()):
        self.aggs, self.groups, self.where = list(aggs), list(groups), list(where)


def constant(p, type_, v):
    """the literal of raw value v next to a column of `type_`.  BIGINT and DECIMAL columns get a DECIMAL literal (a DECIMAL's digits with
    the point put back, a BIGINT's with none: scale 0) because a BIGINT literal is parsed through 32 bits, as the reference parses it;
    INT columns a BIGINT literal, DATE columns y-m-d."""
    if type_.tag in (P.DECIMAL, P.BIGINT):
        scale = type_.scale if type_.tag == P.DECIMAL else 0
        s, a = ("-" if v < 0 else ""), abs(v)
        return p.constant(f"{s}{a // 10 ** scale}.{a % 10 ** scale:0{scale}d}" if scale else f"{s}{a}", P.DECIMAL)
    if type_.tag == P.DATE:
        return p.constant(f"{v // 10000}-{v // 100 % 100:02d}-{v % 100:02d}", P.DATE)
    return p.constant(str(v), P.BIGINT)


def plan(st, tables):
    """the statement over tables[0] as a plan: scan -> selection -> aggregation -> projection -> materialize"""
    t = tables[0]
    p = P.Plan(tables)
    node = p.scan(t.name)
    conds = []
    for col, op, v in st.where:
        conds.append(getattr(p, op)(p.attr(col), constant(p, t.col(col).type, v)))
    if conds:
        node = p.selection(p.conjunction(conds), node)
    groups = [p.attr(g) for g in st.groups]
    # (an INT column is aggregated as BIGINT: the reference has no sum / min / max of INT)
    value = lambda c: p.typecast(T.BIGINT(), p.attr(c)) if t.col(c).type.tag == P.INT else p.attr(c)
    aggs = [p.count(p.star()) if f == "count" else getattr(p, f)(value(c)) for f, c in st.aggs]
    node = p.aggregation(aggs, groups, node)
    node = p.projection(groups + [p.as_(f"x{i}", a) for i, a in enumerate(aggs)], node)
    return p.set_root(p.materialize(node))


def _wrap64(v):
    return (v + (1 << 63)) % (1 << 64) - (1 << 63)


_OPS = {"lt": lambda a, b: a < b, "le": lambda a, b: a <= b, "ge": lambda a, b: a >= b, "gt": lambda a, b: a > b}


def reference(st, t):
    """the statement's rows as tuples of Python integers, sorted (the groups lead every row); no row passes and no groups: no row"""
    cols = {c.name: [int(v) for v in c.data] for c in t.columns if c.data is not None}
    out = {}
    for r in range(t.n_rows):
        if not all(_OPS[op](cols[col][r], v) for col, op, v in st.where):
            continue
        key = tuple(cols[g][r] for g in st.groups)
        acc = out.setdefault(key, [None] * len(st.aggs))
        for i, (f, c) in enumerate(st.aggs):
            v = 1 if f == "count" else cols[c][r]
            if acc[i] is None:
                acc[i] = v
            elif f in ("sum", "count"):
                acc[i] = _wrap64(acc[i] + v)
            else:
                acc[i] = min(acc[i], v) if f == "min" else max(acc[i], v)
    return sorted(k + tuple(v) for k, v in out.items())


def edge_statements(c_type, lo, span, with_sum=True):
    """{name: Statement}: the aggregates of c by b below the column's max (c < lo + span: the predicate cuts between the two largest
    values) and at it (c >= lo + span); a DATE has no sum: a is summed in its place"""
    aggs = [("min", "c"), ("max", "c"), ("count", None)]
    if with_sum:
        aggs = [("sum", "a" if c_type.tag == P.DATE else "c")] + aggs
    return {"below_max": Statement(aggs, ["b"], [("c", "lt", lo + span)]),
            "at_max": Statement(aggs, ["b"], [("c", "ge", lo + span)])}


def late_statement(lo=-(1 << 40), span=65535):
    return Statement([("sum", "c"), ("sum", "d"), ("min", "d"), ("max", "d"), ("count", None)], ["b"], [("c", "ge", lo + span - 299)])


FOLD = Statement([("sum", "c"), ("count", None), ("min", "c"), ("max", "c")])
FOLD_GROUPED = Statement(FOLD.aggs, ["b"])
FOLD_MIXED = Statement([("sum", "c"), ("sum", "e"), ("count", None)], ["b"])
P32_PROBE = Statement([("sum", "c"), ("count", None)], ["b"])


def join_plan(t, r):
    """select k, a, rp from r, t where rk = k and a < 500 (r builds, t probes)"""
    p = P.Plan([r, t])
    probe = p.selection(p.lt(p.attr("a"), p.constant("500", P.BIGINT)), p.scan("t"))
    j = p.hashjoin([p.eq(p.attr("rk"), p.attr("k"))], p.scan("r"), probe, single_match=True)
    return p.set_root(p.materialize(p.projection([p.attr("k"), p.attr("a"), p.attr("rp")], j)))


def join_reference(t, r):
    pay = {int(k): int(v) for k, v in zip(r.col("rk").data, r.col("rp").data)}
    return sorted((int(k), int(a), pay[int(k)]) for k, a in zip(t.col("k").data, t.col("a").data) if a < 500 and int(k) in pay)


def warm_plans():
    """every plan shape of tests/test_gpu_narrow_edges.py as (plan, environment) pairs over small stand-ins of its tables where the text
    does not depend on the size - for the build's code-object warm-up (a compile-only context; each is compiled with narrow scans and
    without)"""
    for cid, c_type, lo, span, with_sum in grid_cases():
        t = edge_table(c_type, EDGE_N, lo, span)
        for st in edge_statements(c_type, lo, span, with_sum).values():
            yield plan(st, [t]), {}
    for cid, c_type, lo, span, pool in TYPED_CASES:
        t = edge_table(c_type, EDGE_N, lo, span, pool=pool)
        for st in edge_statements(c_type, lo, span).values():
            yield plan(st, [t]), {}
    for n in SMALL_N:
        for c_type, lo, span in SMALL_CASES:
            t = edge_table(c_type, n, lo, span)
            for st in edge_statements(c_type, lo, span).values():
                yield plan(st, [t]), {}
    for n in (300_000, 40_000):
        yield plan(late_statement(), [late_table(n)]), {}
    yield plan(late_statement(), [late_table()]), {"RSQ_LATE_LOADS": "0"}
    t, r = join_tables()
    yield join_plan(t, r), {}
    for kind in FOLD_KINDS:
        yield plan(FOLD, [fold_table(4 * TILE + 77, kind, 1)]), {}
        yield plan(FOLD_GROUPED, [fold_table(4 * TILE + 77, kind, 3)]), {}
    yield plan(FOLD_MIXED, [fold_table(4 * TILE + 77, "pos", 3)]), {}
