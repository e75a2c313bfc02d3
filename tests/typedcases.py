"""Tables, statements and an exact reference for tests/test_typed_arith_codegen.py and tests/test_gpu_typed_arith.py: the register
aggregation's arithmetic typed by value range (codegen_internal.h ExprGen::emitTyped), its 32-bit first-row tracker and its
software-pipelined loop.  A column's ENVELOPE is its sign class and the bit width of max(|min|, |max|); the tables here put a column's
values at both ends of an envelope, so that a product emitted one bit too narrow wraps.

Expressions are nested tuples - ("col", name), ("const", raw), ("add" | "sub" | "mul", a, b) - read by the plan builder and by the
reference alike.  All columns are DECIMAL(15, 2) and constants are written with two decimals, so no operand is rescaled: raw values
are added, subtracted and multiplied as they stand (the way TPC-H Q1's l_extendedprice * (1 - l_discount) * (1 + l_tax) is).  The
reference computes over Python integers, every operation and every sum wrapped to int64 the way rsq::add / sub / mul wrap."""
import os
import sys

import numpy as np

from resql_amd import plan as P

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import narrowcases as N  # noqa: E402

T = P.TypeInit
DEC = T.DECIMAL(15, 2)
K = 100                                                  # the constant 1.00, raw
ROWS = 4096


def col(name): return ("col", name)
def const(raw): return ("const", raw)
def add(a, b): return ("add", a, b)
def sub(a, b): return ("sub", a, b)
def mul(a, b): return ("mul", a, b)


ONE_PRODUCT = mul(col("c"), sub(const(K), col("d")))                                   # c * (1 - d)
TWO_PRODUCTS = mul(mul(col("c"), sub(const(K), col("d"))), add(const(K), col("e")))    # c * (1 - d) * (1 + e)


def _wrap64(v):
    return (v + (1 << 63)) % (1 << 64) - (1 << 63)


def evaluate(e, row):
    if e[0] == "col":
        return row[e[1]]
    if e[0] == "const":
        return e[1]
    a, b = evaluate(e[1], row), evaluate(e[2], row)
    return _wrap64(a + b if e[0] == "add" else a - b if e[0] == "sub" else a * b)


def envelope(bits, negative):
    """(lo, span) of a column whose values lie at both ends of the envelope of `bits` bits: [0, 2^bits - 1], or [-(2^bits - 1), 2^bits - 1]"""
    m = (1 << bits) - 1
    return (-m, 2 * m) if negative else (0, m)


def _dec(values):
    return np.array([int(v) for v in values], dtype=DEC.np_dtype)


def product_table(c_bits, d_bits, e_bits, negative, n=ROWS, seed=3):
    """g: three groups; c, d, e: N.edge_values over the envelopes - the two ends in rows 0-5, on both sides of the tile boundary at rows
    127 / 128 and in the last two rows.  d and e swap their ends against c's (the seed moves the random rows only), so every pairing
    of extremes meets: rows 0 / 1 hold c's ends, rows 2 / 3 the same swapped."""
    rng = np.random.default_rng(seed)
    cv = N.edge_values(n, *envelope(c_bits, negative), seed=seed)
    dv = N.edge_values(n, *envelope(d_bits, negative), seed=seed + 1)
    ev = N.edge_values(n, *envelope(e_bits, negative), seed=seed + 2)
    # (rows 0-3 of edge_values: lo hi hi lo.  d: lo lo hi hi and e: lo hi lo hi give all eight corners in rows 0-3 and 4-7)
    lo_d, hi_d = envelope(d_bits, negative)[0], sum(envelope(d_bits, negative))
    lo_e, hi_e = envelope(e_bits, negative)[0], sum(envelope(e_bits, negative))
    lo_c, hi_c = envelope(c_bits, negative)[0], sum(envelope(c_bits, negative))
    for i in range(8):
        if i < n:
            cv[i] = hi_c if i & 1 else lo_c
            dv[i] = hi_d if i & 2 else lo_d
            ev[i] = hi_e if i & 4 else lo_e
    return P.Table("t", [P.Column("g", T.BIGINT(), rng.integers(0, 3, n).astype(np.int64)),
                         P.Column("c", DEC, _dec(cv)), P.Column("d", DEC, _dec(dv)), P.Column("e", DEC, _dec(ev))], n)


def expr_node(p, e):
    if e[0] == "col":
        return p.attr(e[1])
    if e[0] == "const":
        s, a = ("-" if e[1] < 0 else ""), abs(e[1])
        return p.constant(f"{s}{a // 100}.{a % 100:02d}", P.DECIMAL)
    return getattr(p, e[0])(expr_node(p, e[1]), expr_node(p, e[2]))


def plan(exprs, t, groups=("g",), count=True):
    """select <groups>, sum(e) for e in exprs [, count(*)] from t group by <groups> (no ORDER BY: the groups' first rows decide the order)"""
    p = P.Plan([t])
    gs = [p.attr(g) for g in groups]
    aggs = [p.sum(expr_node(p, e)) for e in exprs] + ([p.count(p.star())] if count else [])
    node = p.aggregation(aggs, gs, p.scan(t.name))
    node = p.projection(gs + [p.as_(f"x{i}", a) for i, a in enumerate(aggs)], node)
    return p.set_root(p.materialize(node))


def reference(exprs, t, groups=("g",), count=True):
    """the statement's rows as tuples of Python integers, sorted (the emission order is the oracle's to say: it follows from the
    groups' first rows through the reference's hash table)"""
    cols = {c.name: [int(v) for v in c.data] for c in t.columns}
    out = {}
    for r in range(t.n_rows):
        row = {k: v[r] for k, v in cols.items()}
        acc = out.setdefault(tuple(row[g] for g in groups), [0] * (len(exprs) + (1 if count else 0)))
        for i, e in enumerate(exprs):
            acc[i] = _wrap64(acc[i] + evaluate(e, row))
        if count:
            acc[-1] += 1
    return sorted(k + tuple(v) for k, v in out.items())


# (id, c bits, d bits, e bits): inside the classes and one bit past each boundary
PRODUCT_CASES = [("24x7x7", 24, 7, 7), ("25x7x7", 25, 7, 7), ("24x8x7", 24, 8, 7), ("24x7x8", 24, 7, 8)]
STATEMENTS = {"one_product": [ONE_PRODUCT], "two_products": [TWO_PRODUCTS]}


# ---- first rows -------------------------------------------------------------------------------------------------------------------
FIRST_ROW_N = [127, 128, 129, 8 * 3 * 128 + 77]
FIRST_ROWS = [col("c")]


def first_row_table(n, seed=9):
    """six dense groups 0..5: group 5's only row is row 0, group 0's only row is the last row (a tail row unless n is a multiple of
    128), group 3 is absent, 1 / 2 / 4 share the rest with 4 appearing first"""
    rng = np.random.default_rng(seed)
    g = rng.choice(np.array([1, 2, 4], dtype=np.int64), n)
    g[0], g[n - 1] = 5, 0
    if n > 3:
        g[1], g[2] = 4, 2
    c = rng.integers(0, 1 << 20, n)
    return P.Table("t", [P.Column("g", T.BIGINT(), g.astype(np.int64)), P.Column("c", DEC, _dec(c))], n)


# ---- the build's warm-up ----------------------------------------------------------------------------------------------------------
def warm_plans():
    """every plan shape of tests/test_gpu_typed_arith.py as (plan, environment) pairs, for the build's code-object warm-up (each is
    compiled with narrow scans and without)"""
    for _, cb, db, eb in PRODUCT_CASES:
        for negative in (False, True):
            t = product_table(cb, db, eb, negative, n=300)
            for exprs in STATEMENTS.values():
                yield plan(exprs, t), {}
    yield plan(FIRST_ROWS, first_row_table(300)), {}
