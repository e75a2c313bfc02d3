"""Narrow images (frame of reference + byte width) as the code generator sees them, checked without a GPU: which width a column's
statistics give, that the frame's base is a kernel argument and not text, that TPC-H Q1 / Q6 generate one source at SF 0.01 and SF 10,
and that RSQ_NARROW_SCANS=0 gives the source the scans had without images, byte for byte."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from resql_amd import plan as P, tpch

T = P.TypeInit
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx(tmp_path_factory):
    from resql_amd import engine
    c = engine.Context(device=-1, cache_dir=str(tmp_path_factory.mktemp("kcache_narrow")))
    yield c
    c.close()


def _plan(t):
    """select b, sum(c), count(*) from t where a < 2^62 group by b (an INT or DATE column c: sum(a), and c in the selection)"""
    p = P.Plan([t])
    b = p.attr("b")
    tag = t.columns[2].type.tag
    sc, cnt = p.sum(p.attr("a" if tag in (P.DATE, P.INT) else "c")), p.count(p.star())
    plan = p.scan(t.name)
    where = p.lt(p.attr("a"), p.constant(str(1 << 62), P.BIGINT))
    if tag == P.DATE:
        where = p.and_(where, p.le(p.attr("c"), p.constant("1998-09-02", P.DATE)))
    elif tag == P.INT:
        where = p.and_(where, p.lt(p.attr("c"), p.constant("1000000", P.BIGINT)))
    plan = p.selection(where, plan)
    plan = p.aggregation([sc, cnt], [b], plan)
    plan = p.projection([b, p.as_("s", sc), p.as_("n", cnt)], plan)
    return p.set_root(p.materialize(plan))


def _table(c_type, c_values, n=4096):
    rng = np.random.default_rng(5)
    vals = np.resize(np.asarray(c_values), n)
    return P.Table("t", [P.Column("a", T.BIGINT(), rng.integers(0, 1000, n).astype(np.int64)),
                         P.Column("b", T.BIGINT(), rng.integers(0, 4, n).astype(np.int64)),
                         P.Column("c", c_type, vals.astype(np.int32 if c_type.tag in (P.INT, P.DATE) else np.int64))], n)


def _source(ctx, plan):
    q = ctx.compile(plan, [ctx.table(t) for t in plan.tables])
    try:
        return q.explain, q.source
    finally:
        q.close()


def _width_of_c(src):
    """the narrow width column c (the scan's third column, c2) is read at; 0 = the wide column"""
    m = re.search(r"const (u8|u16|u32|i64|i32)\* c2;", src)
    assert m, src[:2000]
    return {"u8": 1, "u16": 2, "u32": 4}.get(m.group(1), 0)


@pytest.mark.parametrize("lo,span,want", [
    (0, 255, 1), (0, 256, 2), (7, 65535, 2), (7, 65536, 4), (0, (1 << 32) - 1, 4), (0, 1 << 32, 0),
    (-1000, 200, 1), (-(1 << 40), 65535, 2), (-5, 70000, 4),
])
def test_width_at_the_boundaries(ctx, lo, span, want):
    t = _table(T.BIGINT(), [lo, lo + span, lo + span // 2])
    ex, src = _source(ctx, _plan(t))
    assert _width_of_c(src) == want
    assert ("fb2" in src) == (want != 0)


def test_int64_extremes_stay_wide(ctx):
    i64 = np.iinfo(np.int64)
    for vals in ([i64.min, i64.min + 3], [i64.max - 3, i64.max], [i64.min, i64.max]):
        _, src = _source(ctx, _plan(_table(T.BIGINT(), vals)))
        assert _width_of_c(src) == 0


def test_decimal_date_and_int(ctx):
    _, src = _source(ctx, _plan(_table(T.DECIMAL(12, 2), [100, 10_000_000])))
    assert _width_of_c(src) == 4                                          # 8-byte DECIMAL, range below 2^32
    _, src = _source(ctx, _plan(_table(T.DATE(), [19920102, 19981201])))
    assert _width_of_c(src) == 2                                          # 4-byte DATE, range 61 099
    assert "rsq::dec<i32>(a.c2[r], a.fb2)" in src                         # the tail rows decode as well
    _, src = _source(ctx, _plan(_table(T.INT(), [-100, 100])))
    assert _width_of_c(src) == 1                                          # INT: one byte ...
    _, src = _source(ctx, _plan(_table(T.INT(), [0, 1000])))
    assert _width_of_c(src) == 0                                          # ... or the wide column (keys grow with the table)
    _, src = _source(ctx, _plan(_table(T.DATE(), [19920102, 19920102 + 200])))
    assert _width_of_c(src) == 1


def test_the_base_is_an_argument_not_text(ctx):
    a = _source(ctx, _plan(_table(T.BIGINT(), [987_654_321, 987_654_321 + 40_000])))[1]
    b = _source(ctx, _plan(_table(T.BIGINT(), [123_456_789, 123_456_789 + 50_000])))[1]
    assert "987654321" not in a and "123456789" not in b
    assert "i64 fb2;" in a and a == b                                     # one kernel for every frame of the same width


def test_q1_q6_same_source_at_sf001_and_sf10_statistics(ctx):
    cols = tpch.Q1_COLUMNS
    small = tpch.lineitem_table(0.01, cols)
    large = tpch.lineitem_table(10, cols, n_rows=400_000)                 # the first rows of SF 10: its value ranges
    for make in (tpch.q1_plan, tpch.q6_plan):
        ex_s, src_s = _source(ctx, make(small))
        ex_l, src_l = _source(ctx, make(large))
        assert src_s == src_l
        assert "rsq::ld2n(" in src_s and "B/row stored]" in ex_s
    assert "38 B/row, 11 B/row stored]" in _source(ctx, tpch.q1_plan(small))[0]
    assert "28 B/row, 8 B/row stored]" in _source(ctx, tpch.q6_plan(small))[0]


_KILL = r"""
import sys
sys.path.insert(0, sys.argv[1])
from resql_amd import engine, tpch
ctx = engine.Context(device=-1, cache_dir=sys.argv[2])
li = tpch.lineitem_table(0.01, tpch.Q1_COLUMNS + ["l_orderkey"])
cu, od = tpch.customer_table(0.01), tpch.orders_table(0.01)
for plan in (tpch.q1_plan(li), tpch.q6_plan(li), tpch.q3_plan(cu, od, li)):
    q = ctx.compile(plan, [ctx.table(t) for t in plan.tables])
    sys.stdout.write(q.source + "\n=====\n")
    q.close()
ctx.close()
"""


def test_the_kill_switch_gives_the_wide_scans(tmp_path):
    def run(sw):
        env = dict(os.environ, RSQ_NARROW_SCANS=sw)
        return subprocess.run([sys.executable, "-c", _KILL, ROOT, str(tmp_path / ("kc" + sw))], env=env, check=True,
                              capture_output=True, text=True).stdout
    off, on = run("0"), run("1")
    # byte for byte the sources the engine generated before narrow images existed (tests/golden/wide_scan_sources: TPC-H Q1, Q6, Q3
    # at SF 0.01, recorded from the code generator without them)
    gold = os.path.join(ROOT, "tests", "golden", "wide_scan_sources")
    want = "".join(open(os.path.join(gold, n + ".txt")).read() + "\n=====\n" for n in ("q1", "q6", "q3"))
    assert off == want
    assert "ld2n" in on and "32-bit partial sums" in on and off != on
