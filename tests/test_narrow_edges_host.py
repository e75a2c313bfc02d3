"""tests/narrowcases.py before any kernel runs: its Python-integer reference agrees with the oracle on every case of
tests/test_gpu_narrow_edges.py, the code generator gives 32-bit partial sums exactly where |value| < 2^24 is known (and nowhere
else), every decode case is scanned at the width it is meant to exercise, and RSQ_MAX_GRID changes no kernel text."""
import os
import sys

import numpy as np
import pytest

from oracle import orc
from resql_amd import plan as P

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import narrowcases as N  # noqa: E402

T = P.TypeInit
GRID = N.grid_cases()


@pytest.fixture(scope="module")
def ctx(tmp_path_factory):
    from resql_amd import engine
    c = engine.Context(device=-1, cache_dir=str(tmp_path_factory.mktemp("kcache_narrow_edges")))
    yield c
    c.close()


def _agree(st, t):
    want = orc.execute(N.plan(st, [t]))
    ref = N.reference(st, t)
    assert sorted(want.rows()) == ref
    return ref


def _source(ctx, plan):
    tabs = [ctx.table(t) for t in plan.tables]
    q = ctx.compile(plan, tabs)
    try:
        return q.source, q.explain
    finally:
        q.close()
        for t in tabs:
            t.close()


# ---- the reference against the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,c_type,lo,span,with_sum", GRID, ids=[c[0] for c in GRID])
def test_reference_is_the_oracle_on_the_decode_grid(cid, c_type, lo, span, with_sum):
    t = N.edge_table(c_type, N.EDGE_N, lo, span)
    for st in N.edge_statements(c_type, lo, span, with_sum).values():
        rows = _agree(st, t)
        assert rows                                                       # (both sides of the cut hold rows)


@pytest.mark.parametrize("cid,c_type,lo,span,pool", N.TYPED_CASES, ids=[c[0] for c in N.TYPED_CASES])
def test_reference_is_the_oracle_on_date_and_int(cid, c_type, lo, span, pool):
    t = N.edge_table(c_type, N.EDGE_N, lo, span, pool=pool)
    for st in N.edge_statements(c_type, lo, span).values():
        assert _agree(st, t)


@pytest.mark.parametrize("n", N.SMALL_N)
def test_reference_is_the_oracle_on_the_small_tables(n):
    for c_type, lo, span in N.SMALL_CASES:
        t = N.edge_table(c_type, n, lo, span)
        for st in N.edge_statements(c_type, lo, span).values():
            _agree(st, t)


def test_reference_is_the_oracle_on_the_late_load_and_join_cases():
    assert _agree(N.late_statement(), N.late_table())
    t, r = N.join_tables()
    want = orc.execute(N.join_plan(t, r))
    assert sorted(want.rows()) == N.join_reference(t, r) and want.n_rows > 1000


@pytest.mark.parametrize("kind", N.FOLD_KINDS)
def test_reference_is_the_oracle_on_the_fold_tables(kind):
    """(one size: the statements are sums of a constant, the sizes differ in nothing the reference could get wrong)"""
    n = 8 * 65 * N.TILE + 77
    assert _agree(N.FOLD, N.fold_table(n, kind, 1)) == N.fold_reference(N.FOLD, n, kind, 1)
    rows = _agree(N.FOLD_GROUPED, N.fold_table(n, kind, 3))
    assert rows == N.fold_reference(N.FOLD_GROUPED, n, kind, 3) and len(rows) == 3 and sum(r[2] for r in rows) == n
    assert _agree(N.FOLD_MIXED, N.fold_table(n, kind, 3)) == N.fold_reference(N.FOLD_MIXED, n, kind, 3)


def test_the_sum_without_a_fold_would_not_fit_32_bits():
    """what the fold tests rest on: 65 tiles are 130 rows of a lane, and 130 * (2^24 - 1) is past 2^31 - 1; the 2 * 32 + 1 rows a lane
    meets between two folds are not"""
    assert 130 * N.P32_MAX > (1 << 31) - 1 and 65 * N.P32_MAX <= (1 << 31) - 1


# ---- where the code generator keeps 32-bit partial sums --------------------------------------------------------------------------
@pytest.mark.parametrize("c_min,c_max,want", [
    (0, N.P32_MAX, True), (-N.P32_MAX, 0, True), (0, N.P32_MAX + 1, False), (-N.P32_MAX - 1, 0, False),
])
def test_partial_sums_at_the_bound(ctx, c_min, c_max, want):
    t = N.p32_table(c_min, c_max)
    src, ex = _source(ctx, N.plan(N.P32_PROBE, [t]))
    col = "1_0"                                                           # accumulator 1 (sum(c)), group 0
    assert ("i32 p32_" + col + " = 0;" in src) == want
    assert "i32 p32_2_0 = 0;" in src                                      # the count has one either way
    assert "32-bit partial sums" in ex
    if want:
        assert "st.p32_" + col + " = 0;" in src and "if (++st.fold_n == 32) { st.fold_n = 0;" in src


def test_no_partial_sums_without_narrow_scans(ctx, monkeypatch):
    t = N.p32_table(0, N.P32_MAX)
    assert "p32_" in _source(ctx, N.plan(N.P32_PROBE, [t]))[0]
    monkeypatch.setenv("RSQ_NARROW_SCANS", "0")
    assert "p32_" not in _source(ctx, N.plan(N.P32_PROBE, [t]))[0]


def test_no_partial_sum_for_an_expression(ctx):
    t = N.p32_table(0, 1000)
    p = P.Plan([t])
    s = p.sum(p.mul(p.attr("c"), p.constant("2", P.BIGINT)))
    node = p.aggregation([s], [p.attr("b")], p.scan("t"))
    p.set_root(p.materialize(p.projection([p.attr("b"), p.as_("s", s)], node)))
    assert "p32_" not in _source(ctx, p)[0]


def _join_then_aggregate(t):
    """select b, sum(c), count(*) from r, t where rk = a and a < 30 group by b"""
    r = P.Table("r", [P.Column("rk", T.BIGINT(), np.arange(0, 2000, 2, dtype=np.int64))], 1000)
    p = P.Plan([r, t])
    probe = p.selection(p.lt(p.attr("a"), p.constant("30", P.BIGINT)), p.scan("t"))
    j = p.hashjoin([p.eq(p.attr("rk"), p.attr("a"))], p.scan("r"), probe, single_match=True)
    sc, cn = p.sum(p.attr("c")), p.count(p.star())
    node = p.projection([p.attr("b"), p.as_("s", sc), p.as_("n", cn)], p.aggregation([sc, cn], [p.attr("b")], j))
    return p.set_root(p.materialize(node))


def test_no_partial_sums_behind_a_wave_compaction(ctx, monkeypatch):
    t = N.p32_table(0, N.P32_MAX)
    src, ex = _source(ctx, _join_then_aggregate(t))
    assert "wave compaction" in ex and "in registers" in ex and "p32_" not in src
    monkeypatch.setenv("RSQ_COMPACT", "0")                                # the same plan without the compaction has them
    src, ex = _source(ctx, _join_then_aggregate(t))
    assert "wave compaction" not in ex and "p32_" in src


def test_no_partial_sums_over_a_derived_table(ctx):
    t = N.p32_table(0, N.P32_MAX)
    p = P.Plan([t])
    cnt = p.count(p.star())
    inner = p.aggregation([cnt], [p.attr("a")], p.scan("t"))
    p.set_root(p.materialize(p.aggregation([p.sum(cnt), p.count(p.star())], [], inner)), request_all=True)
    src, ex = _source(ctx, p)
    assert "scan derived0" in ex and "in registers" in ex and "p32_" not in src


# ---- widths and the launch-width knob ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("span", N.SPANS)
def test_decode_cases_are_scanned_at_their_width(ctx, span):
    for c_type, lo in ((T.BIGINT(), -(1 << 62)), (T.DECIMAL(12, 2), (1 << 62) - (1 << 33))):
        t = N.edge_table(c_type, N.EDGE_N, lo, span)
        st = N.edge_statements(c_type, lo, span, False)["below_max"]
        src, _ = _source(ctx, N.plan(st, [t]))
        assert N.scanned_type(src, st, t, "c") == N.width_type(span)


def test_max_grid_leaves_the_kernel_text_alone(ctx, monkeypatch):
    t = N.fold_table(4 * 33 * N.TILE + 77, "pos", 3)
    late = N.late_table(5000)
    plans = [N.plan(N.FOLD_GROUPED, [t]), N.plan(N.late_statement(), [late])]
    before = [_source(ctx, p) for p in plans]
    for g in ("1", "4", "65535", "0", "65536", "-3"):
        monkeypatch.setenv("RSQ_MAX_GRID", g)
        assert [_source(ctx, p) for p in plans] == before, g


def test_the_build_warms_every_plan():
    """__graft_entry__.build() compiles warm_plans() number 0 to 199 into the code-object cache"""
    assert 0 < sum(1 for _ in N.warm_plans()) <= 200
