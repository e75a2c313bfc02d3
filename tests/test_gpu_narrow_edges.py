"""Narrow-image decode and 32-bit partial sums on the GPU at the edges of their value ranges (tests/narrowcases.py).  Every case is
answered three times over - by the narrow scan (the default), by the wide scan (RSQ_NARROW_SCANS=0) and by the oracle - and once more
by narrowcases' Python-integer reference; all four are equal byte for byte / tuple for tuple, and the source shows that the case ran
at the width it is meant for.  The fold of the partial sums is reached through RSQ_MAX_GRID=1: one workgroup, so a wave owns dozens
of tiles of a table of 10^5 rows."""
import os
import sys

import pytest

from oracle import orc
from resql_amd import plan as P, tpch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import narrowcases as N  # noqa: E402

pytestmark = pytest.mark.gpu
T = P.TypeInit
GRID = N.grid_cases()


def _run(ctx, plan, tabs):
    """two executions of one compiled statement (the second starts from what the first left behind): (result, source, explain)"""
    q = ctx.compile(plan, tabs)
    try:
        q.execute()
        first = q.result()
        q.execute()
        again = q.result()
        assert first.text == again.text and first.tuples == again.tuples
        return first, q.source, q.explain
    finally:
        q.close()


def _check(ctx, monkeypatch, plan, tabs, ref, ordered=True):
    """narrow == oracle, narrow == wide, narrow == the Python-integer reference; returns the narrow run's (source, explain)"""
    want = orc.execute(plan)
    got, src, ex = _run(ctx, plan, tabs)
    monkeypatch.setenv("RSQ_NARROW_SCANS", "0")
    wide, wide_src, _ = _run(ctx, plan, tabs)
    monkeypatch.delenv("RSQ_NARROW_SCANS")
    assert "ld2n" not in wide_src and "p32_" not in wide_src
    if ordered:
        assert got.text == want.text and got.tuples == want.tuples
        assert got.text == wide.text and got.tuples == wide.tuples
    else:                                                                 # (a materialised join: rows in any order)
        assert sorted(got.text.splitlines()) == sorted(want.text.splitlines()) and got.n_rows == want.n_rows
        assert sorted(got.text.splitlines()) == sorted(wide.text.splitlines())
    assert sorted(got.rows()) == ref
    return src, ex


def _edge_case(ctx, monkeypatch, c_type, n, lo, span, with_sum=True, pool=None, width=True):
    t = N.edge_table(c_type, n, lo, span, pool=pool)
    dt = ctx.table(t)
    try:
        for st in N.edge_statements(c_type, lo, span, with_sum).values():
            src, _ = _check(ctx, monkeypatch, N.plan(st, [t]), [dt], N.reference(st, t))
            if width:
                assert N.scanned_type(src, st, t, "c") == N.width_type(span)
    finally:
        dt.close()


# ---- decode edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,c_type,lo,span,with_sum", GRID, ids=[c[0] for c in GRID])
def test_decode_at_the_ends_of_the_range(gpu_ctx, monkeypatch, cid, c_type, lo, span, with_sum):
    _edge_case(gpu_ctx, monkeypatch, c_type, N.EDGE_N, lo, span, with_sum)


@pytest.mark.parametrize("cid,c_type,lo,span,pool", N.TYPED_CASES, ids=[c[0] for c in N.TYPED_CASES])
def test_decode_of_date_and_int_columns(gpu_ctx, monkeypatch, cid, c_type, lo, span, pool):
    _edge_case(gpu_ctx, monkeypatch, c_type, N.EDGE_N, lo, span, pool=pool)


@pytest.mark.parametrize("n", N.SMALL_N)
def test_decode_in_tables_around_one_tile(gpu_ctx, monkeypatch, n):
    """1, 2 and 127 rows: tail rows only (rsq::dec on the image's own type); 128: one tile and no tail; 129, 257: both"""
    for c_type, lo, span in N.SMALL_CASES:
        _edge_case(gpu_ctx, monkeypatch, c_type, n, lo, span, width=False)


# ---- the late-load form ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_grid", [None, "4"])
def test_late_loads_behind_a_narrow_edge_column(gpu_ctx, monkeypatch, max_grid):
    """the leading column's top 300 values of 65 536 pass; under RSQ_MAX_GRID=4 (16 waves, 2 343 tiles) the pipelined loop goes round
    dozens of times per wave"""
    if max_grid:
        monkeypatch.setenv("RSQ_MAX_GRID", max_grid)
    t = N.late_table()
    st = N.late_statement()
    dt = gpu_ctx.table(t)
    try:
        src, ex = _check(gpu_ctx, monkeypatch, N.plan(st, [t]), [dt], N.reference(st, t))
    finally:
        dt.close()
    assert "late loads" in ex and "lead_pred" in src
    assert N.scanned_type(src, st, t, "c") == "u16" and N.scanned_type(src, st, t, "d") == "u8"
    assert "p32_" in src                                                  # sum(d) and the count fold, in the pipelined loop


def test_late_loads_plain_loop_under_a_small_grid(gpu_ctx, monkeypatch):
    """the same table through the loop that is not software-pipelined (RSQ_LATE_LOADS=0: every column is loaded eagerly), one tile
    after the other in 16 waves"""
    monkeypatch.setenv("RSQ_MAX_GRID", "4")
    monkeypatch.setenv("RSQ_LATE_LOADS", "0")
    t = N.late_table()
    st = N.late_statement()
    dt = gpu_ctx.table(t)
    try:
        src, ex = _check(gpu_ctx, monkeypatch, N.plan(st, [t]), [dt], N.reference(st, t))
    finally:
        dt.close()
    assert "late loads" not in ex and "lead_pred" not in src and "p32_" in src


# ---- a join ---------------------------------------------------------------------------------------------------------------------
def test_join_on_a_narrow_key_with_a_narrow_payload(gpu_ctx, monkeypatch):
    t, r = N.join_tables()
    dr, dt = gpu_ctx.table(r), gpu_ctx.table(t)
    try:
        src, _ = _check(gpu_ctx, monkeypatch, N.join_plan(t, r), [dr, dt], N.join_reference(t, r), ordered=False)
    finally:
        dr.close()
        dt.close()
    build, probe = src.split("// generated by")[1:]                       # (one source per pipeline: r builds, t probes)
    assert N.scan_types(build) == {0: "u32", 1: "u32"}                    # rk (a range of 65 538), rp (2^32 - 1)
    assert N.scan_types(probe)[0] == "u16" and "rsq::ld2n(a.c0 + b, a.fb0" in probe


# ---- the fold of the 32-bit partial sums ----------------------------------------------------------------------------------------
def _fold_case(ctx, monkeypatch, st, tiles, tail, kind, groups):
    monkeypatch.setenv("RSQ_MAX_GRID", "1")
    n = N.FOLD_WAVES * tiles * N.TILE + tail
    t = N.fold_table(n, kind, groups)
    dt = ctx.table(t)
    try:
        src, ex = _check(ctx, monkeypatch, N.plan(st, [t]), [dt], N.fold_reference(st, n, kind, groups))
    finally:
        dt.close()
    assert N.waves_per_launch(src, 1) == N.FOLD_WAVES                     # (what gives every wave exactly `tiles` tiles)
    assert "32-bit partial sums folded every 32 tiles" in ex
    return src


@pytest.mark.parametrize("kind", N.FOLD_KINDS)
@pytest.mark.parametrize("tail", N.FOLD_TAILS)
@pytest.mark.parametrize("tiles", N.FOLD_TILES)
def test_partial_sums_fold_in_time(gpu_ctx, monkeypatch, tiles, tail, kind):
    """every row +-(2^24 - 1): a lane that did not fold after 32 tiles is past 2^31 - 1 at its 65th tile, a fold that kept its partial
    sum counts 32 tiles twice (from 32 tiles on), one that kept its counter folds once only (from 65 on).  One group: the select form
    of the update; three groups by lane: the branchy form, every row of a lane in one group's partial sum."""
    src = _fold_case(gpu_ctx, monkeypatch, N.FOLD, tiles, tail, kind, 1)
    assert "i32 p32_1_0 = 0;" in src and "const bool m = gid == 0;" in src
    src = _fold_case(gpu_ctx, monkeypatch, N.FOLD_GROUPED, tiles, tail, kind, 3)
    assert "i32 p32_1_2 = 0;" in src and "if (gid == 2) {" in src


@pytest.mark.parametrize("tiles", N.FOLD_TILES)
def test_a_column_one_past_the_bound_stays_64_bit_next_to_one_that_folds(gpu_ctx, monkeypatch, tiles):
    src = _fold_case(gpu_ctx, monkeypatch, N.FOLD_MIXED, tiles, 77, "pos", 3)
    assert "i32 p32_1_0 = 0;" in src and "i32 p32_3_0 = 0;" in src        # sum(c) and the count
    assert "p32_2_" not in src and "st.acc_2_0 = rsq::add(st.acc_2_0, in2);" in src      # sum(e), max(e) = 2^24: row by row into the i64


# ---- the knob itself ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_grid", [None, "1"])
def test_max_grid_changes_no_answer(monkeypatch, max_grid):
    from resql_amd import engine
    if max_grid:
        monkeypatch.setenv("RSQ_MAX_GRID", max_grid)
    ctx = engine.Context(device=0)                                        # (its own context: its own plan memo)
    try:
        for plan in (tpch.q1_plan(tpch.lineitem_table(0.01, tpch.Q1_COLUMNS)), tpch.synthetic_plan(tpch.synthetic_table(50_000, 8), 1 << 29)):
            want = orc.execute(plan)
            tabs = [ctx.table(t) for t in plan.tables]
            got, _, _ = _run(ctx, plan, tabs)
            assert got.text == want.text and got.tuples == want.tuples
    finally:
        ctx.close()


def test_statements_compiled_under_different_grids_share_a_context(gpu_ctx, monkeypatch):
    """the plan memo keys on the setting, the code-object cache does not: one context answers the same statement under three settings"""
    t = N.late_table(40_000)
    st = N.late_statement()
    plan, ref = N.plan(st, [t]), N.reference(st, t)
    dt = gpu_ctx.table(t)
    try:
        sources = []
        for g in (None, "1", "3", None):
            if g:
                monkeypatch.setenv("RSQ_MAX_GRID", g)
            else:
                monkeypatch.delenv("RSQ_MAX_GRID", raising=False)
            got, src, _ = _run(gpu_ctx, plan, [dt])
            assert sorted(got.rows()) == ref
            sources.append(src)
        assert len(set(sources)) == 1
    finally:
        dt.close()
