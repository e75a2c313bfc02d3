"""The register aggregation's second form, rows into per-lane LDS cells, on the GPU (tests/rowcellscases.py): every statement is answered by
a context that runs form 1 wherever a launch fits it (set_row_cells(1)) and by one that generates no second form
(set_row_cells(0)), both byte for byte what the oracle answers and what a Python-integer reference does."""
import os
import sys

import pytest

from oracle import orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import narrowcases as N  # noqa: E402
import ldsfoldcases as L  # noqa: E402
import rowcellscases as R  # noqa: E402

pytestmark = pytest.mark.gpu
CELLS, REGISTERS = "aggregation form of the last execution: 1, rows into LDS cells", "aggregation form of the last execution: 0, registers"


@pytest.fixture(scope="module")
def forms():
    from resql_amd import engine
    always, never = engine.Context(device=0), engine.Context(device=0)
    always.set_row_cells(1)
    never.set_row_cells(0)
    yield always, never
    always.close()
    never.close()


def _run(ctx, plan, table, times=1):
    dt = ctx.table(table)
    q = ctx.compile(plan, [dt])
    try:
        q.await_kernels()                                                 # (a statement may start on the interpreter: the forms are the specialised kernels')
        results = []
        for _ in range(times):
            q.execute()
            results.append(q.result())
        for r in results[1:]:
            assert r.text == results[0].text and r.tuples == results[0].tuples
        return results[0], q.explain
    finally:
        q.close()
        dt.close()


def _check(forms, plan, table, ref, times=1, want=None):
    """both contexts == the oracle, order included, and == the reference; the explain texts of (form 1's context, form 0's)"""
    want = want or orc.execute(plan)
    out = []
    for ctx in forms:
        got, ex = _run(ctx, plan, table, times)
        assert got.text == want.text and got.tuples == want.tuples
        assert sorted(got.rows()) == ref
        out.append(ex)
    assert "RSQ_ROW_CELLS" not in out[1] and "aggregation form" not in out[1]
    return out


def _workgroups(ex, n):
    """the explain text's line about the form names the grid of the last launch"""
    assert f"; {n} workgroups" in ex[ex.index("aggregation form of the last execution"):], ex


@pytest.mark.parametrize("n,max_grid,workgroups", [(n, "1", 1) for n in R.ROWS] + [(n, "4", 2) for n in R.ROWS_TWO_WORKGROUPS])
def test_rows_groups_and_accumulators(forms, monkeypatch, n, max_grid, workgroups):
    """in one workgroup and in two: group 5 in row 0 only, group 0 in the last (tail) row only, group 3 never; three sums in one word, a
    signed sum, min and max beside them"""
    monkeypatch.setenv("RSQ_MAX_GRID", max_grid)
    t = R.packed_table(n)
    ex, _ = _check(forms, N.plan(R.PACKED, [t]), t, N.reference(R.PACKED, t))
    if n >= 6:                                                            # (fewer rows: fewer groups, other statistics, maybe no second form)
        assert "[second form: rows into per-lane LDS cells" in ex and CELLS in ex
        _workgroups(ex, workgroups)


@pytest.mark.parametrize("n,max_grid,workgroups", [(4 * N.TILE + 77, "1", 1), (R.ROWS_TWO_WORKGROUPS[1], "4", 2)])
def test_every_row_in_one_group_and_the_image_is_refilled(forms, monkeypatch, n, max_grid, workgroups):
    """three executions in a row give one relation: no cell keeps what the execution before left in it"""
    monkeypatch.setenv("RSQ_MAX_GRID", max_grid)
    t = R.one_group_table(n)
    ex, _ = _check(forms, N.plan(R.PACKED, [t]), t, R.one_group_reference(n), times=3)
    assert CELLS in ex
    _workgroups(ex, workgroups)
    if workgroups == 2:                                                   # (min and max beside two sums that share no word)
        t = L.minmax_table(L.MINMAX_N)
        ex, _ = _check(forms, N.plan(L.MINMAX, [t]), t, N.reference(L.MINMAX, t), times=3)
        assert CELLS in ex
        _workgroups(ex, 2)


@pytest.mark.parametrize("n,max_grid,inside", [(R.EDGE_INSIDE, "1", True), (R.EDGE_PAST, "1", False), (R.EDGE_INSIDE_TWO, "4", True), (R.EDGE_PAST_TWO, "4", False)])
def test_fields_at_their_edge(forms, monkeypatch, n, max_grid, inside):
    """an 8-bit column at 255 in every row of one group, in one workgroup and in two: just inside the 21-bit bound the word's other
    fields are exact; one tile more and the launch runs form 0"""
    monkeypatch.setenv("RSQ_MAX_GRID", max_grid)
    t = R.one_group_table(n)
    ex, _ = _check(forms, N.plan(R.PACKED, [t]), t, R.one_group_reference(n))
    assert (CELLS if inside else REGISTERS) in ex
    _workgroups(ex, 1 if max_grid == "1" else 2)


def test_partial_step_equals_the_full_execution(forms, monkeypatch):
    """(two workgroups: both flush their fields into the partial table)"""
    import torch
    monkeypatch.setenv("RSQ_MAX_GRID", "4")
    t = R.packed_table(R.ROWS_TWO_WORKGROUPS[1])
    plan = N.plan(R.PACKED, [t])
    want = orc.execute(plan)
    for ctx in forms:
        dt = ctx.table(t)
        q = ctx.compile(plan, [dt])
        try:
            q.await_kernels()
            q.execute()
            full = q.result()
            partial = torch.zeros(sum(q.partial_layout()), dtype=torch.int64, device=torch.device("cuda", 0))
            torch.cuda.synchronize()
            q.bind_partial(partial.data_ptr(), partial.numel() * 8)
            for _ in range(2):
                q.execute_partial_async()
                q.finalize()
                got = q.result()
                assert got.text == full.text and got.tuples == full.tuples
            assert full.text == want.text and full.tuples == want.tuples
            if ctx is forms[0]:
                assert CELLS in q.explain
                _workgroups(q.explain, 2)
        finally:
            q.close()
            dt.close()


def test_the_default_context_measures_both_forms_and_decides(gpu_ctx):
    """two executions in registers, two in cells, then one form for good - and the same relation all along"""
    t = R.packed_table(R.ROWS_TWO_WORKGROUPS[1])
    plan = N.plan(R.PACKED, [t])
    want = orc.execute(plan)
    dt = gpu_ctx.table(t)
    q = gpu_ctx.compile(plan, [dt])
    try:
        q.await_kernels()
        seen = []
        for _ in range(6):
            q.execute()
            got = q.result()
            assert got.text == want.text and got.tuples == want.tuples
            ex = q.explain
            seen.append(1 if CELLS in ex else 0 if REGISTERS in ex else None)
        assert seen[:4] == [0, 0, 1, 1] and seen[4] == seen[5] and seen[4] in (0, 1)
        assert "(decided; " in q.explain and "best kernel times" in q.explain
    finally:
        q.close()
        dt.close()


def test_a_mode_set_later_holds_from_the_next_launch_on():
    """a compiled two-form statement obeys the context's mode as it is at the launch: 1, then 0, then 1 again - one relation"""
    from resql_amd import engine
    t = R.packed_table(R.ROWS_TWO_WORKGROUPS[0])
    plan = N.plan(R.PACKED, [t])
    want = orc.execute(plan)
    ctx = engine.Context(device=0)
    try:
        ctx.set_row_cells(1)
        dt = ctx.table(t)
        q = ctx.compile(plan, [dt])
        try:
            q.await_kernels()
            for mode, line in ((1, CELLS), (0, REGISTERS), (1, CELLS)):
                ctx.set_row_cells(mode)
                q.execute()
                got = q.result()
                assert got.text == want.text and got.tuples == want.tuples
                assert line in q.explain
        finally:
            q.close()
            dt.close()
    finally:
        ctx.close()
