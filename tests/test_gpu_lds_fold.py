"""The register aggregation's 32-bit partial sums folded into the workgroup's LDS image, on the GPU (tests/ldsfoldcases.py): tile
counts per wave from none to past two fold periods in one workgroup and in two, a min and a max next to two partial sums over groups
seen once, never and in the last tail row, 64 cells, tables below one tile, repeated executions and the partial step of a multi-GPU
execution.  Every statement is answered by the narrow scan (the default), by the wide scan (RSQ_NARROW_SCANS=0, no partial sums) and by
the oracle, byte for byte, and by a Python-integer reference; every compiled statement is executed twice."""
import os
import sys

import pytest

from oracle import orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import narrowcases as N  # noqa: E402
import ldsfoldcases as L  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(ctx, plan, tabs, times=2):
    q = ctx.compile(plan, tabs)
    try:
        results = []
        for _ in range(times):
            q.execute()
            results.append(q.result())
        for r in results[1:]:
            assert r.text == results[0].text and r.tuples == results[0].tuples
        return results[0], q.source, q.explain
    finally:
        q.close()


def _check(ctx, monkeypatch, plan, tabs, ref, times=2):
    """narrow == oracle and narrow == wide, order included; narrow == the Python-integer reference; the narrow run's (source, explain)"""
    want = orc.execute(plan)
    got, src, ex = _run(ctx, plan, tabs, times)
    monkeypatch.setenv("RSQ_NARROW_SCANS", "0")
    wide, wide_src, _ = _run(ctx, plan, tabs)
    monkeypatch.delenv("RSQ_NARROW_SCANS")
    assert "p32_" not in wide_src
    assert got.text == want.text and got.tuples == want.tuples
    assert got.text == wide.text and got.tuples == wide.tuples
    assert sorted(got.rows()) == ref
    return src, ex


def _folds(src, ex):
    assert "32-bit partial sums folded every 32 tiles" in ex and "(u64)(i64)st.p32_1_0); st.p32_1_0 = 0;" in src
    assert "if (++st.fold_n == 32) { st.fold_n = 0; rsq::lds_merge<0>(&s_lane[" in src


# ---- tiles per wave around the fold period ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_grid", ["1", "4"])
@pytest.mark.parametrize("tail", L.FOLD_TAILS)
@pytest.mark.parametrize("tiles", L.FOLD_TILES)
def test_folds_into_the_image_in_time(gpu_ctx, monkeypatch, tiles, tail, max_grid):
    """waves x T x 128 + r rows of +-(2^24 - 1): a partial sum that is not folded after 32 tiles is past 2^31 - 1 at the 65th, one that
    is folded and kept counts its tiles twice, one added without its sign is off by 2^32.  RSQ_MAX_GRID=1: one 512-thread workgroup,
    every wave owns T tiles; =4: two workgroups, and both flush (from two tiles a wave on: a smaller table is one workgroup's)."""
    monkeypatch.setenv("RSQ_MAX_GRID", max_grid)
    n = L.fold_rows(max_grid, tiles, tail)
    for kind in L.FOLD_KINDS:
        for st, groups in ((N.FOLD, 1), (N.FOLD_GROUPED, 3)):
            t = N.fold_table(n, kind, groups)
            dt = gpu_ctx.table(t)
            try:
                src, ex = _check(gpu_ctx, monkeypatch, N.plan(st, [t]), [dt], N.fold_reference(st, n, kind, groups))
            finally:
                dt.close()
            assert N.waves_per_launch(src, int(max_grid)) == L.GRID_WAVES[max_grid]
            if n >= 6:                                                    # (fewer rows: fewer groups; none: no statistics, no partial sums)
                _folds(src, ex)
                assert ("if (gid == 2) {" in src) == (groups == 3)


# ---- min and max next to partial sums ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_grid", ["1", None])
def test_min_and_max_keep_their_identities_next_to_the_folds(gpu_ctx, monkeypatch, max_grid):
    """sum(c), count(*), min(c), max(c) by g: group 5 is seen in row 0 only, group 0 in the last tail row only, group 3 never - its
    cells stay the identities the image was filled with before the first fold, through every fold, until the epilogue"""
    if max_grid:
        monkeypatch.setenv("RSQ_MAX_GRID", max_grid)
    t = L.minmax_table(L.MINMAX_N)
    dt = gpu_ctx.table(t)
    try:
        src, ex = _check(gpu_ctx, monkeypatch, N.plan(L.MINMAX, [t]), [dt], N.reference(L.MINMAX, t))
    finally:
        dt.close()
    _folds(src, ex)
    assert "i64 acc_3_5 = (i64)0x7fffffffffffffffull;" in src and "i64 acc_4_5 = (i64)0x8000000000000000ull;" in src
    assert "acc_1_" not in src and "acc_2_" not in src and "u32 fr_5 = 0xffffffffu;" in src


# ---- the register form's cell limit -----------------------------------------------------------------------------------------------
def test_sixty_four_cells(gpu_ctx, monkeypatch):
    monkeypatch.setenv("RSQ_MAX_GRID", "1")
    t = L.cells64_table()
    dt = gpu_ctx.table(t)
    try:
        src, ex = _check(gpu_ctx, monkeypatch, N.plan(L.CELLS64, [t]), [dt], N.reference(L.CELLS64, t))
    finally:
        dt.close()
    _folds(src, ex)
    assert "__shared__ u64 s_lane[4096];" in src and "i32 p32_2_15 = 0;" in src


# ---- tables below one tile --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", L.SMALL_N)
def test_small_tables_pass_through_fill_final_fold_and_epilogue(gpu_ctx, monkeypatch, n):
    for st, t, ref in ((N.FOLD_GROUPED, N.fold_table(n, "neg", 3), N.fold_reference(N.FOLD_GROUPED, n, "neg", 3)),
                       (L.MINMAX, L.minmax_table(n), None)):
        dt = gpu_ctx.table(t)
        try:
            _check(gpu_ctx, monkeypatch, N.plan(st, [t]), [dt], N.reference(st, t) if ref is None else ref)
        finally:
            dt.close()


# ---- no state between launches ----------------------------------------------------------------------------------------------------
def test_three_executions_give_one_relation(gpu_ctx, monkeypatch):
    monkeypatch.setenv("RSQ_MAX_GRID", "4")
    t = L.minmax_table(L.MINMAX_N)
    dt = gpu_ctx.table(t)
    try:
        src, ex = _check(gpu_ctx, monkeypatch, N.plan(L.MINMAX, [t]), [dt], N.reference(L.MINMAX, t), times=3)
    finally:
        dt.close()
    _folds(src, ex)


# ---- the partial step of a multi-GPU execution (the flat flush, RSQ_OUT_STRIDE 1) --------------------------------------------------
@pytest.mark.parametrize("max_grid", ["4", None])
def test_partial_step_equals_the_full_execution(gpu_ctx, monkeypatch, max_grid):
    import torch
    if max_grid:
        monkeypatch.setenv("RSQ_MAX_GRID", max_grid)
    t = L.minmax_table(L.MINMAX_N)
    plan = N.plan(L.MINMAX, [t])
    want = orc.execute(plan)
    dt = gpu_ctx.table(t)
    q = gpu_ctx.compile(plan, [dt])
    try:
        _folds(q.source, q.explain)
        q.execute()
        full = q.result()
        n_min, n_max, n_sum = q.partial_layout()
        assert (n_min, n_max, n_sum) == (12, 6, 12)
        partial = torch.zeros(n_min + n_max + n_sum, dtype=torch.int64, device=torch.device("cuda", 0))
        torch.cuda.synchronize()
        q.bind_partial(partial.data_ptr(), partial.numel() * 8)
        for _ in range(2):                                                # (the second step starts from what the first left behind)
            q.execute_partial_async()
            q.finalize()
            got = q.result()
            assert got.text == full.text and got.tuples == full.tuples
        assert full.text == want.text and full.tuples == want.tuples
    finally:
        q.close()
        dt.close()
