"""The register aggregation's typed arithmetic, 32-bit first-row tracker and software-pipelined loop on the GPU (tests/typedcases.py).
Every statement is answered by the narrow scan (the default), by the wide scan (RSQ_NARROW_SCANS=0) and by the oracle, byte for byte,
and by typedcases' Python-integer reference; every compiled statement is executed twice."""
import os
import re
import sys

import pytest

from oracle import orc
from resql_amd import plan as P

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import narrowcases as N  # noqa: E402
import typedcases as X  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(ctx, plan, tabs):
    q = ctx.compile(plan, tabs)
    try:
        q.execute()
        first = q.result()
        q.execute()
        again = q.result()
        assert first.text == again.text and first.tuples == again.tuples
        return first, q.source
    finally:
        q.close()


def _check(ctx, monkeypatch, plan, tabs, ref):
    """narrow == oracle and narrow == wide, order included; narrow == the Python-integer reference; returns the narrow run's source"""
    want = orc.execute(plan)
    got, src = _run(ctx, plan, tabs)
    monkeypatch.setenv("RSQ_NARROW_SCANS", "0")
    wide, wide_src = _run(ctx, plan, tabs)
    monkeypatch.delenv("RSQ_NARROW_SCANS")
    assert "ld2n" not in wide_src and "i32 n_" not in wide_src and "fr_0" not in wide_src
    assert got.text == want.text and got.tuples == want.tuples
    assert got.text == wide.text and got.tuples == wide.tuples
    assert sorted(got.rows()) == ref
    return src


# ---- products at the ends of their envelopes, inside the classes and one bit past each boundary ------------------------------------
@pytest.mark.parametrize("negative", [False, True], ids=["nonneg", "neg"])
@pytest.mark.parametrize("cid,c_bits,d_bits,e_bits", X.PRODUCT_CASES, ids=[c[0] for c in X.PRODUCT_CASES])
def test_products_at_the_ends_of_their_envelopes(gpu_ctx, monkeypatch, cid, c_bits, d_bits, e_bits, negative):
    t = X.product_table(c_bits, d_bits, e_bits, negative)
    dt = gpu_ctx.table(t)
    try:
        for exprs in X.STATEMENTS.values():
            src = _check(gpu_ctx, monkeypatch, X.plan(exprs, t), [dt], X.reference(exprs, t))
            assert ", i32 n_1, i32 n_2" in src and "u32 fr_0 = 0xffffffffu;" in src
            if cid == "24x7x7" and not negative:
                assert "rsq::mul(" not in src and "(n_1 * (((i32)100) - n_2))" in src      # the first product in 32 bits
            else:
                assert "(i64)(n_1) * (i64)((((i32)100) - n_2))" in src or cid == "24x7x8"  # ... widened where it may not fit
    finally:
        dt.close()


# ---- first rows -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row0", [0, (1 << 33) + 5])
@pytest.mark.parametrize("n", X.FIRST_ROW_N)
def test_first_rows_decide_the_order(gpu_ctx, monkeypatch, n, row0):
    """one workgroup (RSQ_MAX_GRID=1); group 5 is seen in row 0 only, group 0 in the last row only, group 3 never"""
    monkeypatch.setenv("RSQ_MAX_GRID", "1")
    t = X.first_row_table(n)
    dt = gpu_ctx.table(t)
    try:
        if row0:
            dt.set_row0(row0)
        src = _check(gpu_ctx, monkeypatch, X.plan(X.FIRST_ROWS, t), [dt], X.reference(X.FIRST_ROWS, t))
    finally:
        dt.close()
    assert "u32 fr_5 = 0xffffffffu;" in src and "a.row0 + (i64)st.fr_5" in src and "if (gid == 5) {" in src


# ---- the pipelined loop's edges ---------------------------------------------------------------------------------------------------
def _loop_shape(ctx):
    """(waves of a launch under RSQ_MAX_GRID=1, tiles in flight per wave) of the grouped sum-and-count kernel, read from its source"""
    t = N.fold_table(4 * N.TILE + 77, "alt", 3)
    dt = ctx.table(t)
    try:
        q = ctx.compile(N.plan(N.FOLD_GROUPED, [t]), [dt])
        src = q.source
        q.close()
    finally:
        dt.close()
    assert "const i64 nt = tt0 + nwaves" in src                           # the software-pipelined loop, its prefetch clamped
    assert "(nt < tend ? nt : tend - 1)" in src
    return N.waves_per_launch(src, 1), int(re.search(r"t \+= nwaves \* tstep \* (\d+)\)", src).group(1))


@pytest.mark.parametrize("r", [0, 1, 77])
@pytest.mark.parametrize("step", ["0", "1", "U", "U+1", "2U", "2U+1"])
def test_pipelined_loop_at_its_edges(gpu_ctx, monkeypatch, step, r):
    """waves x T x 128 + r rows under RSQ_MAX_GRID=1: every wave owns exactly T tiles - none, one, one round of the loop, one round and
    a tile (the second round's other tiles are the clamped prefetch only), two rounds, two and a tile"""
    monkeypatch.setenv("RSQ_MAX_GRID", "1")
    waves, U = _loop_shape(gpu_ctx)
    tiles = {"0": 0, "1": 1, "U": U, "U+1": U + 1, "2U": 2 * U, "2U+1": 2 * U + 1}[step]
    n = waves * tiles * N.TILE + r
    t = N.fold_table(n, "alt", 3)
    dt = gpu_ctx.table(t)
    try:
        src = _check(gpu_ctx, monkeypatch, N.plan(N.FOLD_GROUPED, [t]), [dt], N.fold_reference(N.FOLD_GROUPED, n, "alt", 3))
    finally:
        dt.close()
    assert "if (++st.fold_n == 32) { st.fold_n = 0;" in src
    if n >= 6:                                                            # (fewer rows hold fewer than the three groups; none: no statistics)
        assert "i32 p32_1_2 = 0;" in src and "const i64 nt = tt0 + nwaves" in src
