"""Scalar expressions on the GPU at their value edges (tests/exprcases.py): the generated row functions over rsq::add / sub / mul / div
and the casts, as projections, as predicates, below aggregates (narrow scans, wide scans, a computed group key); every typed form of
the register aggregation's range-typed arithmetic at the ends of its envelope; the finishing evaluators of the host tail and of the
device tail; the division error word.  Every statement is executed twice; every answer is compared exactly - integers with the plain
integer model, text and tuple bytes with the oracle, result types with the model's."""
import os
import sys

import pytest

from oracle import orc
from resql_amd import engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exprcases as X  # noqa: E402

pytestmark = pytest.mark.gpu
FAMILY_IDS = sorted(X.FAMILIES)


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


def _types(res, types):
    assert [str(t) for t in res.types] == [str(t) for t in types]


def _answer(ctx, plan, tabs, rows, types, ordered=True):
    """the statement twice on the device: the model's integers and types, the oracle's text and bytes"""
    want = orc.execute(plan)
    got, src = _run(ctx, plan, tabs)
    _types(got, types)
    assert (got.rows() if ordered else sorted(got.rows())) == rows
    assert got.text == want.text and got.tuples == want.tuples
    return got, src


@pytest.fixture(scope="module")
def family(gpu_ctx):
    """the families' tables, each created once on the device"""
    made = {}

    def get(name):
        if name not in made:
            t = X.FAMILIES[name]["table"]()
            made[name] = (t, gpu_ctx.table(t))
        return made[name]
    yield get
    for _, dt in made.values():
        dt.close()


# ---- projections ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FAMILY_IDS)
def test_projections_row_by_row(gpu_ctx, family, name):
    t, dt = family(name)
    for exprs in X.FAMILIES[name]["projections"]:
        rows, types = X.project_model(exprs, t)
        got, _ = _answer(gpu_ctx, X.projection_plan(exprs, t), [dt], rows, types)
        assert got.n_rows == X.ROWS


# ---- predicates -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in FAMILY_IDS if X.FAMILIES[n]["predicates"]])
def test_predicates_pass_the_models_rows(gpu_ctx, family, name):
    t, dt = family(name)
    passing = set()
    for cond in X.FAMILIES[name]["predicates"]:
        rows, types = X.project_model([], t, where=cond)
        _answer(gpu_ctx, X.selection_plan(cond, t), [dt], rows, types)
        passing.add(len(rows))
    assert len(passing) > 1                                               # (the predicates do select)


# ---- below aggregates -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FAMILY_IDS)
def test_aggregates_narrow_wide_and_by_a_computed_key(gpu_ctx, family, monkeypatch, name):
    t, dt = family(name)
    fam = X.FAMILIES[name]
    plan = X.aggregation_plan(fam["agg"], t)
    rows, types = X.aggregate_model(fam["agg"], t)
    got, _ = _answer(gpu_ctx, plan, [dt], rows, types, ordered=False)
    monkeypatch.setenv("RSQ_NARROW_SCANS", "0")
    wide, wide_src = _answer(gpu_ctx, plan, [dt], rows, types, ordered=False)
    monkeypatch.delenv("RSQ_NARROW_SCANS")
    assert "ld2n" not in wide_src and wide.tuples == got.tuples
    rows, types = X.keyed_model(fam["key"], t)
    got, src = _answer(gpu_ctx, X.keyed_plan(fam["key"], t), [dt], rows, types, ordered=False)
    assert got.n_rows == len(rows) < X.ROWS


def test_a_mixed_case_below_an_aggregate_is_the_oracles(gpu_ctx, family):
    """(derived twice, tests/test_expr_edges_host.py: the oracle and the reference judge it, not the model)"""
    t, dt = family("E")
    plan = X.aggregation_plan(X.E_AGG_MIXED, t)
    want = orc.execute(plan)
    got, _ = _run(gpu_ctx, plan, [dt])
    assert got.text == want.text and got.tuples == want.tuples and [str(x) for x in got.types] == [str(x) for x in want.types]


# ---- family F: every typed form of the register aggregation ------------------------------------------------------------------------
@pytest.mark.parametrize("fid", [f.id for f in X.FORMS])
def test_typed_forms_at_the_ends_of_their_envelopes(gpu_ctx, monkeypatch, fid):
    """narrow == oracle == wide, order included; narrow == the model; the narrow source holds the form the case names"""
    f = X.FORM[fid]
    t = X.form_table(f)
    plan = X.form_plan(f, t)
    rows, types = X.form_model(f, t)
    dt = gpu_ctx.table(t)
    try:
        got, src = _answer(gpu_ctx, plan, [dt], rows, types, ordered=False)
        monkeypatch.setenv("RSQ_NARROW_SCANS", "0")
        wide, wide_src = _run(gpu_ctx, plan, [dt])
        monkeypatch.delenv("RSQ_NARROW_SCANS")
    finally:
        dt.close()
    assert f.text in src and not [a for a in f.absent if a in src]
    assert "ld2n" not in wide_src and "i32 n_" not in wide_src and "__umul24" not in wide_src and "__mul24" not in wide_src
    assert got.text == wide.text and got.tuples == wide.tuples


# ---- the finishing evaluators -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def finish(gpu_ctx):
    t = X.table_finish()
    dt = gpu_ctx.table(t)
    yield t, dt
    dt.close()


@pytest.mark.parametrize("name", sorted(X.FINISH))
def test_projections_over_aggregates_on_the_host_tail(gpu_ctx, finish, monkeypatch, capfd, name):
    t, dt = finish
    rows, types = X.finish_model(name, t)
    monkeypatch.setenv("RSQ_TRACE", "1")
    capfd.readouterr()
    _answer(gpu_ctx, X.finish_plan(name, t), [dt], rows, types, ordered=False)
    assert "device tail" not in capfd.readouterr().err


@pytest.mark.parametrize("computed_key", [False, True], ids=["dense", "hash_rows"])
def test_avg_on_the_device_tail(gpu_ctx, finish, monkeypatch, capfd, computed_key):
    """a negative sum its count does not divide, a sum x 100 that wraps, a group of one row: through k_dense_rows (the workgroup's LDS
    table) and through k_row_result_rows (the group rows of the generic hash aggregation)"""
    t, dt = finish
    rows, types = X.finish_model("avg", t)
    for k, v in ({} if computed_key else X.FEW).items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("RSQ_DEVICE_TAIL_MIN", "1")
    monkeypatch.setenv("RSQ_TRACE", "1")
    capfd.readouterr()
    _answer(gpu_ctx, X.finish_plan("avg", t, computed_key), [dt], rows, types, ordered=False)
    assert "device tail" in capfd.readouterr().err


# ---- the division error word --------------------------------------------------------------------------------------------------------
def _fails(ctx, plan, tabs):
    q = ctx.compile(plan, tabs)
    try:
        for _ in range(2):
            with pytest.raises(engine.EngineError) as e:
                q.execute()
            assert e.value.status == 5 and "Division by zero" in str(e.value)
    finally:
        q.close()


@pytest.mark.parametrize("n,at,kind", X.error_cases())
def test_division_error_word(gpu_ctx, n, at, kind):
    """the only trapping row first, on either side of the tile seam, last: the statement fails with RSQ_ERR_RUNTIME and the context goes
    on answering; the same row filtered out raises nothing; filtered by an AND beside the division it does (no short circuit)"""
    t = X.error_table(n, at, kind)
    guard = X.ERR_GUARD if kind == "zero" else X.ERR_GUARD_MIN
    dt = gpu_ctx.table(t)
    try:
        _fails(gpu_ctx, X.projection_plan([X.ERR_DIV], t), [dt])
        rows, types = X.project_model([X.ERR_DIV], t, where=guard)
        got, _ = _answer(gpu_ctx, X.projection_plan([X.ERR_DIV], t, where=guard), [dt], rows, types)
        assert got.n_rows == n - 1
        if kind == "zero":
            _fails(gpu_ctx, X.selection_plan(X.ERR_UNGUARDED, t), [dt])
            _answer(gpu_ctx, X.projection_plan([X.ERR_DIV], t, where=guard), [dt], rows, types)
    finally:
        dt.close()


# ---- the compat flag --------------------------------------------------------------------------------------------------------------
def test_int_to_bigint_extends_from_16_bits_under_the_compat_flag(gpu_ctx, family, monkeypatch):
    t, _ = family("C")
    wide_rows, _ = X.project_model(X.C_INT, t)
    rows, types = X.project_model(X.C_INT, t, int16=True)
    assert rows != wide_rows
    monkeypatch.setenv("RSQ_REFERENCE_INT16_CAST", "1")                   # (the oracle's switch for the same rule)
    ctx = engine.Context(device=0, compat_flags=engine.COMPAT_JIT_INT16_CAST)
    try:
        dt = ctx.table(t)
        try:
            _, src = _answer(ctx, X.projection_plan(X.C_INT, t), [dt], rows, types)
        finally:
            dt.close()
    finally:
        ctx.close()
    assert "((i64)(short)(" in src
