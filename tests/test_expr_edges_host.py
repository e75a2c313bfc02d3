"""tests/exprcases.py before any kernel runs: the plain integer model against the oracle on every statement of every family, values
and result types, and against the unmodified reference where it is built; the refusals and their messages; the texts the code
generator gives each statement (the rsq:: functions of the row functions, the typed form of every family-F case); and that every
family-F table reaches the boundary of its form - an emission one class too narrow gives another value in rows 0-7 and again at the
tile seam or in the tail."""
import os
import sys

import pytest

from oracle import orc
from resql_amd import plan as P

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exprcases as X  # noqa: E402

needs_ref = pytest.mark.skipif(not orc.have_reference(), reason="oracle/_ref/ref_harness not built")
FAMILY_IDS = sorted(X.FAMILIES)
INT16 = ("C", "D")                       # the families with INT -> BIGINT casts: the reference's JIT extends them from 16 bits


@pytest.fixture(scope="module")
def ctx(tmp_path_factory):
    from resql_amd import engine
    c = engine.Context(device=-1, cache_dir=str(tmp_path_factory.mktemp("kcache_expr_edges")))
    yield c
    c.close()


@pytest.fixture(scope="module")
def tables():
    return {name: fam["table"]() for name, fam in X.FAMILIES.items()}


def _source(ctx, plan):
    tabs = [ctx.table(t) for t in plan.tables]
    try:
        q = ctx.compile(plan, tabs)
        try:
            return q.source, q.explain
        finally:
            q.close()
    finally:
        for t in tabs:
            t.close()


def _same(res, rows, types, ordered=True):
    assert [str(t) for t in res.types] == [str(t) for t in types]
    assert (res.rows() if ordered else sorted(res.rows())) == rows


def statements(name, t, int16=False):
    """(what, plan, model rows, model types, ordered) of every statement of a family"""
    fam = X.FAMILIES[name]
    out = []
    for i, exprs in enumerate(fam["projections"]):
        out.append((f"projection {i}", X.projection_plan(exprs, t)) + X.project_model(exprs, t, int16=int16) + (True,))
    for i, c in enumerate(fam["predicates"]):
        out.append((f"predicate {i}", X.selection_plan(c, t)) + X.project_model([], t, where=c, int16=int16) + (True,))
    if not int16:
        out.append(("aggregation", X.aggregation_plan(fam["agg"], t)) + X.aggregate_model(fam["agg"], t) + (False,))
        out.append(("computed key", X.keyed_plan(fam["key"], t)) + X.keyed_model(fam["key"], t) + (False,))
    return out


# ---- the model is the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FAMILY_IDS)
def test_model_is_the_oracle(tables, name):
    for what, plan, rows, types, ordered in statements(name, tables[name]):
        res = orc.execute(plan)
        _same(res, rows, types, ordered)
        assert res.serialize() == res.text                               # (plan.Result's writer, which the GPU tests read results through)


def test_the_smallest_decimal_keeps_its_own_sign_in_every_writer(tables):
    """INT64_MIN as a DECIMAL: '-' and the digits of a signed negation, which is INT64_MIN again - in the oracle's text and in
    plan.Result's (the engine's own writers: tests/test_gpu_result_text.py)"""
    res = orc.execute(X.projection_plan([X.col("da")], tables["A"]))
    assert res.value(0, 1) == X.I64_MIN and res.serialize_value(0, 1) == "--92233720368547758.08"
    assert res.text.splitlines()[1] == "0|--92233720368547758.08|"


@pytest.mark.parametrize("name", INT16)
def test_model_is_the_oracle_under_the_16_bit_cast(tables, name, monkeypatch):
    monkeypatch.setenv("RSQ_REFERENCE_INT16_CAST", "1")
    differs = False
    for what, plan, rows, types, ordered in statements(name, tables[name], int16=True):
        _same(orc.execute(plan), rows, types, ordered)
        differs |= rows != X.project_model(X.FAMILIES[name]["projections"][int(what.split()[1])], tables[name])[0] if what.startswith("projection") else False
    assert differs                                                        # (the 16-bit rule changes an answer of the family)


def test_computed_keys_meet_only_after_the_wrap(tables):
    """family A's key a * b: rows whose exact products differ fall into one group of the wrapped product"""
    t = tables["A"]
    rows = X.rows_of(t)
    exact = {r["a"] * r["b"] for r in rows}
    wrapped = {X.wrap64(v) for v in exact}
    assert len(wrapped) < len(exact) and len(X.keyed_model(X.A_KEY, t)[0]) == len(wrapped)


def test_a_mixed_case_below_an_aggregate_is_derived_twice(tables):
    """the aggregation's pass casts the branches, the projection's pass derives the cast CASE again: sum(case .. then BIGINT else DECIMAL(12,2))
    is a DECIMAL(19,0) - not what one pass gives (the model's type), in the oracle as in the reference"""
    t = tables["E"]
    res = orc.execute(X.aggregation_plan(X.E_AGG_MIXED, t))
    assert [str(x) for x in res.types[1:7]] == ["BIGINT"] * 3 + ["DECIMAL(19,0)"] * 3
    assert str(X.typed(X.E_AGG_MIXED[1], X.schema_of(t)).type) == "DECIMAL(12,2)"


def test_types_the_two_orders_of_a_mixed_case_give(tables):
    s = X.schema_of(tables["E"])
    assert str(X.typed(X.E_EXPRS[0], s).type) == "BIGINT" and str(X.typed(X.E_EXPRS[1], s).type) == "DECIMAL(12,2)"
    assert X.constant("4294967297", P.BIGINT)[0] == 1


# ---- the division error word --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,at,kind", X.error_cases())
def test_trap_cases_fail_in_the_oracle_as_in_the_model(n, at, kind):
    t = X.error_table(n, at, kind)
    guard = X.ERR_GUARD if kind == "zero" else X.ERR_GUARD_MIN
    with pytest.raises(X.Trap):
        X.project_model([X.ERR_DIV], t)
    with pytest.raises(orc.OracleError, match="Division"):
        orc.execute(X.projection_plan([X.ERR_DIV], t))
    rows, types = X.project_model([X.ERR_DIV], t, where=guard)           # the trapping row filtered out: an answer
    assert len(rows) == n - 1
    _same(orc.execute(X.projection_plan([X.ERR_DIV], t, where=guard)), rows, types)
    if kind == "zero":                                                   # AND has no short circuit
        with pytest.raises(X.Trap):
            X.project_model([], t, where=X.ERR_UNGUARDED)
        with pytest.raises(orc.OracleError, match="Division by zero"):
            orc.execute(X.selection_plan(X.ERR_UNGUARDED, t))


def test_family_b_holds_every_pairing_and_no_trapping_one(tables):
    rows = X.rows_of(tables["B"])
    pairs = {(r["a"], r["b"]) for r in rows}
    assert {(a, b) for a in X.DIVIDENDS for b in X.DIVISORS} - {(X.I64_MIN, -1)} <= pairs
    assert (X.I64_MIN, -1) not in pairs and all(r["b"] for r in rows)


# ---- the unmodified reference -------------------------------------------------------------------------------------------------------
def _reference_text(text):
    """the oracle's text as the reference binary writes it: a DECIMAL INT64_MIN is negated there in a signed multiplication (undefined;
    values.h:103-109) and the binary prints one sign where the oracle and the engine print the wrapped negation's second one"""
    return text.replace("--", "-")


@needs_ref
@pytest.mark.parametrize("name", FAMILY_IDS)
def test_oracle_is_the_reference(tables, name, monkeypatch):
    """every statement of A-E the reference can compile and whose answer it defines: a CASE without ELSE leaves its result register as
    it was (ExpressionsJitFlounder.h:720-754), so those expressions stay out; INT -> BIGINT compares under the 16-bit switch"""
    if name in INT16:
        monkeypatch.setenv("RSQ_REFERENCE_INT16_CAST", "1")
    fam, t = X.FAMILIES[name], tables[name]
    plans = []
    for exprs in fam["projections"]:
        keep = [e for e in exprs if not X.has_open_case(e)]
        if keep:
            plans.append(X.projection_plan(keep, t))
    plans += [X.selection_plan(c, t) for c in fam["predicates"] if not X.has_open_case(c)]
    keep = [e for e in fam["agg"] if not X.has_open_case(e)]
    plans += [X.aggregation_plan(keep, t), X.keyed_plan(fam["key"], t)]
    if name == "E":
        plans.append(X.aggregation_plan(X.E_AGG_MIXED, t))
    for plan in plans:
        assert orc.run_reference(plan)[0] == _reference_text(orc.execute(plan).text)


# ---- what the code generator makes of them --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FAMILY_IDS)
def test_projections_call_the_functions_their_expressions_need(ctx, tables, name):
    t = tables[name]
    s = X.schema_of(t)
    for exprs in X.FAMILIES[name]["projections"]:
        src, _ = _source(ctx, X.projection_plan(exprs, t))
        want = set().union(*[X.functions(X.typed(e, s)) for e in exprs])
        for f in ("rsq::add(", "rsq::sub(", "rsq::mul(", "rsq::div("):
            assert (f in src) == (f in want), f
        assert ("a.err)" in src) == ("rsq::div(" in want)


@pytest.mark.parametrize("expr,predicate,message", X.C_REFUSED, ids=["scale_difference_9", "int_plus_int", "int_less_than_int", "decimal_division"])
def test_refusals_and_their_messages(ctx, tables, expr, predicate, message):
    from resql_amd import engine
    t = tables["C"]
    plan = X.selection_plan(expr, t) if predicate else X.projection_plan([expr], t)
    with pytest.raises(X.Refused, match=message.replace("(", r"\(").replace(")", r"\)")):
        X.typed(expr, X.schema_of(t))
    with pytest.raises(engine.EngineError) as e:
        _source(ctx, plan)
    assert e.value.status == 2 and message in str(e.value)
    with pytest.raises(orc.OracleError):
        orc.execute(plan)


def test_the_compat_flag_extends_from_16_bits(tmp_path):
    from resql_amd import engine
    t = X.table_c()
    c = engine.Context(device=-1, cache_dir=str(tmp_path), compat_flags=engine.COMPAT_JIT_INT16_CAST)
    try:
        src, _ = _source(c, X.projection_plan(X.C_INT, t))
    finally:
        c.close()
    assert "((i64)(short)(" in src


@pytest.mark.parametrize("fid", [f.id for f in X.FORMS])
def test_family_f_source_holds_the_form(ctx, fid):
    f = X.FORM[fid]
    t = X.form_table(f)
    plan = X.form_plan(f, t)
    src, ex = _source(ctx, plan)
    assert "in registers" in ex and f.text in src and not [a for a in f.absent if a in src]
    assert "rsq::dec<i32>(" in src or "rsq::ld2n(" in src or fid.startswith("decode_i64")      # narrow images
    rows, types = X.form_model(f, t)
    _same(orc.execute(plan), rows, types, ordered=False)
    assert len(rows) == 3


# ---- every family-F table reaches its boundary --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", [f.id for f in X.FORMS if f.narrow])
def test_family_f_tables_reach_their_boundary(fid):
    """an emission one class too narrow - an unsigned or signed widening product, or a widened sum, as a wrapped 32-bit one; a 24-bit
    multiply with 23 / 22-bit operands; a plain 32-bit product as a 24-bit multiply - differs from the exact value in rows 0-7 and again
    in rows 126-129 or the last two"""
    f = X.FORM[fid]
    pairs = X.narrower(f, X.form_table(f))
    for rows in X.EDGE_ROWS:
        assert [i for i in rows if pairs[i][0] != pairs[i][1]], (fid, rows)


def test_family_f_sums_reach_their_last_values():
    """the forms with no class below them: the 32-bit sum and difference at 2^31 - 2 and +-(2^31 - 1), the i32 decode at +-(2^31 - 1), the
    i64 decode one past it"""
    def values(fid):
        f = X.FORM[fid]
        t = X.form_table(f)
        n = X.typed(f.expr, X.schema_of(t))
        v = [X.compute(n, r) for r in X.rows_of(t)]
        return [{v[i] for i in rows} for rows in X.EDGE_ROWS]
    for fid, ends in (("add32_30p30", {X.M31 - 1}), ("sub32_31m31", {X.M31, -X.M31}), ("decode_i32_top", {X.M31}), ("decode_i32_bottom", {-X.M31}),
                      ("decode_i64_top", {X.M31 + 1}), ("decode_i64_bottom", {-X.M31 - 1}), ("uwide_16x16", {4294836225})):
        for seen in values(fid):
            assert ends <= seen, (fid, ends)


# ---- the finishing evaluators' table ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(X.FINISH))
def test_finishing_model_is_the_oracle(name):
    t = X.table_finish()
    rows, types = X.finish_model(name, t)
    _same(orc.execute(X.finish_plan(name, t)), rows, types, ordered=False)


def test_avg_table_has_its_three_groups():
    t = X.table_finish()
    rows = X.rows_of(t)
    sums = {g: sum(r["a"] for r in rows if r["g"] == g) for g in (0, 1, 2)}
    counts = {g: sum(1 for r in rows if r["g"] == g) for g in (0, 1, 2)}
    assert counts[0] == 1 and sums[1] < 0 and (sums[1] * 100) % counts[1] != 0
    assert not X.I64_MIN <= sums[2] * 100 <= X.I64_MAX and X.I64_MIN <= sums[2] <= X.I64_MAX


# ---- the builder and the warm-up ----------------------------------------------------------------------------------------------------
def test_builder_refuses_a_node_below_two_parents():
    p = P.Plan([X.table_e()])
    b = X.Builder(p)
    n = b.node(X.col("p"))
    b.wrap(p.sum, n)
    with pytest.raises(ValueError, match="already the child"):
        b.wrap(p.min, n)
    e = X.add(X.col("p"), X.col("p"))
    q = P.Plan([X.table_e()])
    root = X.Builder(q).node(X.mul(e, e))                               # one tuple used twice: four attribute nodes, two ADD nodes
    assert len(q.exprs) == 7 and len({c for x in q.exprs for c in x.children}) == 6 and root == 6


def test_warm_up_list_fits_the_build():
    plans = list(X.warm_plans())
    assert 40 <= len(plans) <= 96
