"""Nested-loops joins, opt-in per context (RSQ_ENGINE_NESTED_LOOPS): the SQL front end folds pieces that no equality links the
way the reference's planner does (planner.h:458-469), and the configuration field that bounds the pairs.  No GPU needed."""
import json
import os

import pytest

from resql_amd import engine, tpch_full

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "nlj_reference.json")) as f:
    GOLD = json.load(f)


@pytest.fixture(scope="module")
def flagged():
    ctx = engine.Context(device=-1, engine_flags=engine.ENGINE_NESTED_LOOPS)
    db = tpch_full.database(GOLD["sf"])
    tabs = [ctx.table(db[k]) for k in GOLD["tables"]]
    yield ctx, tabs
    for t in tabs:
        t.close()
    ctx.close()


def test_fixtures_cover_the_cases():
    assert len(GOLD["cases"]) >= 30
    assert sum("refused" in c for c in GOLD["cases"]) >= 2
    assert all("NESTEDLOOPSJOIN" in c["plan"] for c in GOLD["cases"])


@pytest.mark.parametrize("i", range(len(GOLD["cases"])))
def test_plan_text_is_the_reference_planners(flagged, i):
    """operator tree, MaterializeOp wrappers and fold order (creation order of the pieces' roots) as the reference's planner makes them"""
    ctx, tabs = flagged
    c = GOLD["cases"][i]
    assert ctx.sql_plan_text(c["sql"], tabs) == c["plan"], c["sql"]


def test_the_issue_statements_fold_in_creation_order(flagged):
    ctx, tabs = flagged
    t = ctx.sql_plan_text("select * from region, nation where r_regionkey = 1 and n_nationkey < 3", tabs)
    assert t.splitlines()[1].startswith("MATERIALIZE {NESTEDLOOPSJOIN {MATERIALIZE {SELECTION")
    assert t.index("SCAN region") < t.index("SCAN nation")
    t = ctx.sql_plan_text("select count(*) from nation, region, supplier where n_regionkey < r_regionkey and s_suppkey < 3 and "
                          "n_nationkey < 2", tabs)
    assert t.index("SCAN region") < t.index("SCAN supplier") < t.index("SCAN nation")
    assert t.count("NESTEDLOOPSJOIN") == 2


def test_type_errors_stay_errors_on_a_flagged_context(flagged):
    """INT < INT between two columns: the reference refuses it in code generation; so does the engine (RSQ_ERR_TYPE)"""
    ctx, tabs = flagged
    with pytest.raises(engine.EngineError) as e:
        ctx.sql_compile("select count(*) from nation, region where n_regionkey < r_regionkey", tabs)
    assert e.value.status == 2
    assert "LESS_THAN code generation not implemented for datatype" in str(e.value)


def test_without_the_flag_the_plan_is_refused():
    ctx = engine.Context(device=-1)
    db = tpch_full.database(GOLD["sf"])
    tabs = [ctx.table(db[k]) for k in GOLD["tables"]]
    try:
        for c in GOLD["cases"][:5]:
            with pytest.raises(engine.EngineError, match="nested-loops") as e:
                ctx.sql_plan_text(c["sql"], tabs)
            assert e.value.status == 3
    finally:
        for t in tabs:
            t.close()
        ctx.close()


def test_c_abi_plan_needs_the_flag():
    from resql_amd import plan as P
    db = tpch_full.database(GOLD["sf"])
    p = P.Plan([db["region"], db["nation"]])
    nlj = p.nestedloopsjoin(p.scan("region"), p.scan("nation"))
    p.set_root(p.materialize(p.projection([p.attr("r_name"), p.attr("n_name")], nlj)))
    for flags, status in ((0, 3), (engine.ENGINE_NESTED_LOOPS, 0)):
        ctx = engine.Context(device=-1, engine_flags=flags)
        tabs = [ctx.table(db["region"]), ctx.table(db["nation"])]
        try:
            if status:
                with pytest.raises(engine.EngineError) as e:
                    ctx.compile(p, tabs)
                assert e.value.status == status
            else:
                ctx.compile(p, tabs).close()
        finally:
            for t in tabs:
                t.close()
            ctx.close()


def test_old_size_config_reads_the_budget_as_zero():
    """a host built against the header before nested_loops_max_pairs: the field is not read (0: the default)"""
    cfg = engine.rsq_config.make(-1, engine_flags=engine.ENGINE_NESTED_LOOPS, nested_loops_max_pairs=-5)
    cfg.struct_size = engine.rsq_config.nested_loops_max_pairs.offset
    L = engine.lib()
    h = engine.C.c_void_p()
    assert L.rsq_ctx_create(engine.C.byref(cfg), engine.C.byref(h)) == 0
    L.rsq_ctx_destroy(h)


def test_negative_budget_is_invalid():
    with pytest.raises(engine.EngineError) as e:
        engine.Context(device=-1, engine_flags=engine.ENGINE_NESTED_LOOPS, nested_loops_max_pairs=-1)
    assert e.value.status == 1
    assert "nested_loops_max_pairs" in str(e.value)
