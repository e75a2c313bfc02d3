"""Derived aggregations on a compile-only context (no GPU): every plan of tests/derivedcases.py compiles, in a child process of its
own so that a crash of the compiler fails one test, and its explain text names each derived table and its sub-query.  Plans the
engine leaves out (a derived aggregation in a nested-loops plan) and plans the reference refuses fail with the expected status and,
for the latter, the reference's words (tests/golden/derived_agg_reference.json)."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import derivedcases as D  # noqa: E402
from resql_amd import engine, tpch_full  # noqa: E402
from resql_amd import plan as P  # noqa: E402

# derived tables each plan has at its top level (the sub-queries hold the deeper ones)
DERIVED = {"two_derived_sides": 2}

CHILD = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import derivedcases as D
from resql_amd import engine, tpch_full
db = tpch_full.database(0.01)
ctx = engine.Context(device=-1)
plan = getattr(D, {name!r})(db)
tabs = [ctx.table(t) for t in plan.tables]
try:
    q = ctx.compile(plan, tabs)
except engine.EngineError as e:
    print("STATUS", e.status, e); sys.exit(3)
sys.stdout.write(q.explain)
q.close(); ctx.close()
"""


@pytest.mark.parametrize("case", [f.__name__ for f in D.CASES])
def test_compiles_in_child_with_derived_tables(case):
    r = subprocess.run([sys.executable, "-X", "faulthandler", "-c", CHILD.format(root=ROOT, tests=HERE, name=case)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "compile of %s ended with %d\n%s%s" % (case, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    n = DERIVED.get(case, 1)
    for k in range(n):
        assert "derived table derived%d (" % k in r.stdout, r.stdout
        assert "scan derived%d [rows of this execution" % k in r.stdout, r.stdout
    assert sum(1 for l in r.stdout.splitlines() if l.startswith("derived table ")) == n, r.stdout
    assert "  | pipeline 0: scan " in r.stdout, r.stdout


@pytest.fixture(scope="module")
def small():
    db = tpch_full.database(0.01)
    ctx = engine.Context(device=-1, engine_flags=engine.ENGINE_NESTED_LOOPS)
    tabs = [ctx.table(db[k]) for k in D.TABLES]
    yield db, ctx, tabs
    for t in tabs:
        t.close()
    ctx.close()


def test_explain_names_columns_in_reference_numbering(small):
    db, ctx, tabs = small
    q = ctx.compile(D.agg_over_agg(db), tabs)
    try:
        assert "columns l_orderkey:INT|expr3:BIGINT" in q.explain, q.explain
    finally:
        q.close()


def test_three_levels_nest_sub_queries(small):
    db, ctx, tabs = small
    q = ctx.compile(D.agg_three_deep(db), tabs)
    try:
        assert "  |   | pipeline 0: scan orders" in q.explain, q.explain
    finally:
        q.close()


def test_nested_loops_plan_with_derived_aggregation_is_refused(small):
    db, ctx, tabs = small
    p = D._plan(db)
    c = p.count(p.star())
    a = p.aggregation([c], [p.attr("n_regionkey")], p.scan("nation"))
    p.set_root(p.materialize(p.nestedloopsjoin(p.materialize(p.scan("region")), a)), request_all=True)
    with pytest.raises(engine.EngineError) as e:
        ctx.compile(p, tabs)
    assert e.value.status == 3
    assert "derived aggregation grouped by [n_regionkey]" in str(e.value) and "nested-loops" in str(e.value)


@pytest.mark.parametrize("case,status", [(f.__name__, s) for f, s in D.REFUSED])
def test_refused_with_the_reference_words(small, case, status):
    with open(os.path.join(HERE, "golden", "derived_agg_reference.json")) as f:
        words = json.load(f)["refused"][case]
    assert words.startswith("ResqlError: ")
    db, ctx, tabs = small
    with pytest.raises(engine.EngineError) as e:
        ctx.compile(getattr(D, case)(db), tabs)
    assert e.value.status == status
    assert words[len("ResqlError: "):] in str(e.value), (str(e.value), words)
