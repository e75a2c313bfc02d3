"""Derived aggregations on the GPU: every plan of tests/derivedcases.py gives the reference's bytes (tests/golden/derived_agg_reference.json,
recorded by tests/golden/make_derived_agg_golden.py) on both kernel tiers; at SF1 and after an adopted input column is rewritten the
repository oracle (orc.execute) stands in for it.  Both inputs of the derived-table writer (device tail and host tail), repeated
executions, any emission order as a multiset, the report, the ReSQL binding; partial and multi-GPU execution refuse such plans."""
import hashlib
import json
import os
import sys

import numpy as np

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import derivedcases as D  # noqa: E402
from oracle import orc  # noqa: E402
from resql_amd import engine, tpch_full  # noqa: E402
from resql_amd import plan as P  # noqa: E402

with open(os.path.join(HERE, "golden", "derived_agg_reference.json")) as f:
    GOLD = json.load(f)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small(ctx):
    db = tpch_full.database(0.01)
    tabs = [ctx.table(db[k]) for k in D.TABLES]
    yield db, tabs
    for t in tabs:
        t.close()


def _run(ctx, plan, tabs):
    q = ctx.compile(plan, tabs)
    try:
        q.execute()
        return q.result().text
    finally:
        q.close()


def _run_case(ctx, small, case):
    db, tabs = small
    plan = getattr(D, case)(db)
    if case in D.LITERAL:          # (the two literal tables of the edge cases)
        return ctx.run(plan).text
    return _run(ctx, plan, tabs)


def _matches_reference(case, text):
    g = GOLD["cases"][case]
    if "text" in g:
        assert text == g["text"]
    assert text.count("\n") - 1 == g["rows"]
    assert hashlib.sha256(text.encode()).hexdigest() == g["sha256"]


def test_fixture_covers_every_case():
    assert sorted(GOLD["cases"]) == sorted(f.__name__ for f in D.CASES)


@pytest.mark.parametrize("case", [f.__name__ for f in D.CASES])
def test_case_matches_reference(ctx, small, case):
    _matches_reference(case, _run_case(ctx, small, case))


@pytest.mark.parametrize("case", [f.__name__ for f in D.CASES])
def test_case_same_bytes_with_forced_interpreters(ctx, small, case, monkeypatch):
    monkeypatch.setenv("RSQ_FORCE_GENERIC", "1")
    _matches_reference(case, _run_case(ctx, small, case))


def test_repeated_executions(ctx, small):
    db, tabs = small
    q = ctx.compile(D.q18(db), tabs)
    try:
        for _ in range(3):
            q.execute()
            _matches_reference("q18", q.result().text)
    finally:
        q.close()


def _sub_plan(db):
    p = D._plan(db)
    s = p.sum(p.attr("l_quantity"))
    return p.set_root(p.materialize(p.aggregation([s], [p.attr("l_orderkey")], p.scan("lineitem"))), request_all=True)


def test_report_counts_the_sub_query(ctx, small):
    """having_hash_key = the sub-query (the aggregation as a statement of its own) + the writer + the materialisation over the
    derived table (count and write passes)"""
    db, tabs = small
    sub = ctx.compile(_sub_plan(db), tabs)
    q = ctx.compile(D.having_hash_key(db), tabs)
    try:
        sub.execute(); sub.execute()
        q.execute(); q.execute()
        assert q.report().num_kernels >= sub.report().num_kernels + 1 + 2
        assert q.report().bytes_read > sub.report().bytes_read
    finally:
        q.close()
        sub.close()


def test_overwritten_adopted_column_gives_the_new_answer(ctx):
    """one compiled query; l_quantity is rewritten in place between executions: the derived table is recomputed"""
    import torch
    db = tpch_full.database(0.01)
    li = db["lineitem"]
    tok, tq = li.col("l_orderkey").type, li.col("l_quantity").type
    ok = np.ascontiguousarray(li.col("l_orderkey").data)
    qty = np.ascontiguousarray(li.col("l_quantity").data).copy()
    dok, dq = torch.from_numpy(ok).cuda(), torch.from_numpy(qty).cuda()
    t = ctx.table_from_device("lineitem", len(ok), [("l_orderkey", tok, dok.data_ptr()), ("l_quantity", tq, dq.data_ptr())])

    def plan(qv):
        p = P.Plan([P.Table("lineitem", [P.Column("l_orderkey", tok, ok), P.Column("l_quantity", tq, qv)], len(ok))])
        s = p.sum(p.attr("l_quantity"))
        a = p.aggregation([s], [p.attr("l_orderkey")], p.scan("lineitem"))
        return p.set_root(p.materialize(p.selection(p.gt(s, p.constant(250, P.DECIMAL)), a)), request_all=True)

    q = ctx.compile(plan(qty), [t])
    try:
        q.execute()
        first = q.result().text
        assert first == orc.execute(plan(qty)).text
        dq.mul_(2)
        torch.cuda.synchronize()
        q.execute()
        second = q.result().text
        assert second == orc.execute(plan(qty * 2)).text
        assert second.count("\n") > first.count("\n")
    finally:
        q.close()
        t.close()


def test_compile_execute_destroy_twice(ctx, small):
    db, tabs = small
    for _ in range(2):
        _matches_reference("two_derived_sides", _run(ctx, D.two_derived_sides(db), tabs))


@pytest.mark.skipif(not orc.have_reference(), reason="oracle/_ref/ref_harness was not shipped")
def test_q18_through_the_resql_binding(small):
    db, _ = small
    hip, _ = orc.run_reference(D.q18(db), engine="hip")
    _matches_reference("q18", hip)


def test_emit_any_is_a_multiset_of_the_answer(small):
    db, _ = small
    c = engine.Context(device=0, emission_order=engine.EMIT_ANY)
    tabs = [c.table(db[k]) for k in D.TABLES]
    try:
        got = _run(c, D.agg_over_string_key(db), tabs).splitlines()
        want = GOLD["cases"]["agg_over_string_key"]["text"].splitlines()
        assert got[0] == want[0] and sorted(got[1:]) == sorted(want[1:])
    finally:
        for t in tabs:
            t.close()
        c.close()


def test_partial_execution_refused(ctx, small):
    db, tabs = small
    q = ctx.compile(D.having_ungrouped(db), tabs)
    try:
        with pytest.raises(engine.EngineError) as e:
            q.execute_partial()
        assert e.value.status == 3 and "derived aggregation" in str(e.value)
    finally:
        q.close()


def test_multi_context_refused(small):
    db, _ = small
    m = engine.MultiContext([0, 0])
    shards = [[m.shards[i].table(db[k]) for k in D.TABLES] for i in range(2)]
    try:
        with pytest.raises(engine.EngineError) as e:
            m.compile(D.having_hash_key(db), shards)
        assert e.value.status == 3 and "derived aggregation" in str(e.value)
    finally:
        for s in shards:
            for t in s:
                t.close()
        m.close()


def test_device_tail_and_host_tail_give_same_bytes(ctx, monkeypatch, capfd):
    db = tpch_full.database(0.1, fill_unused=False)
    tabs = [ctx.table(db[k]) for k in D.TABLES]
    try:
        monkeypatch.setenv("RSQ_TRACE", "1")
        dev = _run(ctx, D.agg_over_agg(db), tabs)
        err = capfd.readouterr().err
        assert "derived0: " in err and "from the device tail's tuples" in err, err[-3000:]
        monkeypatch.setenv("RSQ_DEVICE_TAIL", "0")
        host = _run(ctx, D.agg_over_agg(db), tabs)
        err = capfd.readouterr().err
        assert "from the host tail's tuples" in err
        assert dev == host == orc.execute(D.agg_over_agg(db)).text
    finally:
        for t in tabs:
            t.close()


@pytest.mark.parametrize("case", ["q18", "agg_over_agg", "build_side", "two_derived_sides"])
def test_sf1_matches_oracle(ctx, case):
    db = tpch_full.database(1.0, fill_unused=False)
    tabs = [ctx.table(db[k]) for k in D.TABLES]
    try:
        build = (lambda d: D.q18(d, threshold=300)) if case == "q18" else getattr(D, case)
        got = _run(ctx, build(db), tabs)
        assert got == orc.execute(build(db)).text
        if case == "q18":
            assert got.count("\n") - 1 == 79
    finally:
        for t in tabs:
            t.close()
