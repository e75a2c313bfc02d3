"""ORDER BY ... LIMIT over a materialisation decided from candidates the device selects (Context.set_order_limit(1); order_limit.hip,
engine_mattail.cpp orderLimitOnDevice, tail.cpp runOrderLimitTail).  The device path is never compared with itself: every statement is held
against (a) the CPU oracle, text and tuples byte for byte, and (b) the same compiled statement with the setter at 0.  Every case names
the path and the fallback reason it expects (tests/orderlimitcases.py) - none may fall back silently - and is executed twice, so the
warm materialisation (its write pass runs with the remembered row total) is covered.  The reference's own answers
(tests/golden/order_limit_reference.json) come through the statement loop."""
import json
import os

import numpy as np
import pytest

from resql_amd import engine, plan as P, tpch, tpch_full
from oracle import orc

import orderlimitcases as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def world(gpu_ctx):
    host = {k: O.TABLES[k]() for k in ("t", "few", "flags", "same")}
    tabs = {k: gpu_ctx.table(v) for k, v in host.items()}
    yield gpu_ctx, tabs, host
    for t in tabs.values():
        t.close()


@pytest.fixture(autouse=True)
def setter_back_at_the_default(gpu_ctx):
    yield
    gpu_ctx.set_order_limit(engine.ORDER_LIMIT_HOST)          # (the context is the session's)


def held_against_both_yardsticks(world, sql, name, path, reason):
    """-> (the statement's report under setting 1, the oracle's result)"""
    ctx, tabs, host = world
    want = orc.execute(ctx.sql_plan(sql, [tabs[name]], [host[name]]))
    q = ctx.sql_compile(sql, [tabs[name]])
    try:
        assert q.order_limit_report()["planned"] == (0 if reason == O.SHAPE else 1)
        ctx.set_order_limit(engine.ORDER_LIMIT_HOST)
        q.execute()
        base, rep0 = q.result(), q.order_limit_report()
        assert base.text == want.text and base.tuples == want.tuples, sql
        assert rep0["path"] == 0 and rep0["fallback_reason"] == O.NONE and rep0["candidates"] == 0 and rep0["select_ms"] == 0
        ctx.set_order_limit(engine.ORDER_LIMIT_DEVICE)
        for execution in range(2):
            q.execute()
            got, rep = q.result(), q.order_limit_report()
            assert got.text == want.text and got.tuples == want.tuples, (sql, execution)
            assert got.text == base.text and got.tuples == base.tuples
            assert (rep["path"], rep["fallback_reason"]) == (path, reason), (sql, execution, rep)
        return rep, want
    finally:
        q.close()


@pytest.mark.parametrize("sql,name,path,reason", O.DEVICE)
def test_decided_from_the_candidates(world, sql, name, path, reason):
    rep, want = held_against_both_yardsticks(world, sql, name, path, reason)
    limit = int(sql.rsplit("limit ", 1)[1])
    host = world[2][name]
    assert want.n_rows == limit
    assert rep["want"] == limit + 1 and rep["capacity"] == max(4 * (limit + 1), O.MIN_CAPACITY)
    assert rep["select_ms"] > 0 and rep["copy_ms"] > 0 and rep["tail_ms"] > 0
    first = sql.split("order by ")[1].split()[0].rstrip(",")
    if " where " not in sql and first in ("k", "d"):          # the candidates are numpy's: every row at or in front of the (limit + 1)-th leading value
        key = host.col(first).data
        key = key.view(np.int32) if key.dtype == np.uint32 else key          # (a DATE orders as signed 32 bits)
        _, where = O.expected_selection(key, " %s desc" % first in sql, limit + 1)
        assert rep["rows"] == host.n_rows and rep["candidates"] == len(where)
        assert rep["key_is32"] == (first == "d")
    else:
        assert limit + 1 <= rep["candidates"] <= rep["capacity"] and 4 * limit < rep["rows"] <= host.n_rows
    if " where " in sql:
        assert rep["rows"] == int((host.col("f").data == 7).sum())          # about one row in a hundred


@pytest.mark.parametrize("sql,name,path,reason", O.HOST)
def test_the_host_path_runs_and_says_why(world, sql, name, path, reason):
    rep, want = held_against_both_yardsticks(world, sql, name, path, reason)
    limit = int(sql.rsplit("limit ", 1)[1])
    host = world[2][name]
    if reason == O.SHAPE:
        assert rep["rows"] == 0 and rep["candidates"] == 0 and rep["first_key_column"] == -1
        return
    assert rep["want"] == limit + 1 and rep["capacity"] == max(4 * (limit + 1), O.MIN_CAPACITY)
    if reason == O.FEW_ROWS:          # decided before anything is launched
        assert 4 * limit >= rep["rows"] and rep["candidates"] == 0 and rep["select_ms"] == 0
        assert want.n_rows == min(limit, rep["rows"])
        assert rep["rows"] == (0 if " where " in sql else host.n_rows)
    elif reason == O.OVERFLOW:        # the count is exact: every row shares the first key's value
        assert rep["candidates"] == rep["rows"] == host.n_rows > rep["capacity"] and rep["select_ms"] > 0 and rep["tail_ms"] == 0
    else:                             # TIES: the leading six candidates tie on the only key; the answer is the quicksort's over the scan order
        flags = host.col("flag").data
        assert rep["candidates"] == int((flags == 0).sum()) and rep["rows"] == host.n_rows and rep["tail_ms"] > 0
        assert want.n_rows == limit


def test_partial_execution_answers_as_before_and_reports_the_shape(world):
    ctx, tabs, _ = world
    q = ctx.sql_compile(O.DEVICE[1][0], [tabs["t"]])
    try:
        errors = []
        for where in (engine.ORDER_LIMIT_HOST, engine.ORDER_LIMIT_DEVICE):
            ctx.set_order_limit(where)
            with pytest.raises(engine.EngineError) as e:
                q.execute_partial()
            errors.append((e.value.status, str(e.value)))
        assert errors[0] == errors[1] and errors[0][0] == 3
        rep = q.order_limit_report()
        assert rep["planned"] == 1 and rep["path"] == 0 and rep["fallback_reason"] == O.SHAPE
    finally:
        q.close()


def test_the_setter_is_read_at_every_execution(world):
    """compiled under 0, flipped between executions: each execution follows the value it finds"""
    ctx, tabs, host = world
    sql = O.DEVICE[4][0]
    want = orc.execute(ctx.sql_plan(sql, [tabs["t"]], [host["t"]]))
    ctx.set_order_limit(engine.ORDER_LIMIT_HOST)
    q = ctx.sql_compile(sql, [tabs["t"]])
    try:
        for where in (0, 1, 1, 0, 1, 0):
            ctx.set_order_limit(where)
            q.execute()
            got, rep = q.result(), q.order_limit_report()
            assert got.text == want.text and got.tuples == want.tuples
            assert (rep["path"], rep["fallback_reason"]) == (where, O.NONE)
            assert (rep["candidates"] > 0) == (where == 1)
    finally:
        q.close()


def test_behind_the_interpreter_tier(world, monkeypatch):
    """the statement answered by the whole-pipeline interpreter (as tests/test_gpu_generic_pipeline.py forces it): it fills the same
    columns, the selection reads them, the bytes are the same"""
    ctx, tabs, host = world
    monkeypatch.setenv("RSQ_GENERIC", "1")
    monkeypatch.setenv("RSQ_FORCE_GENERIC", "1")
    sql = "select k, u, d from t where f < 50 order by k desc, u limit 10"
    want = orc.execute(ctx.sql_plan(sql, [tabs["t"]], [host["t"]]))
    q = ctx.sql_compile(sql, [tabs["t"]])
    try:
        assert "generic pre-compiled interpreter" in q.explain and "forced" in q.explain
        for where in (1, 1, 0):
            ctx.set_order_limit(where)
            q.execute()
            got, rep = q.result(), q.order_limit_report()
            assert got.text == want.text and got.tuples == want.tuples
            assert (rep["path"], rep["fallback_reason"]) == (where, O.NONE)
    finally:
        q.close()


def test_shards_of_a_multi_context_keep_the_host_merge():
    """rsq_multi_* concatenates the shards' host columns and runs one tail over them: with the setter at 1 on every shard the shards
    hold their tails back (the shape is not the device path's) and the answer is the one-context answer"""
    n = 60_000
    host = tpch.synthetic_table(n, 64)

    def plan_of(t):
        p = P.Plan([t])
        node = p.projection([p.attr("b"), p.attr("c"), p.as_("e", p.add(p.attr("c"), p.attr("d")))], p.scan("t"))
        return p.set_root(p.orderby([p.desc(p.attr("c")), p.asc(p.attr("b"))], node), limit=50)

    want = orc.execute(plan_of(host))
    m = engine.MultiContext([0, 0, 0])
    try:
        shards = m.generate(engine.GEN_SYNTHETIC, n, 1.0, param=64)
        answers = []
        for where in (engine.ORDER_LIMIT_HOST, engine.ORDER_LIMIT_DEVICE):
            for s in m.shards:
                s.set_order_limit(where)
            q = m.compile(plan_of(tpch.synthetic_table(0, 64)), [[t] for t in shards])
            q.execute()
            answers.append(q.result())
            q.close()
        for got in answers:
            assert got.n_rows == want.n_rows == 50 and got.text == want.text and got.tuples == want.tuples
        for t in shards:
            t.close()
    finally:
        m.close()


def test_the_reference_answers_through_the_statement_loop(gpu_ctx):
    """what the unmodified reference answers for eight statements of the eligible shape over the eight-table database, from
    Database.execute under setting 1 - decided from the candidates every time"""
    with open(os.path.join(ROOT, "tests", "golden", "order_limit_reference.json")) as f:
        gold = json.load(f)
    tables = tpch_full.database(gold["sf"])
    db = engine.Database(gpu_ctx)
    try:
        for k in gold["tables"]:
            db.add_table(gpu_ctx.table(tables[k]))
        gpu_ctx.set_order_limit(engine.ORDER_LIMIT_DEVICE)
        for case in gold["cases"]:
            got = db.execute(case["sql"])
            rep = db.order_limit_report
            assert got.text == case["result"], case["sql"]
            assert (rep["planned"], rep["path"], rep["fallback_reason"]) == (1, 1, O.NONE), (case["sql"], rep)
            assert rep["want"] == case["limit"] + 1 <= rep["candidates"]
        gpu_ctx.set_order_limit(engine.ORDER_LIMIT_HOST)
        got = db.execute(gold["cases"][0]["sql"])
        assert got.text == gold["cases"][0]["result"] and db.order_limit_report["path"] == 0
    finally:
        db.close()
