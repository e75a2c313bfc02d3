"""A materialisation's result tuples packed on the device (Context.set_result_pack(1); result_pack.hip, engine_mattail.cpp resultPackOnDevice) and
read there by the device text (result_text.hip).  The device path is never compared with itself: every statement is held against (a) the
CPU oracle, tuples and text byte for byte, and (b) the same compiled statement with the setter at 0.  Every case names the path, the
fallback reason and sorted_on_host it expects (tests/resultpackcases.py) - none may fall back silently - and is executed twice under
setting 1, so the warm materialisation (its write pass runs with the remembered row total) is covered, then once more under 0 and under
1 on the same compiled statement, so buffer lifetimes and the reset of the result's device pointer are.  The reference's own answers
(tests/golden/result_pack_reference.json) come through the statement loop."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from resql_amd import engine, plan as P, tpch
from oracle import orc

import resultpackcases as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST, DEVICE = engine.RESULT_PACK_HOST, engine.RESULT_PACK_DEVICE


@pytest.fixture(scope="module")
def world(gpu_ctx):
    host = {k: make() for k, make in R.TABLES.items()}
    tabs = {k: gpu_ctx.table(v) for k, v in host.items()}
    yield gpu_ctx, tabs, host
    for t in tabs.values():
        t.close()


@pytest.fixture(autouse=True)
def setters_back_at_their_defaults(gpu_ctx):
    yield
    gpu_ctx.set_result_pack(HOST)          # (the context is the session's)
    gpu_ctx.set_order_limit(engine.ORDER_LIMIT_HOST)
    gpu_ctx.set_result_text(0)


def host_text(q) -> bytes:
    """rsq_result_serialize of the statement's result view: the host's text of the tuples the view hands out"""
    L = engine.lib()
    v = P.rsq_result_view()
    q.ctx._check(L.rsq_query_result(q.h, C.byref(v)))
    p = L.rsq_result_serialize(C.byref(v))
    assert p
    try:
        return C.string_at(p)
    finally:
        L.rsq_free(p)


def schema_line(res) -> str:
    return "#schema " + "".join(f"{n}:{t}|" for n, t in zip(res.names, res.types)) + "\n"


def executed(q, want, base=None):
    """one execution: its tuples and host text against the oracle's (and the setting-0 execution's), its device text against its host text
    -> (result, host text, pack report, text report)"""
    q.execute()
    got, text, rep = q.result(text=False), host_text(q), q.result_pack_report()
    assert got.n_rows == want.n_rows and got.tuples == want.tuples
    assert schema_line(got) + text.decode("latin1") == want.text
    if base is not None:
        assert got.tuples == base[0].tuples and text == base[1]
    dev_text, text_rep = q.result_text(mode=engine.TEXT_DEVICE)
    assert dev_text == text and text_rep["path"] == 1
    return got, text, rep, text_rep


@pytest.mark.parametrize("name,sql,names,order_limit,path,reason,sorted_on_host", R.CASES, ids=R.CASE_IDS)
def test_held_against_the_oracle_and_setting_0(world, name, sql, names, order_limit, path, reason, sorted_on_host):
    ctx, tabs, host = world
    want = orc.execute(ctx.sql_plan(sql, [tabs[n] for n in names], [host[n] for n in names]))
    ctx.set_order_limit(order_limit)
    q = ctx.sql_compile(sql, [tabs[n] for n in names])
    try:
        assert q.result_pack_report()["planned"] == (0 if reason == R.SHAPE else 1)
        ctx.set_result_pack(HOST)
        for execution in range(2):          # (the second is warm, as every execution under setting 1 below)
            base = executed(q, want)
            rep0, kernels0 = base[2], q.report().num_kernels
            assert (rep0["path"], rep0["fallback_reason"], rep0["sorted_on_host"]) == (0, R.NONE, 0)
            assert rep0["kernel_ms"] == 0 and rep0["copy_ms"] == 0 and rep0["sort_ms"] == 0 and base[3]["tuples_from_device"] == 0
        for where in (DEVICE, DEVICE, HOST, DEVICE):
            ctx.set_result_pack(where)
            got, text, rep, text_rep = executed(q, want, base)
            if where == HOST:          # whatever ran before: the host's tuples, no device pointer left over
                assert (rep["path"], rep["fallback_reason"], text_rep["tuples_from_device"]) == (0, R.NONE, 0)
                assert q.report().num_kernels == kernels0
                continue
            assert (rep["path"], rep["fallback_reason"], rep["sorted_on_host"]) == (path, reason, sorted_on_host), (sql, rep)
            assert q.report().num_kernels == kernels0 + path          # one launch packs all rows
            assert text_rep["tuples_from_device"] == (1 if path == 1 and not sorted_on_host else 0)
            if text_rep["tuples_from_device"]:
                assert text_rep["upload_ms"] == 0
            if reason != R.SHAPE:
                assert (rep["rows"], rep["tuple_size"], rep["tuple_bytes"]) == (want.n_rows, want.tuple_size, want.n_rows * want.tuple_size)
            if path == 1:
                assert rep["kernel_ms"] > 0 and rep["copy_ms"] > 0 and (rep["sort_ms"] > 0) == bool(sorted_on_host)
            else:
                assert rep["kernel_ms"] == 0 and rep["copy_ms"] == 0 and rep["sort_ms"] == 0
            ol = q.order_limit_report()
            if name == "order_limit_device":
                assert (ol["path"], ol["fallback_reason"]) == (1, engine.ORDER_LIMIT_FALLBACK_NONE)
            elif name == "ties":
                assert (ol["path"], ol["fallback_reason"]) == (0, engine.ORDER_LIMIT_FALLBACK_TIES)
        if name == "filter":          # few rows, but more than host-mapped output columns hold
            assert want.n_rows == R.filter_rows(host["big"]) and want.n_rows * R.ROW_BYTES > R.MAPPED_BYTES
        elif name == "small":
            assert 0 < want.n_rows * R.ROW_BYTES <= R.MAPPED_BYTES
        elif name == "nothing":
            assert want.n_rows == 0
        elif name == "own_limit":
            assert want.n_rows == 30000
        elif name in ("all", "order", "join"):
            assert want.n_rows == R.BIG_ROWS
    finally:
        q.close()


def test_partial_execution_reports_the_shape(world):
    ctx, tabs, _ = world
    q = ctx.sql_compile("select id, g from big", [tabs["big"]])
    try:
        ctx.set_result_pack(DEVICE)
        with pytest.raises(engine.EngineError) as e:
            q.execute_partial()
        assert e.value.status == 3
        rep = q.result_pack_report()
        assert (rep["planned"], rep["path"], rep["fallback_reason"]) == (1, 0, R.SHAPE)
    finally:
        q.close()


def test_shards_of_a_multi_context_keep_the_host_merge():
    """rsq_multi_* concatenates the shards' host columns and runs one tail over them: with the setter at 1 on both shard contexts the
    shards hold their tails back (SHAPE) and the answer is the one-context answer.  A shard's statement has no report accessor: the evidence
    for SHAPE is the launch count, which a packed shard would raise by one"""
    n = 20_000
    host = tpch.synthetic_table(n, 64)

    def plan_of(t):
        p = P.Plan([t])
        return p.set_root(p.materialize(p.projection([p.attr("b"), p.attr("c"), p.as_("e", p.add(p.attr("c"), p.attr("d")))], p.scan("t"))))

    want = orc.execute(plan_of(host))
    m = engine.MultiContext([0, 0])
    try:
        shards = m.generate(engine.GEN_SYNTHETIC, n, 1.0, param=64)
        answers, kernels = [], []
        for where in (HOST, DEVICE):
            for s in m.shards:
                s.set_result_pack(where)
            q = m.compile(plan_of(tpch.synthetic_table(0, 64)), [[t] for t in shards])
            q.execute()
            answers.append(q.result())
            kernels.append(q.report()[0].num_kernels)
            q.close()
        for got in answers:
            assert got.n_rows == want.n_rows == n and got.tuples == want.tuples
        assert kernels[0] == kernels[1]
        for t in shards:
            t.close()
    finally:
        m.close()


def test_nested_loops_outer_statement_is_packed_its_inner_side_is_not():
    """a context of its own with RSQ_ENGINE_NESTED_LOOPS: the statement materialises 140 002 pairs and packs them on the device; the inner
    side is a sub-query whose own execution keeps the host path (SHAPE) - the statement's launches grow by the one pack kernel, not two"""
    ctx = engine.Context(device=0, engine_flags=engine.ENGINE_NESTED_LOOPS)
    big, dim = R.big_table(), R.dim_table()
    tabs = [ctx.table(big), ctx.table(dim)]
    try:
        q = ctx.sql_compile(R.NESTED_LOOPS_SQL, tabs)
        assert "nested-loops" in q.explain and q.result_pack_report()["planned"] == 1
        results, kernels = [], []
        for where in (HOST, HOST, DEVICE, DEVICE):
            ctx.set_result_pack(where)
            q.execute()
            res, rep = q.result(text=False), q.result_pack_report()
            results.append((res.tuples, host_text(q)))
            kernels.append(q.report().num_kernels)
            assert (rep["path"], rep["fallback_reason"], rep["rows"], rep["tuple_size"]) == (where, R.NONE, 2 * R.BIG_ROWS, 32)
            dev_text, text_rep = q.result_text(mode=engine.TEXT_DEVICE)
            assert dev_text == results[-1][1] and text_rep["tuples_from_device"] == where
        assert results[1] == results[0] and results[2] == results[0] and results[3] == results[0]
        assert kernels[2] == kernels[3] == kernels[1] + 1
        tuples = results[0][0]
        assert sorted(tuples[i:i + 32] for i in range(0, len(tuples), 32)) == R.nested_loops_rows(big, dim)
        q.close()
    finally:
        for t in tabs:
            t.close()
        ctx.close()


# ---- the device text reads the tuples where the tail left them ---------------------------------------------------------------------

def test_the_text_reads_the_pack_buffer_in_place_at_any_chunk_base(world):
    ctx, tabs, host = world
    ctx.set_result_pack(DEVICE)
    ctx.set_result_text(1)
    q = ctx.sql_compile(R.TEXT_PLAIN, [tabs["big"]])
    try:
        q.execute()
        want = host_text(q)
        assert want.count(b"\n") == R.BIG_ROWS and q.result(text=False).tuple_size == 449          # (an odd tuple size: chunk bases at odd offsets)
        for chunk_rows in (0, 1000, 777):
            got, rep = q.result_text(mode=0, chunk_rows=chunk_rows)          # mode 0: the context's setting
            assert got == want, chunk_rows
            assert (rep["path"], rep["tuples_from_device"], rep["upload_ms"], rep["rows"]) == (1, 1, 0, R.BIG_ROWS)
            if chunk_rows:
                assert rep["chunks"] == (R.BIG_ROWS + chunk_rows - 1) // chunk_rows
        got, rep = q.result_text(mode=engine.TEXT_HOST)
        assert got == want and rep["path"] == 0 and rep["tuples_from_device"] == 0
    finally:
        q.close()


def test_another_statement_in_between_leaves_the_tuples_alone(world):
    """statement A is executed, then a different large statement B on the same context, then B is destroyed and a third runs: A's device
    text, read from A's own buffer, still equals A's host text"""
    ctx, tabs, _ = world
    ctx.set_result_pack(DEVICE)
    a = ctx.sql_compile("select * from big", [tabs["big"]])
    try:
        a.execute()
        want = host_text(a)
        b = ctx.sql_compile(R.TEXT_OTHER, [tabs["big"]])
        b.execute()
        assert b.result_pack_report()["path"] == 1 and b.result(text=False).n_rows > 30000
        got, rep = a.result_text(mode=engine.TEXT_DEVICE)
        assert got == want and rep["tuples_from_device"] == 1
        b_text = host_text(b)
        assert b.result_text(mode=engine.TEXT_DEVICE)[0] == b_text
        b.close()
        c = ctx.sql_compile("select id, g, s, m from big limit 30000", [tabs["big"]])
        c.execute()
        got, rep = a.result_text(mode=engine.TEXT_DEVICE, chunk_rows=777)
        assert got == want and rep["tuples_from_device"] == 1
        c.close()
    finally:
        a.close()


# ---- the statement loop ------------------------------------------------------------------------------------------------------------

def test_tofile_under_both_setters_writes_the_defaults_file(gpu_ctx, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)                                   # tofile writes "qres.tbl" into the working directory
    files, reports = [], []
    other = engine.Context(device=0)
    try:
        other.set_result_pack(DEVICE)
        other.set_result_text(1)
        for ctx in (gpu_ctx, other):
            db = engine.Database(ctx)
            try:
                db.add_table(ctx.table(R.big_table()))
                db.execute("tofile=true")
                res = db.execute("select * from big")
                assert res.n_rows == R.BIG_ROWS
                with open("qres.tbl", "rb") as f:
                    files.append(f.read())
                reports.append((db.result_pack_report(), db.result_text_report))
                os.remove("qres.tbl")
            finally:
                db.close()
    finally:
        other.close()
    assert files[0] == files[1] and files[0].count(b"\n") == R.BIG_ROWS
    (pack0, text0), (pack1, text1) = reports
    assert (pack0["path"], text0["path"], text0["tuples_from_device"]) == (0, 0, 0)
    assert (pack1["planned"], pack1["path"], pack1["fallback_reason"], pack1["rows"]) == (1, 1, R.NONE, R.BIG_ROWS)
    assert (text1["path"], text1["tuples_from_device"], text1["upload_ms"], text1["text_bytes"]) == (1, 1, 0, len(files[1]))


def test_the_reference_answers_through_the_statement_loop(gpu_ctx):
    """what the unmodified reference answers for six plain SELECTs over the seeded tables, from Database.execute under setting 1 - packed
    on the device every time (each statement's output columns outgrow the host-mapped form)"""
    with open(os.path.join(ROOT, "tests", "golden", "result_pack_reference.json")) as f:
        gold = json.load(f)
    db = engine.Database(gpu_ctx)
    try:
        host = {k: R.GOLD_TABLES[k]() for k in gold["tables"]}
        for k in gold["tables"]:
            db.add_table(gpu_ctx.table(host[k]))
        gpu_ctx.set_result_pack(DEVICE)
        for case in gold["cases"]:
            got = db.execute(case["sql"])
            rep = db.result_pack_report()
            assert got.text == case["result"] and got.n_rows == case["rows"], case["sql"]
            assert (rep["planned"], rep["path"], rep["fallback_reason"], rep["rows"]) == (1, 1, R.NONE, case["rows"]), (case["sql"], rep)
            assert rep["sorted_on_host"] == (1 if "order by" in case["sql"] else 0)
        gpu_ctx.set_result_pack(HOST)
        got = db.execute(gold["cases"][0]["sql"])
        assert got.text == gold["cases"][0]["result"] and db.result_pack_report()["path"] == 0
    finally:
        db.close()
