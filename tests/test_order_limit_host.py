"""ORDER BY ... LIMIT over a materialisation, the parts that need no device: the image of a first sort key and the loop that packs
columns into tuples (resql_amd/csrc/order_limit.h) under the address and undefined-behaviour sanitizers, through a C++ driver built with
g++ (tests/cpp/order_limit_test.cpp); the setter (rsq_ctx_set_order_limit) and the report's struct_size; and `planned`, which a
compile-only context knows for every shape the rule names (tests/orderlimitcases.py PLANNED).  The oracle against what the unmodified
reference answers for statements of the eligible shape (tests/golden/order_limit_reference.json)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from resql_amd import engine, plan as P, tpch_full
from oracle import orc

import orderlimitcases as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "order_limit_reference.json")) as f:
    GOLD = json.load(f)


def test_image_and_tuple_loop_under_sanitizers(tmp_path):
    exe = str(tmp_path / "order_limit_test")
    src = os.path.join(ROOT, "resql_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + src, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "order_limit_test.cpp"),
                           os.path.join(src, "hostref.cpp"), os.path.join(src, "hostpar.cpp"), os.path.join(src, "expr.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "order_limit_test ok" in out.stdout


@pytest.fixture(scope="module")
def shapes():
    ctx = engine.Context(device=-1)
    t = ctx.table(O.shape_table())
    yield ctx, t
    t.close()
    ctx.close()


def test_setter_is_validated(shapes):
    ctx, _ = shapes
    for bad in (2, -1, 7):
        with pytest.raises(engine.EngineError) as e:
            ctx.set_order_limit(bad)
        assert e.value.status == 1 and "order_limit" in str(e.value)
    ctx.set_order_limit(engine.ORDER_LIMIT_DEVICE)
    ctx.set_order_limit(engine.ORDER_LIMIT_HOST)
    assert engine.lib().rsq_ctx_set_order_limit(None, 0) == 1


def test_report_struct_size(shapes):
    ctx, t = shapes
    L = engine.lib()
    full = C.sizeof(engine.rsq_order_limit_report)
    assert full == 88
    q = ctx.sql_compile("select i, g from shapes order by g desc, i limit 10", [t])
    try:
        buf = (C.c_uint8 * full)(*([0xEE] * full))
        as_report = C.cast(buf, C.POINTER(engine.rsq_order_limit_report))
        C.cast(buf, C.POINTER(C.c_uint32))[0] = 4          # refused: not even `planned` fits
        assert L.rsq_query_order_limit_report(q.h, as_report) == 1
        assert "rsq_order_limit_report.struct_size" in L.rsq_last_error(ctx.h).decode()
        assert bytes(buf)[4:] == b"\xee" * (full - 4)
        C.cast(buf, C.POINTER(C.c_uint32))[0] = 28         # up to and including `descending`
        assert L.rsq_query_order_limit_report(q.h, as_report) == 0
        raw = bytes(buf)
        assert raw[28:] == b"\xee" * (full - 28)
        #                                                      size planned path reason column is32 descending
        assert np.frombuffer(raw[:28], dtype=np.int32).tolist() == [28, 1, 0, O.NONE, 1, 0, 1]
        C.cast(buf, C.POINTER(C.c_uint32))[0] = 5000
        assert L.rsq_query_order_limit_report(q.h, as_report) == 1
        assert L.rsq_query_order_limit_report(q.h, None) == 1 and L.rsq_query_order_limit_report(None, as_report) == 1
        rep = q.order_limit_report()
        assert rep == {"planned": 1, "path": 0, "fallback_reason": O.NONE, "first_key_column": 1, "key_is32": 0, "descending": 1, "rows": 0, "want": 0,
                       "candidates": 0, "capacity": 0, "select_ms": 0.0, "copy_ms": 0.0, "tail_ms": 0.0}
    finally:
        q.close()


@pytest.mark.parametrize("sql,planned", O.PLANNED)
def test_planned_is_known_after_compile(shapes, sql, planned):
    ctx, t = shapes
    q = ctx.sql_compile(sql, [t])
    try:
        rep = q.order_limit_report()
        assert rep["planned"] == planned, sql
        assert rep["path"] == 0 and rep["fallback_reason"] == O.NONE          # nothing has executed
        if planned:
            names = [c.split(":")[0] for c in orc.execute(ctx.sql_plan(sql, [t], [O.shape_table()])).text.splitlines()[0][len("#schema "):].split("|") if c]
            first = sql.split("order by ")[1].split()[0].rstrip(",")
            assert names[rep["first_key_column"]] == first
            assert rep["key_is32"] == (1 if first == "dt" else 0) and rep["descending"] == (1 if " %s desc" % first in sql else 0)
        else:
            assert rep["first_key_column"] == -1
    finally:
        q.close()


def test_a_first_key_the_materialisation_does_not_hold_keeps_the_reference_error(shapes):
    """`order by` names an attribute the select list drops: not planned, and the tail's "Order By attribute not found." stays where it is
    raised today (at the execution's tail - there is no device here to reach it)"""
    ctx, t = shapes
    p = P.Plan([O.shape_table()])
    mat = p.materialize(p.projection([p.attr("i")], p.scan("shapes")))
    p.set_root(p.orderby([p.asc(p.attr("g"))], mat), limit=5)
    q = ctx.compile(p, [t])
    try:
        assert q.order_limit_report()["planned"] == 0
    finally:
        q.close()


def test_nested_loops_inner_side_and_the_statement_around_it():
    """A nested-loops join's inner side is a query of its own under a MATERIALIZE root, which carries no ORDER BY - never of the shape
    (a plan description puts its one LIMIT on the root, so a materialisation below an ORDER BY has none of its own either); the statement
    around it, whose last pipeline materialises the pairs, is of the shape"""
    ctx = engine.Context(device=-1, engine_flags=engine.ENGINE_NESTED_LOOPS)
    db = tpch_full.database(0.01)
    tabs = [ctx.table(db[k]) for k in sorted(db)]
    try:
        q = ctx.sql_compile("select r_name, n_nationkey from region, nation where n_nationkey < 6 order by n_nationkey desc, r_name limit 3", tabs)
        rep = q.order_limit_report()
        assert "nested-loops" in q.explain and rep["planned"] == 1 and rep["key_is32"] == 1 and rep["descending"] == 1
        q.close()
    finally:
        for t in tabs:
            t.close()
        ctx.close()


def test_exported_and_bound():
    assert {"rsq_ctx_set_order_limit", "rsq_query_order_limit_report", "rsq_db_order_limit_report", "rsq_prim_column_topk"} <= set(engine.EXPORTED_SYMBOLS)
    L = engine.lib()
    for name in ("rsq_ctx_set_order_limit", "rsq_query_order_limit_report", "rsq_db_order_limit_report", "rsq_prim_column_topk"):
        assert hasattr(L, name)
    with open(os.path.join(ROOT, "integration", "resql_hip_binding.h")) as f:
        assert "void setOrderLimit(int where) { check(rsq_ctx_set_order_limit(ctx_, where)); }" in f.read()


def test_primitive_refuses_what_its_kernels_would_not_bound(shapes):
    ctx, _ = shapes
    key = np.arange(8, dtype=np.int64)
    pay = np.zeros((8, 3), dtype=np.uint8)
    with pytest.raises(engine.EngineError) as e:          # a compile-only context
        ctx.prim_column_topk(key, True, 1, 4, pay)
    assert e.value.status == 3
    L = engine.lib()
    pos, out = np.zeros(4, dtype=np.uint32), np.zeros((4, 3), dtype=np.uint8)
    cnt, thr, notes = C.c_uint64(), C.c_uint64(), C.c_uint32()

    def call(key_width=8, n=8, want=1, capacity=4, width=3):
        return L.rsq_prim_column_topk(ctx.h, key.ctypes.data, key_width, n, 1, want, capacity, pay.ctypes.data, width, pos.ctypes.data, out.ctypes.data,
                                      C.addressof(cnt), C.addressof(thr), C.addressof(notes))
    for kw in ({"key_width": 2}, {"key_width": 16}, {"n": -1}, {"n": 1 << 32}, {"want": 0}, {"want": 1 << 32}, {"capacity": 0}, {"capacity": 1 << 31},
               {"width": 0}, {"width": 4097}):
        assert call(**kw) == 1, kw


# ---- the oracle against the unmodified reference's answers ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tpch():
    ctx = engine.Context(device=-1)
    db = tpch_full.database(GOLD["sf"])
    host = [db[k] for k in GOLD["tables"]]
    tabs = [ctx.table(t) for t in host]
    yield ctx, tabs, host
    for t in tabs:
        t.close()
    ctx.close()


@pytest.mark.parametrize("case", GOLD["cases"], ids=[str(i) for i in range(len(GOLD["cases"]))])
def test_oracle_equals_the_reference_on_eligible_statements(tpch, case):
    ctx, tabs, host = tpch
    q = ctx.sql_compile(case["sql"], tabs)
    try:
        assert q.order_limit_report()["planned"] == 1, case["sql"]
    finally:
        q.close()
    assert orc.execute(ctx.sql_plan(case["sql"], tabs, host)).text == case["result"], case["sql"]
