"""The device tail of a materialisation, the parts that need no device: the bytes of a tuple's field (resql_amd/csrc/result_pack.h) against
columnsToTuples over a zeroed buffer, and the decision whether a relation fits the device path, under the address and undefined-behaviour
sanitizers through a C++ driver built with g++ (tests/cpp/result_pack_test.cpp); the setter (rsq_ctx_set_result_pack) and the report's
struct_size; and `planned`, which a compile-only context knows for every shape (tests/resultpackcases.py PLANNED).  The oracle against
what the unmodified reference answers for plain SELECTs of the eligible shape (tests/golden/result_pack_reference.json)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from resql_amd import engine, plan as P, tpch_full
from oracle import orc

import resultpackcases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "result_pack_reference.json")) as f:
    GOLD = json.load(f)


def test_fields_and_fit_under_sanitizers(tmp_path):
    exe = str(tmp_path / "result_pack_test")
    src = os.path.join(ROOT, "resql_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + src, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "result_pack_test.cpp"),
                           os.path.join(src, "hostref.cpp"), os.path.join(src, "hostpar.cpp"), os.path.join(src, "expr.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "result_pack_test ok" in out.stdout


@pytest.fixture(scope="module")
def world():
    ctx = engine.Context(device=-1)
    tabs = [ctx.table(R.big_table(300)), ctx.table(R.dim_table())]
    yield ctx, tabs
    for t in tabs:
        t.close()
    ctx.close()


def test_setter_is_validated(world):
    ctx, _ = world
    for bad in (2, -1, 7):
        with pytest.raises(engine.EngineError) as e:
            ctx.set_result_pack(bad)
        assert e.value.status == 1 and "result_pack" in str(e.value)
    ctx.set_result_pack(engine.RESULT_PACK_DEVICE)
    ctx.set_result_pack(engine.RESULT_PACK_HOST)
    assert (engine.RESULT_PACK_HOST, engine.RESULT_PACK_DEVICE) == (0, 1)
    assert engine.lib().rsq_ctx_set_result_pack(None, 0) == 1


def test_report_struct_size(world):
    ctx, tabs = world
    L = engine.lib()
    full = C.sizeof(engine.rsq_result_pack_report)
    assert full == 64
    q = ctx.sql_compile("select id, g from big order by g desc, id", tabs)
    try:
        buf = (C.c_uint8 * full)(*([0xEE] * full))
        as_report = C.cast(buf, C.POINTER(engine.rsq_result_pack_report))
        C.cast(buf, C.POINTER(C.c_uint32))[0] = 4          # refused: not even `planned` fits
        assert L.rsq_query_result_pack_report(q.h, as_report) == 1
        assert "rsq_result_pack_report.struct_size" in L.rsq_last_error(ctx.h).decode()
        assert bytes(buf)[4:] == b"\xee" * (full - 4)
        C.cast(buf, C.POINTER(C.c_uint32))[0] = 20         # up to and including `sorted_on_host`
        assert L.rsq_query_result_pack_report(q.h, as_report) == 0
        raw = bytes(buf)
        assert raw[20:] == b"\xee" * (full - 20)
        #                                                      size planned path reason sorted
        assert np.frombuffer(raw[:20], dtype=np.int32).tolist() == [20, 1, 0, R.NONE, 0]
        C.cast(buf, C.POINTER(C.c_uint32))[0] = 5000
        assert L.rsq_query_result_pack_report(q.h, as_report) == 1
        assert L.rsq_query_result_pack_report(q.h, None) == 1 and L.rsq_query_result_pack_report(None, as_report) == 1
        assert q.result_pack_report() == {"planned": 1, "path": 0, "fallback_reason": R.NONE, "sorted_on_host": 0, "tuple_size": 0, "rows": 0,
                                          "tuple_bytes": 0, "kernel_ms": 0.0, "copy_ms": 0.0, "sort_ms": 0.0}
    finally:
        q.close()
    # the statement loop's report: the same rule, before any SELECT has run
    db = engine.Database(ctx)
    try:
        buf = (C.c_uint8 * full)(*([0xEE] * full))
        as_report = C.cast(buf, C.POINTER(engine.rsq_result_pack_report))
        for size, status in ((4, 1), (7, 1), (8, 0), (4097, 1)):
            C.cast(buf, C.POINTER(C.c_uint32))[0] = size
            assert L.rsq_db_result_pack_report(db.h, as_report) == status, size
        assert bytes(buf)[8:] == b"\xee" * (full - 8)
        assert db.result_pack_report()["planned"] == 0
    finally:
        db.close()


@pytest.mark.parametrize("sql,planned", R.PLANNED)
def test_planned_is_known_after_compile(world, sql, planned):
    ctx, tabs = world
    q = ctx.sql_compile(sql, tabs)
    try:
        rep = q.result_pack_report()
        assert rep["planned"] == planned, sql
        assert rep["path"] == 0 and rep["fallback_reason"] == R.NONE and rep["rows"] == 0          # nothing has executed
    finally:
        q.close()


def test_more_than_64_materialised_columns_are_not_planned():
    ctx = engine.Context(device=-1)
    try:
        for n_cols, planned in ((64, 1), (65, 0)):
            host = P.Table("t", [P.Column(f"c{i}", P.TypeInit.INT(), np.arange(10, dtype=np.int32) + i) for i in range(n_cols)], 10)
            t = ctx.table(host)
            q = ctx.sql_compile("select * from t", [t])
            assert q.result_pack_report()["planned"] == planned, n_cols
            q.close()
            t.close()
    finally:
        ctx.close()


def test_nested_loops_statement_is_planned():
    """the statement around a nested-loops join materialises the pairs: of the shape.  Its inner side is a query of its own, which the
    execution marks as a sub-query (tests/test_gpu_result_pack.py)"""
    ctx = engine.Context(device=-1, engine_flags=engine.ENGINE_NESTED_LOOPS)
    db = tpch_full.database(0.01)
    tabs = [ctx.table(db[k]) for k in sorted(db)]
    try:
        q = ctx.sql_compile("select r_name, n_nationkey from region, nation where n_nationkey < 6", tabs)
        assert "nested-loops" in q.explain and q.result_pack_report()["planned"] == 1
        q.close()
    finally:
        for t in tabs:
            t.close()
        ctx.close()


def test_exported_and_bound():
    names = {"rsq_ctx_set_result_pack", "rsq_query_result_pack_report", "rsq_db_result_pack_report", "rsq_prim_pack_tuples"}
    assert names <= set(engine.EXPORTED_SYMBOLS)
    L = engine.lib()
    for name in names:
        assert hasattr(L, name)
    with open(os.path.join(ROOT, "integration", "resql_hip_binding.h")) as f:
        assert "void setResultPack(int where) { check(rsq_ctx_set_result_pack(ctx_, where)); }" in f.read()


def test_primitive_refuses_what_its_kernel_would_not_bound(world):
    ctx, _ = world
    with pytest.raises(engine.EngineError) as e:          # a compile-only context
        ctx.prim_pack_tuples([np.arange(8, dtype=np.int32)], [P.TypeInit.INT()])
    assert e.value.status == 3
    L = engine.lib()
    col = np.arange(8, dtype=np.int32)
    out = np.zeros(8 * 4 + 64, dtype=np.uint8)
    ptrs = (C.c_void_p * 1)(col.ctypes.data)
    types = (P.rsq_type * 1)(P.TypeInit.INT().c())

    def call(n_cols=1, n_rows=8, columns=ptrs, out_ptr=out.ctypes.data):
        return L.rsq_prim_pack_tuples(ctx.h, columns, types, n_cols, n_rows, out_ptr, len(out))
    for kw in ({"n_cols": 0}, {"n_cols": 65}, {"n_rows": -1}, {"n_rows": 1 << 31}, {"columns": None}, {"out_ptr": None},
               {"columns": (C.c_void_p * 1)(None)}):
        assert call(**kw) == 1, kw


# ---- the oracle against the unmodified reference's answers ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gold_world():
    ctx = engine.Context(device=-1)
    host = [R.GOLD_TABLES[k]() for k in GOLD["tables"]]
    tabs = [ctx.table(t) for t in host]
    yield ctx, tabs, host
    for t in tabs:
        t.close()
    ctx.close()


def test_the_recorded_cases_cover_what_they_should():
    sqls = [c["sql"] for c in GOLD["cases"]]
    assert sqls == R.GOLD_STATEMENTS and len(sqls) == 6
    assert sqls[0] == "select * from gold" and {str(c.type) for c in R.gold_table(1).columns} >= {"INT", "BIGINT", "DATE", "BOOL", "CHAR(1)", "CHAR(10)", "VARCHAR(12)", "DECIMAL(15,2)"}
    assert " where f < 90" in sqls[1] and "order by" in sqls[2] and "limit" not in sqls[2]
    assert "order by" in sqls[3] and "limit 20" in sqls[3] and "order by" not in sqls[4] and "limit 70" in sqls[4] and "gold, gdim" in sqls[5]


@pytest.mark.parametrize("case", GOLD["cases"], ids=[str(i) for i in range(len(GOLD["cases"]))])
def test_oracle_equals_the_reference_on_eligible_statements(gold_world, case):
    ctx, tabs, host = gold_world
    q = ctx.sql_compile(case["sql"], tabs)
    try:
        assert q.result_pack_report()["planned"] == 1, case["sql"]
    finally:
        q.close()
    want = orc.execute(ctx.sql_plan(case["sql"], tabs, host))
    assert want.n_rows == case["rows"] and want.text == case["result"], case["sql"]
