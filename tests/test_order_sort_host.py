"""ORDER BY over a materialisation sorted on the device, the parts that need no device: the image of a key cell, the layout of the
composite key, its words against compareTyped and the decision whether an execution's buffers fit (resql_amd/csrc/order_sort.h), under the
address and undefined-behaviour sanitizers through a C++ driver built with g++ (tests/cpp/order_sort_test.cpp); the setter
(rsq_ctx_set_order_sort) and the report's struct_size; and `planned`, which a compile-only context knows for every shape
(tests/ordersortcases.py PLANNED).  The oracle against what the unmodified reference answers for statements of the eligible shape
(tests/golden/order_sort_reference.json)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from resql_amd import engine, plan as P, tpch_full
from oracle import orc

import ordersortcases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "order_sort_reference.json")) as f:
    GOLD = json.load(f)


def test_images_layouts_words_and_fit_under_sanitizers(tmp_path):
    exe = str(tmp_path / "order_sort_test")
    src = os.path.join(ROOT, "resql_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + src, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "order_sort_test.cpp"),
                           os.path.join(src, "hostref.cpp"), os.path.join(src, "hostpar.cpp"), os.path.join(src, "expr.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "order_sort_test ok" in out.stdout


@pytest.fixture(scope="module")
def world():
    ctx = engine.Context(device=-1)
    tabs = [ctx.table(S.TABLES["shapes"]())]
    yield ctx, tabs
    for t in tabs:
        t.close()
    ctx.close()


def test_setter_is_validated(world):
    ctx, _ = world
    for bad in (2, -1, 7):
        with pytest.raises(engine.EngineError) as e:
            ctx.set_order_sort(bad)
        assert e.value.status == 1 and "order_sort" in str(e.value)
    ctx.set_order_sort(engine.ORDER_SORT_DEVICE)
    ctx.set_order_sort(engine.ORDER_SORT_HOST)
    assert (engine.ORDER_SORT_HOST, engine.ORDER_SORT_DEVICE) == (0, 1)
    assert (S.NONE, S.SHAPE, S.SMALL, S.DOES_NOT_FIT, S.TIES, S.ORDER_LIMIT) == (0, 1, 2, 3, 4, 5)
    assert engine.lib().rsq_ctx_set_order_sort(None, 0) == 1


def test_report_struct_size(world):
    ctx, tabs = world
    L = engine.lib()
    full = C.sizeof(engine.rsq_order_sort_report)
    assert full == 144
    q = ctx.sql_compile("select i, g from shapes order by g desc, i", tabs)
    try:
        buf = (C.c_uint8 * full)(*([0xEE] * full))
        as_report = C.cast(buf, C.POINTER(engine.rsq_order_sort_report))
        C.cast(buf, C.POINTER(C.c_uint32))[0] = 4          # refused: not even `planned` fits
        assert L.rsq_query_order_sort_report(q.h, as_report) == 1
        assert "rsq_order_sort_report.struct_size" in L.rsq_last_error(ctx.h).decode()
        assert bytes(buf)[4:] == b"\xee" * (full - 4)
        C.cast(buf, C.POINTER(C.c_uint32))[0] = 20         # up to and including `keys`
        assert L.rsq_query_order_sort_report(q.h, as_report) == 0
        raw = bytes(buf)
        assert raw[20:] == b"\xee" * (full - 20)
        #                                                      size planned path reason keys
        assert np.frombuffer(raw[:20], dtype=np.int32).tolist() == [20, 1, 0, S.NONE, 2]
        C.cast(buf, C.POINTER(C.c_uint32))[0] = 5000
        assert L.rsq_query_order_sort_report(q.h, as_report) == 1
        assert L.rsq_query_order_sort_report(q.h, None) == 1 and L.rsq_query_order_sort_report(None, as_report) == 1
        assert q.order_sort_report() == {"planned": 1, "path": 0, "fallback_reason": S.NONE, "keys": 2, "key_bits": [0] * 8, "total_bits": 0, "words": 0,
                                         "passes": 0, "tuple_size": 0, "rows": 0, "lead": 0, "out_rows": 0, "tied_pairs": 0, "range_ms": 0.0,
                                         "sort_ms": 0.0, "pack_ms": 0.0, "gather_ms": 0.0, "copy_ms": 0.0}
    finally:
        q.close()
    # the statement loop's report: the same rule, before any SELECT has run
    db = engine.Database(ctx)
    try:
        buf = (C.c_uint8 * full)(*([0xEE] * full))
        as_report = C.cast(buf, C.POINTER(engine.rsq_order_sort_report))
        for size, status in ((4, 1), (7, 1), (8, 0), (4097, 1)):
            C.cast(buf, C.POINTER(C.c_uint32))[0] = size
            assert L.rsq_db_order_sort_report(db.h, as_report) == status, size
        assert bytes(buf)[8:] == b"\xee" * (full - 8)
        assert db.order_sort_report()["planned"] == 0
    finally:
        db.close()


@pytest.mark.parametrize("sql,planned,keys", S.PLANNED)
def test_planned_is_known_after_compile(world, sql, planned, keys):
    ctx, tabs = world
    q = ctx.sql_compile(sql, tabs)
    try:
        rep = q.order_sort_report()
        assert (rep["planned"], rep["keys"]) == (planned, keys), sql
        assert rep["path"] == 0 and rep["fallback_reason"] == S.NONE and rep["rows"] == 0          # nothing has executed
    finally:
        q.close()


def test_the_planned_cases_cover_the_rule():
    sqls = {sql: planned for sql, planned, _ in S.PLANNED}
    assert sqls["select i, g from shapes order by g desc, i"] == 1 and sqls["select i, m from shapes order by m, i limit 0"] == 1
    assert sqls["select i, dt from shapes order by dt, i limit %d" % (2**20 + 1)] == 1
    assert sorted(keys for _, planned, keys in S.PLANNED if planned)[-1] == 8
    nine = [sql for sql in sqls if " order by " in sql and sql.split(" order by ")[1].count(",") == 8]
    assert len(nine) == 1 and sqls[nine[0]] == 0
    for key in ("s", "w", "o", "c"):          # a string, BOOL or CHAR(1) key in first and in later position
        assert sqls["select %s, i from shapes order by %s, i" % (key, key)] == 0 and sqls["select i, %s from shapes order by i, %s" % (key, key)] == 0
    assert any("group by" in sql and not planned for sql, planned in sqls.items())
    assert any(" as x" in sql and planned for sql, planned in sqls.items())


def test_exported_and_bound():
    names = {"rsq_ctx_set_order_sort", "rsq_query_order_sort_report", "rsq_db_order_sort_report", "rsq_prim_sort_rows", "rsq_prim_gather_tuples"}
    assert names <= set(engine.EXPORTED_SYMBOLS)
    L = engine.lib()
    for name in names:
        assert hasattr(L, name)
    with open(os.path.join(ROOT, "integration", "resql_hip_binding.h")) as f:
        assert "void setOrderSort(int where) { check(rsq_ctx_set_order_sort(ctx_, where)); }" in f.read()


def test_primitives_refuse_what_their_kernels_would_not_bound(world):
    ctx, _ = world
    with pytest.raises(engine.EngineError) as e:          # a compile-only context
        ctx.prim_sort_rows([np.arange(8, dtype=np.int32)], [P.TypeInit.INT()], [0], [False])
    assert e.value.status == 3
    with pytest.raises(engine.EngineError) as e:
        ctx.prim_gather_tuples(np.zeros(32, dtype=np.uint8), 4, np.arange(8, dtype=np.uint32), 8)
    assert e.value.status == 3
    L = engine.lib()
    col = np.arange(8, dtype=np.int32)
    perm = np.zeros(8, dtype=np.uint32)
    ptrs = (C.c_void_p * 1)(col.ctypes.data)
    types = (P.rsq_type * 1)(P.TypeInit.INT().c())
    ties, words, bits = C.c_int64(0), C.c_int32(0), (C.c_int32 * 8)()

    def sort(n_cols=1, key=0, n_keys=1, n_rows=8, lead=8, out=perm.ctypes.data):
        return L.rsq_prim_sort_rows(ctx.h, ptrs, types, n_cols, (C.c_int32 * 9)(*([key] * 9)), (C.c_int32 * 9)(), n_keys, n_rows, lead, out,
                                    C.addressof(ties), C.addressof(bits), C.addressof(words))
    for kw in ({"n_cols": 0}, {"key": 1}, {"key": -1}, {"n_keys": 0}, {"n_keys": 9}, {"n_rows": -1}, {"n_rows": 1 << 31}, {"lead": 9}, {"lead": -1}, {"out": None}):
        assert sort(**kw) == 1, kw
    tuples = np.zeros(32, dtype=np.uint8)
    out = np.zeros(32 + 64, dtype=np.uint8)

    def gather(ts=4, n_rows=8, n_out=8, perm_ptr=perm.ctypes.data):
        return L.rsq_prim_gather_tuples(ctx.h, tuples.ctypes.data, ts, n_rows, perm_ptr, n_out, out.ctypes.data, len(out))
    for kw in ({"ts": 0}, {"n_rows": -1}, {"n_out": 9}, {"n_out": -1}, {"perm_ptr": None}):
        assert gather(**kw) == 1, kw
    perm[3] = 8          # a row the tuples do not hold
    assert gather() == 1
    perm[3] = 0


# ---- the oracle against the unmodified reference's answers ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gold_world():
    ctx = engine.Context(device=-1)
    db = tpch_full.database(GOLD["sf"])
    host = [db[k] for k in GOLD["tables"]]
    tabs = [ctx.table(t) for t in host]
    yield ctx, tabs, host
    for t in tabs:
        t.close()
    ctx.close()


def test_the_recorded_cases_are_the_statement_list():
    assert [c["sql"] for c in GOLD["cases"]] == S.GOLD_STATEMENTS and GOLD["sf"] == S.GOLD_SF and len(S.GOLD_STATEMENTS) == 6
    assert sum(" limit " not in sql for sql in S.GOLD_STATEMENTS) == 3 and any(" where " in sql for sql in S.GOLD_STATEMENTS)
    assert any("limit 2000000" in sql for sql in S.GOLD_STATEMENTS) and any(" as revenue" in sql for sql in S.GOLD_STATEMENTS)


@pytest.mark.parametrize("case", GOLD["cases"], ids=[str(i) for i in range(len(GOLD["cases"]))])
def test_oracle_equals_the_reference_on_eligible_statements(gold_world, case):
    ctx, tabs, host = gold_world
    q = ctx.sql_compile(case["sql"], tabs)
    try:
        assert q.order_sort_report()["planned"] == 1, case["sql"]
    finally:
        q.close()
    want = orc.execute(ctx.sql_plan(case["sql"], tabs, host))
    assert want.n_rows == case["rows"] and S.gold_matches(case, want.text), case["sql"]
