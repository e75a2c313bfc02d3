"""GROUP BY over a dictionary-coded string from a join's build side on the GPU (RSQ_DICT_SCANS=2): the payload word is an address inside
the origin column's dictionary image, and the group's dense rank is (address - dictionary) / width.  Every statement is answered three
ways by one context - under RSQ_DICT_SCANS=2 (dense, executed twice: the table is put back to its identities in between), =1 (coded
scans, hash aggregation) and =0 (wide scans) - and all three are the oracle's answer, text and tuples, emission order included.
The probe side has dictgroupcases.ROWS rows, build sides a few hundred."""
import os
import re
import sys

import numpy as np
import pytest

from resql_amd import engine, plan as P, tpch_full
from oracle import orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dictcases as D  # noqa: E402
import dictgroupcases as G  # noqa: E402
import dictjoincases as J  # noqa: E402

pytestmark = pytest.mark.gpu
T = P.TypeInit
OF = J.NOTE + " of "
IN_PLACE = "the build table's own columns"


@pytest.fixture(scope="module", autouse=True)
def _join_keys_on():
    """the images are opt-in (read when a table is created and when a statement is compiled): on for this module's tables"""
    old = os.environ.get("RSQ_DICT_SCANS")
    os.environ["RSQ_DICT_SCANS"] = "2"
    yield
    if old is None:
        os.environ.pop("RSQ_DICT_SCANS", None)
    else:
        os.environ["RSQ_DICT_SCANS"] = old


def _run(ctx, stmt, tabs, want, executions=1):
    q = ctx.sql_compile(stmt, tabs) if isinstance(stmt, str) else ctx.compile(stmt, tabs)
    try:
        for _ in range(executions):
            q.execute()
            got = q.result()
            assert got.text == want.text and got.tuples == want.tuples, stmt
        return q.source, q.explain, got
    finally:
        q.close()


def _check(ctx, monkeypatch, stmt, host, tabs=None, dense=True, env=None):
    """the statement (SQL text or a plan) under RSQ_DICT_SCANS=2 and `env`, twice; then under 1 and under 0; all against the oracle.
    Returns the first run's (source, explain after its executions, answer)"""
    own = tabs is None
    if own:
        tabs = [ctx.table(t) for t in host]
    try:
        want = orc.execute(ctx.sql_plan(stmt, tabs, host) if isinstance(stmt, str) else stmt)
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        src, ex, got = _run(ctx, stmt, tabs, want, executions=2)
        for k in (env or {}):
            monkeypatch.delenv(k)
        assert (OF in ex) == dense, ex
        if dense:
            assert "aggregation dense" in ex and re.search(r"const u64 r = dict_rank<\d+>\(\w+, a\.gd\d+\);", src)
        monkeypatch.setenv("RSQ_DICT_SCANS", "1")
        s1, e1, _ = _run(ctx, stmt, tabs, want)
        assert "dict_rank" not in s1 and OF not in e1
        monkeypatch.setenv("RSQ_DICT_SCANS", "0")
        s0, e0, _ = _run(ctx, stmt, tabs, want)
        assert "vc_" not in s0 and J.NOTE not in e0
        monkeypatch.setenv("RSQ_DICT_SCANS", "2")
        return src, ex, got
    finally:
        if own:
            for t in tabs:
                t.close()


@pytest.fixture(scope="module")
def std_tables(gpu_ctx):
    host = list(J.tables())
    devs = [gpu_ctx.table(t) for t in host]
    yield host, devs
    for d in devs:
        d.close()


@pytest.mark.parametrize("kind", ["CHAR", "VARCHAR"])
def test_built_table(gpu_ctx, monkeypatch, kind):
    """(a) r's keys are scattered: the table is built, and the address it stores points into the image.  'liamm' / 'mmail' collide in
    Values::hash, so the emission order is exercised"""
    src, ex, got = _check(gpu_ctx, monkeypatch, J.JOIN_PAYLOAD, list(J.tables(getattr(T, kind)(6))))
    assert "aggregation dense groups=4 " in ex and "in workgroup LDS table" in ex and IN_PLACE not in ex and got.n_rows == 4


def test_direct_table(gpu_ctx, monkeypatch):
    """(b) r's keys are 0..n-1 in row order: the probe reads r in place, the code column and the dictionary instead of the wide column;
    with RSQ_JOIN_RANK=0 the same statement builds a hash table"""
    host = list(J.tables(keys=np.arange(600)))
    tabs = [gpu_ctx.table(t) for t in host]
    try:
        src, ex, _ = _check(gpu_ctx, monkeypatch, J.JOIN_PAYLOAD, host, tabs)
        assert IN_PLACE in ex and "a.ht0_dict1 + (u32)a.ht0_code1[ht0_s] * 6u" in src
        src, ex, _ = _check(gpu_ctx, monkeypatch, J.JOIN_PAYLOAD, host, tabs, env={"RSQ_JOIN_RANK": "0"})
        assert IN_PLACE not in ex and "ht0_code1" not in src
    finally:
        for t in tabs:
            t.close()


def test_two_hops(gpu_ctx, monkeypatch):
    """(c) 25 CHAR(25) names -> a 300-row table that carries the name's address on -> the probe of t, grouped by the name"""
    plan = J.two_hop_plan()
    src, ex, got = _check(gpu_ctx, monkeypatch, plan, list(plan.tables))
    assert "key nname by dictionary code of n.nname (25 entries)" in ex and re.search(r"dict_rank<25>\(ht1_v\d+, a\.gd0\)", src)
    assert IN_PLACE in ex                                                 # (m's probe of n reads n in place: the direct form feeds the carry)


def test_q5(gpu_ctx, monkeypatch):
    """(c) TPC-H Q5 at the scale of the codegen test: n_name goes nation -> the supplier's table -> lineitem's probe"""
    db = tpch_full.database(0.01)
    host = [db[k] for k in sorted(db)]
    src, ex, got = _check(gpu_ctx, monkeypatch, tpch_full.QUERIES["q5"], host)
    assert "aggregation dense groups=25 " in ex and "key n_name by dictionary code of nation.n_name (25 entries)" in ex


def test_q10_keeps_the_hash_form_and_reads_n_name_through_the_dictionary(gpu_ctx, monkeypatch):
    """Q10 groups by c_custkey and six values that hang off it: a hash aggregation under every switch.  Under 2 its n_name has an origin, so
    the probe of nation reads the code column and the dictionary in place, and the group rows are rebuilt from that address"""
    db = tpch_full.database(0.01)
    host = [db[k] for k in sorted(db)]
    src, ex, got = _check(gpu_ctx, monkeypatch, tpch_full.QUERIES["q10"], host, dense=False)
    assert "hash aggregation" in ex and re.search(r"a\.ht\d+_dict\d+ \+ \(u32\)a\.ht\d+_code\d+\[ht\d+_s\] \* 25u", src)


@pytest.mark.parametrize("count", [1, 2, 256, 257])
def test_build_side_dictionary_sizes(gpu_ctx, monkeypatch, count):
    """(d)"""
    src, ex, got = _check(gpu_ctx, monkeypatch, J.JOIN_PAYLOAD, list(J.tables(T.VARCHAR(9), G.values(count))), dense=count <= 256)
    assert got.n_rows == count
    if count <= 256:
        assert f"aggregation dense groups={count} " in ex
    else:
        assert "hash aggregation" in ex and "its bytes do not stand in a dictionary image" in ex      # 257 values: no image, still right


@pytest.mark.parametrize("kind", ["CHAR", "VARCHAR"])
def test_edge_values_as_the_build_column(gpu_ctx, monkeypatch, kind):
    """(e) 'ab' against 'ab ' (one group to CHAR, with the spelling of the first row; two to VARCHAR), the empty value, full-width values"""
    src, ex, got = _check(gpu_ctx, monkeypatch, J.JOIN_PAYLOAD, list(J.tables(getattr(T, kind)(9), D.edge_values(9, 12))))
    assert "aggregation dense groups=12 " in ex and got.n_rows == (11 if kind == "CHAR" else 12)


def test_mixed_keys_in_lds(gpu_ctx, monkeypatch, std_tables):
    """(f) a build-side coded key, a scan-own coded key and a byte set"""
    host, devs = std_tables
    src, ex, _ = _check(gpu_ctx, monkeypatch, J.MIXED, host, devs)
    assert f"aggregation dense groups={4 * 12 * 3} " in ex and "key ru by dictionary code of r.ru (4 entries), key s by dictionary code (12 entries)" in ex
    assert re.search(r"const int gk1 = \(int\)\(q_\d+\);", src)           # (the scan-own key's code travels in the queue as before)


@pytest.mark.parametrize("tail", [None, "1"], ids=["host_tail", "device_tail"])
def test_with_a_numeric_key_in_hbm(gpu_ctx, monkeypatch, capfd, std_tables, tail):
    """(f) 4 x 1000 cells: the HBM table; with RSQ_DEVICE_TAIL_MIN=1 the device tail makes the tuples"""
    host, devs = std_tables
    monkeypatch.setenv("RSQ_TRACE", "1")
    capfd.readouterr()
    src, ex, _ = _check(gpu_ctx, monkeypatch, J.HBM, host, devs, env={"RSQ_DEVICE_TAIL_MIN": tail} if tail else None)
    assert "aggregation dense groups=4000 " in ex and "in HBM table" in ex
    if tail:
        assert "device tail" in capfd.readouterr().err


def test_space_equivalent_entries_fold_on_the_device(gpu_ctx, monkeypatch, capfd):
    """(f) the same over CHAR(9) edge values: 'ab' and 'ab ' are two ranks and one group, folded by the device tail"""
    monkeypatch.setenv("RSQ_TRACE", "1")
    capfd.readouterr()
    src, ex, _ = _check(gpu_ctx, monkeypatch, J.HBM, list(J.tables(T.CHAR(9), D.edge_values(9, 12))), env={"RSQ_DEVICE_TAIL_MIN": "1"})
    err = capfd.readouterr().err
    assert "aggregation dense groups=12000 " in ex and "device tail" in err and "groups equal up to trailing spaces merged" in err


@pytest.mark.parametrize("mode,form", [("1", "in registers"), ("2", "in lane-private LDS"), ("3", "in workgroup LDS table")])
def test_register_and_lds_forms(gpu_ctx, monkeypatch, std_tables, mode, form):
    """(g)"""
    host, devs = std_tables
    src, ex, _ = _check(gpu_ctx, monkeypatch, J.JOIN_PAYLOAD, host, devs, env={"RSQ_AGG_MODE": mode})
    assert form in ex


def test_no_row_passes(gpu_ctx, monkeypatch, std_tables):
    """(h)"""
    host, devs = std_tables
    src, ex, got = _check(gpu_ctx, monkeypatch, J.NO_ROW, host, devs)
    assert got.n_rows == 0


def test_an_entry_no_probe_row_matches_is_no_group(gpu_ctx, monkeypatch):
    """(h) one build row's key is outside t's values and its ru occurs nowhere else: a rank of the dictionary without a group"""
    src, ex, got = _check(gpu_ctx, monkeypatch, J.JOIN_PAYLOAD, list(J.lonely_tables()))
    assert "aggregation dense groups=5 " in ex and got.n_rows == 4


@pytest.mark.parametrize("sql,form", [(J.TOP, "in workgroup LDS table"), (J.HBM_TOP, "in HBM table")], ids=["lds", "hbm"])
def test_order_by_limit_above(gpu_ctx, monkeypatch, std_tables, sql, form):
    """(i)"""
    host, devs = std_tables
    src, ex, got = _check(gpu_ctx, monkeypatch, sql, host, devs)
    assert form in ex and got.n_rows == (3 if sql == J.TOP else 10)


def test_append_to_the_origin_table_refuses_the_old_statement(gpu_ctx, monkeypatch):
    """(j) the appended value sorts in front of the old ones: r's dictionary is rebuilt and every rank moves.  The statement compiled
    before holds the old dictionary: refused, as for a scan-own key; a fresh compile sees five entries"""
    t = J.probe_side()
    a, b = J.appended_tables()
    tt, ta, tb = gpu_ctx.table(t), gpu_ctx.table(a), gpu_ctx.table(b)
    try:
        want = orc.execute(gpu_ctx.sql_plan(J.JOIN_PAYLOAD, [tt, ta], [t, a]))
        q = gpu_ctx.sql_compile(J.JOIN_PAYLOAD, [tt, ta])
        q.execute()
        assert q.result().text == want.text and "of r.ru (4 entries)" in q.explain
        ta.append(tb)
        with pytest.raises(engine.EngineError) as e:
            q.execute()
        assert e.value.status == 1
        q.close()
        src, ex, got = _check(gpu_ctx, monkeypatch, J.JOIN_PAYLOAD, [t, J.concat(a, b)], [tt, ta])
        assert "of r.ru (5 entries)" in ex and got.n_rows == 5
    finally:
        for x in (tt, ta, tb):
            x.close()


def test_a_statement_on_two_shards_keeps_the_hash_form():
    """compiled through rsq_multi_query_compile (Context::shardCompile): the shards' results are merged group by group, which wants hash
    aggregations - a dense table over one shard's dictionary has no such merge and would be refused at execution.  Same answer as with
    the images off; one shard's context alone takes the dense form"""
    t, r = J.tables()
    m = engine.MultiContext([0, 0])
    try:
        tabs = [[sh.table(t), sh.table(r)] for sh in m.shards]
        plan = m.shards[0].sql_plan(J.JOIN_PAYLOAD, tabs[0], [t, r])
        answers = []
        for sw in ("2", "0"):
            os.environ["RSQ_DICT_SCANS"] = sw
            try:
                q = m.compile(plan, tabs)
            finally:
                os.environ["RSQ_DICT_SCANS"] = "2"
            q.execute()
            got = q.result()
            answers.append((got.text, got.tuples))
            q.close()
        assert answers[0] == answers[1]
        one = m.shards[0].sql_compile(J.JOIN_PAYLOAD, tabs[0])
        assert OF in one.explain
        one.close()
        for shard in tabs:
            for tb in shard:
                tb.close()
    finally:
        m.close()
