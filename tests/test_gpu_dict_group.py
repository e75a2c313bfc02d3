"""GROUP BY over dictionary-coded string columns on the GPU (RSQ_DICT_SCANS=1): the code the scan loads is the group's dense rank.
Every statement is answered three ways by one context - dense over the codes, with RSQ_DICT_SCANS=0 (wide scans, hash aggregation) and
with RSQ_AGG_MODE=5 (coded scans, hash aggregation) - and all three are the oracle's answer, text and tuples, emission order included.
Shapes are the smallest at which a path can go wrong: rows around one tile, dictionaries of 1 to 257 entries, widths 2, 9 and 25."""
import os
import re
import sys

import numpy as np
import pytest

from resql_amd import engine, plan as P
from oracle import orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dictcases as D  # noqa: E402
import dictgroupcases as G  # noqa: E402

pytestmark = pytest.mark.gpu
T = P.TypeInit


@pytest.fixture(scope="module", autouse=True)
def _dictionary_images_on():
    """the images are opt-in (read when a table is created and when a statement is compiled): on for this module's tables"""
    old = os.environ.get("RSQ_DICT_SCANS")
    os.environ["RSQ_DICT_SCANS"] = "1"
    yield
    if old is None:
        os.environ.pop("RSQ_DICT_SCANS", None)
    else:
        os.environ["RSQ_DICT_SCANS"] = old


def _run(ctx, sql, tabs, want, executions=1):
    q = ctx.sql_compile(sql, tabs)
    try:
        for _ in range(executions):                                       # (the dense table is put back to its identities in between)
            q.execute()
            got = q.result()
            assert got.text == want.text and got.tuples == want.tuples, sql
        return q.source, q.explain
    finally:
        q.close()


def _check(ctx, monkeypatch, sql, host, tabs=None, dense=True, env=None, executions=1):
    """the statement dense over the codes (under `env`), then with the images off and with the hash form forced, all against the oracle;
    returns the first run's (source, explain)"""
    own = tabs is None
    if own:
        tabs = [ctx.table(t) for t in host]
    try:
        want = orc.execute(ctx.sql_plan(sql, tabs, host))
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        src, ex = _run(ctx, sql, tabs, want, executions)
        for k in (env or {}):
            monkeypatch.delenv(k)
        assert (G.NOTE in ex) == dense, ex
        if dense:
            assert "aggregation dense" in ex and re.search(r"\bint gk\d+ = \(int\)\((vc|q)_\d+\);", src)
        monkeypatch.setenv("RSQ_DICT_SCANS", "0")
        s0, e0 = _run(ctx, sql, tabs, want)
        assert "vc_" not in s0 and G.NOTE not in e0
        monkeypatch.setenv("RSQ_DICT_SCANS", "1")
        monkeypatch.setenv("RSQ_AGG_MODE", "5")
        s5, e5 = _run(ctx, sql, tabs, want)
        assert G.NOTE not in e5 and "aggregation dense" not in e5
        monkeypatch.delenv("RSQ_AGG_MODE")
        return src, ex
    finally:
        if own:
            for t in tabs:
                t.close()


@pytest.mark.parametrize("n,count", [(1, 1), (77, 2), (G.ROWS, 7), (G.ROWS, 64), (G.ROWS, 256), (G.ROWS, 257)])
def test_rows_and_dictionary_sizes(gpu_ctx, monkeypatch, n, count):
    t = G.table(n, T.VARCHAR(9), G.values(count))
    src, ex = _check(gpu_ctx, monkeypatch, G.SUMS, [t], dense=count <= 256, executions=2)
    if count <= 256:
        assert f"aggregation dense groups={count} " in ex
    else:
        assert "hash aggregation" in ex                                   # 257 values: no image, the hash form, still right


@pytest.mark.parametrize("kind,w", [("CHAR", 2), ("VARCHAR", 9), ("CHAR", 25), ("VARCHAR", 25)])
def test_edge_values_at_the_widths(gpu_ctx, monkeypatch, kind, w):
    # 'ab' against 'ab ' (one group to CHAR, two entries), the empty value, full-width values, anagrams (they collide in Values::hash)
    t = G.table(G.ROWS, getattr(T, kind)(w), D.edge_values(w))
    _check(gpu_ctx, monkeypatch, G.SUMS, [t])


@pytest.fixture(scope="module")
def edge_tables(gpu_ctx):
    hosts = {kind: G.table(G.ROWS, getattr(T, kind)(9), D.edge_values(9, 12), seed=2 + i) for i, kind in enumerate(("CHAR", "VARCHAR"))}
    devs = {kind: gpu_ctx.table(h) for kind, h in hosts.items()}
    yield hosts, devs
    for d in devs.values():
        d.close()


@pytest.mark.parametrize("name", sorted(G.STATEMENTS))
def test_statements(gpu_ctx, monkeypatch, edge_tables, name):
    hosts, devs = edge_tables
    kinds = ("CHAR", "VARCHAR") if name == "no_order" else ("CHAR",)
    for kind in kinds:
        src, ex = _check(gpu_ctx, monkeypatch, G.STATEMENTS[name], [hosts[kind]], [devs[kind]])
        if name == "two_coded_and_numeric":
            assert "key s by dictionary code (12 entries), key u by dictionary code (5 entries)" in ex


@pytest.mark.parametrize("mode,form", [("1", "in registers"), ("2", "in lane-private LDS"), ("3", "in workgroup LDS table")])
def test_register_and_lds_forms(gpu_ctx, monkeypatch, edge_tables, mode, form):
    hosts, devs = edge_tables
    src, ex = _check(gpu_ctx, monkeypatch, G.COUNT, [hosts["CHAR"]], [devs["CHAR"]], env={"RSQ_AGG_MODE": mode})      # 12 groups x 2 cells
    assert form in ex


@pytest.fixture(scope="module")
def hbm_table(gpu_ctx):
    t = G.table(G.ROWS, T.VARCHAR(9), G.values(256), seed=9)              # 256 entries x a's 1000 values
    dt = gpu_ctx.table(t)
    yield t, dt
    dt.close()


@pytest.mark.parametrize("env", [{}, {"RSQ_PARTITION": "0"}, {"RSQ_PARTITION": "2"}, {"RSQ_PARTITION": "2", "RSQ_STAGED": "0"}],
                         ids=["default", "atomics", "partitioned", "partitioned_unstaged"])
def test_hbm_forms(gpu_ctx, monkeypatch, hbm_table, env):
    t, dt = hbm_table
    src, ex = _check(gpu_ctx, monkeypatch, G.HBM, [t], [dt], env=env, executions=2)
    assert "aggregation dense groups=256000 " in ex and "in HBM table" in ex


@pytest.mark.parametrize("topk", [None, "0"], ids=["candidates", "whole_table"])
def test_hbm_form_ordered_by_an_aggregate_with_limit(gpu_ctx, monkeypatch, hbm_table, topk):
    """ORDER BY an aggregate ... LIMIT over the HBM table: the device selects candidate rows [first row | group id | accumulators] and
    the host tail decodes their group ids (groupsFromDenseRows), coded ranks included; RSQ_DEVICE_TOPK=0 reads the whole table"""
    t, dt = hbm_table
    src, ex = _check(gpu_ctx, monkeypatch, G.HBM_TOP, [t], [dt], env={"RSQ_DEVICE_TOPK": topk} if topk else None, executions=2)
    assert "aggregation dense groups=256000 " in ex and "in HBM table" in ex


def test_two_coded_keys_a_byte_set_and_a_numeric_key(gpu_ctx, monkeypatch):
    t = G.table(G.ROWS, T.CHAR(9), G.values(7), seed=5)
    src, ex = _check(gpu_ctx, monkeypatch, G.MIXED, [t])
    assert f"aggregation dense groups={7 * 5 * 3 * 1000} " in ex


@pytest.mark.parametrize("grid", [None, "4"])
def test_key_column_loaded_late(gpu_ctx, monkeypatch, grid):
    t = G.table(20_000, T.CHAR(9), D.edge_values(9, 12), seed=6)
    src, ex = _check(gpu_ctx, monkeypatch, G.LATE, [t], env={"RSQ_MAX_GRID": grid} if grid else None)
    assert "late loads" in ex and "lead_pred" in src and "const int gk0 = (int)(vc_0);" in src


@pytest.mark.parametrize("kind", ["CHAR", "VARCHAR"])
def test_behind_a_joins_compaction(gpu_ctx, monkeypatch, kind):
    t, r = G.join_tables(kind)
    tabs = [gpu_ctx.table(t), gpu_ctx.table(r)]
    try:
        src, ex = _check(gpu_ctx, monkeypatch, G.JOIN_OWN, [t, r], tabs)
        assert "wave compaction" in ex and "in workgroup LDS table" in ex and re.search(r"const int gk0 = \(int\)\(q_\d+\);", src)      # the code travels in the queue
        if kind == "CHAR":
            _check(gpu_ctx, monkeypatch, G.JOIN_PAYLOAD, [t, r], tabs, dense=False)                  # a build-side payload: the hash form
            # the register and HBM forms behind the same compaction: the code is one of the queue's words there too
            src, ex = _check(gpu_ctx, monkeypatch, G.JOIN_OWN, [t, r], tabs, env={"RSQ_AGG_MODE": "1"})
            assert "wave compaction" in ex and "in registers" in ex and re.search(r"const int gk0 = \(int\)\(q_\d+\);", src)
            src, ex = _check(gpu_ctx, monkeypatch, G.JOIN_OWN_HBM, [t, r], tabs)
            assert "wave compaction" in ex and "aggregation dense groups=12000 " in ex and "in HBM table" in ex
            assert re.search(r"const int gk0 = \(int\)\(q_\d+\);", src)
    finally:
        for x in tabs:
            x.close()


def test_check_stats_gives_the_same_answers(gpu_ctx, monkeypatch, edge_tables):
    hosts, devs = edge_tables
    src, ex = _check(gpu_ctx, monkeypatch, G.TWO_CODED, [hosts["CHAR"]], [devs["CHAR"]], env={"RSQ_CHECK_STATS": "1"})
    assert "if ((u32)gk0 >= 12u)" in src and "if ((u32)gk1 >= 5u)" in src


def _concat(a, b):
    return P.Table(a.name, [P.Column(x.name, x.type, np.concatenate([x.data, y.data])) for x, y in zip(a.columns, b.columns)], a.n_rows + b.n_rows)


def test_append_that_shifts_every_code(gpu_ctx, monkeypatch):
    # the appended values sort in front of the old ones: every old value's code changes
    a = G.table(3_000, T.VARCHAR(9), D.many_values(20), seed=4)
    b = G.table(1_000, T.VARCHAR(9), np.array([b"a%d" % i for i in range(10)], dtype="S9"), seed=5)
    ta, tb = gpu_ctx.table(a), gpu_ctx.table(b)
    try:
        want = orc.execute(gpu_ctx.sql_plan(G.SUMS, [ta], [a]))
        q = gpu_ctx.sql_compile(G.SUMS, [ta])
        q.execute()
        assert q.result().text == want.text and "dictionary code (20 entries)" in q.explain
        ta.append(tb)
        with pytest.raises(engine.EngineError) as e:
            q.execute()                                                   # compiled over the old dictionary: refused
        assert e.value.status == 1
        q.close()
        src, ex = _check(gpu_ctx, monkeypatch, G.SUMS, [_concat(a, b)], [ta])
        assert "dictionary code (30 entries)" in ex
    finally:
        ta.close()
        tb.close()


def test_refresh_over_unchanged_content_keeps_the_statement(gpu_ctx):
    t = G.table(G.ROWS, T.CHAR(9), D.edge_values(9, 12), seed=7)
    dt = gpu_ctx.table(t)
    try:
        want = orc.execute(gpu_ctx.sql_plan(G.SUMS, [dt], [t]))
        q = gpu_ctx.sql_compile(G.SUMS, [dt])
        q.execute()
        assert q.result().text == want.text and G.NOTE in q.explain
        dt.refresh_stats()                                                # same content: the same dictionary, re-encoded in place
        q.execute()
        got = q.result()
        assert got.text == want.text and got.tuples == want.tuples
        q.close()
    finally:
        dt.close()


def test_the_partial_entry_points_answer_as_for_a_hash_aggregation(gpu_ctx, monkeypatch, edge_tables):
    """a dense table keyed by this process's own dictionary never reaches a cross-rank merge: same status and message as with the images off"""
    hosts, devs = edge_tables
    answers = []
    for sw in ("1", "0"):
        monkeypatch.setenv("RSQ_DICT_SCANS", sw)
        q = gpu_ctx.sql_compile(G.SUMS, [devs["CHAR"]])
        assert (G.NOTE in q.explain) == (sw == "1")
        got = []
        for call in (q.execute_partial, q.execute_partial_async, q.partial_layout, lambda: q.bind_partial(256, 8 * 36), q.finalize,
                     lambda: q.finalize_host(np.zeros(36, dtype=np.int64))):
            with pytest.raises(engine.EngineError) as e:
                call()
            got.append((e.value.status, str(e.value)))
        answers.append(got)
        q.close()
    monkeypatch.setenv("RSQ_DICT_SCANS", "1")
    assert answers[0] == answers[1] and all(s == 3 for s, _ in answers[0])


def test_shards_with_different_dictionaries_group_by_the_coded_column():
    """three shards whose dictionaries of s differ: a shard plans as the whole table, its codes are not dense ranks there"""
    vals = D.edge_values(9, 12)
    parts = [G.table(2_000, T.VARCHAR(9), vals, seed=11), G.table(2_000, T.VARCHAR(9), vals[1:], seed=12), G.table(2_000, T.VARCHAR(9), vals[:7], seed=13)]
    whole = _concat(_concat(parts[0], parts[1]), parts[2])
    cc = engine.Context(device=-1)
    try:
        plan_tab = cc.table(whole)
        plan = cc.sql_plan(G.SUMS, [plan_tab], [whole])
        plan_tab.close()
    finally:
        cc.close()
    want = orc.execute(plan)
    m = engine.MultiContext([0, 0, 0])
    try:
        tabs, row0 = [], 0
        for i, p in enumerate(parts):
            tb = m.shards[i].table(p)
            tb.set_row0(row0)
            row0 += p.n_rows
            tabs.append(tb)
        q = m.compile(plan, [[tb] for tb in tabs])
        q.execute()
        got = q.result()
        assert got.text == want.text and got.tuples == want.tuples
        q.close()
        for tb in tabs:
            tb.close()
    finally:
        m.close()


def test_a_table_every_shard_holds_alike_keeps_the_hash_form_under_rsq_multi():
    """the same rows on all three shards: their statistics are equal, the table is not unified and has no row range of a whole - the
    statement still runs on several shards, whose results are merged group by group: the hash form, as without the feature"""
    t = G.table(2_000, T.VARCHAR(9), D.edge_values(9, 12), seed=14)
    m = engine.MultiContext([0, 0, 0])
    try:
        tabs = [sh.table(t) for sh in m.shards]
        plan = m.shards[0].sql_plan(G.SUMS, [tabs[0]], [t])
        answers = []
        for sw in ("1", "0"):
            os.environ["RSQ_DICT_SCANS"] = sw
            try:
                q = m.compile(plan, [[tb] for tb in tabs])
            finally:
                os.environ["RSQ_DICT_SCANS"] = "1"
            q.execute()                                                   # (a dense table over the codes has no group-level merge: it would be refused here)
            got = q.result()
            answers.append((got.text, got.tuples))
            q.close()
        assert answers[0] == answers[1]
        one = m.shards[0].sql_compile(G.SUMS, [tabs[0]])                  # (one context alone: dense over its own dictionary)
        assert G.NOTE in one.explain
        one.close()
        for tb in tabs:
            tb.close()
    finally:
        m.close()
