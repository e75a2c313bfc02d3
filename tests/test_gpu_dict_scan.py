"""Dictionary images on the GPU: a scan that reads one code per row and decodes through the column's dictionary answers what the
oracle answers and what the same context answers with RSQ_DICT_SCANS=0 (the wide string scans) - over row counts around the tile,
widths around the word / chunk / staging boundaries, dictionaries of 1 to 257 entries, the predicates that become truth tables and
those that do not, the sinks, the table's lifecycle, the TPC-H statements at SF1 and shards whose dictionaries differ."""
import os
import sys

import numpy as np
import pytest

from resql_amd import engine, plan as P, tpch_full
from oracle import orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dictcases as D  # noqa: E402

pytestmark = pytest.mark.gpu
T = P.TypeInit


@pytest.fixture(scope="module", autouse=True)
def _dictionary_images_on():
    """the images are opt-in (RSQ_DICT_SCANS=1, read when a table is created and when a statement is compiled): on for this module's
    tables, the module-scoped ones included, and put back afterwards"""
    old = os.environ.get("RSQ_DICT_SCANS")
    os.environ["RSQ_DICT_SCANS"] = "1"
    yield
    if old is None:
        os.environ.pop("RSQ_DICT_SCANS", None)
    else:
        os.environ["RSQ_DICT_SCANS"] = old


def _check(ctx, monkeypatch, sql, host, tabs=None, coded=True):
    """the statement with the dictionary images and without them, both against the oracle; returns the coded run's (source, explain)"""
    own = tabs is None
    if own:
        tabs = [ctx.table(t) for t in host]
    try:
        want = orc.execute(ctx.sql_plan(sql, tabs, host))
        out = {}
        for sw in ("1", "0"):
            monkeypatch.setenv("RSQ_DICT_SCANS", sw)
            q = ctx.sql_compile(sql, tabs)
            try:
                q.execute()
                got = q.result()
                assert got.text == want.text and got.tuples == want.tuples, (sw, sql)
                out[sw] = (q.source, q.explain)
            finally:
                q.close()
        monkeypatch.setenv("RSQ_DICT_SCANS", "1")
        assert "(u32)(vc_" not in out["0"][0]
        assert ("(u32)(vc_" in out["1"][0]) == coded, sql
        return out["1"]
    finally:
        if own:
            for t in tabs:
                t.close()


@pytest.mark.parametrize("n", D.ROW_COUNTS)
def test_row_counts_around_the_tile(gpu_ctx, monkeypatch, n):
    t = D.table(n, T.CHAR(10), D.edge_values(10))
    _check(gpu_ctx, monkeypatch, D.GROUP_SUM, [t], coded=n > 0)


@pytest.mark.parametrize("kind", ["CHAR", "VARCHAR"])
@pytest.mark.parametrize("w", D.WIDTHS)
def test_widths_around_word_chunk_and_staging_boundaries(gpu_ctx, monkeypatch, w, kind):
    vals = D.edge_values(w)
    t = D.table(128 * 9 + 50, getattr(T, kind)(w), vals)
    sql = D.WIDTH_SQL.format(full=vals[2].decode())                       # (a value of the full declared length)
    src, ex = _check(gpu_ctx, monkeypatch, sql, [t])
    assert "dict_bit" in src and f"{w + 8} B/row, 3 B/row stored]" in ex


@pytest.mark.parametrize("count", D.DICT_SIZES)
def test_dictionary_sizes(gpu_ctx, monkeypatch, count):
    t = D.table(3000, T.VARCHAR(9), D.many_values(count))
    _check(gpu_ctx, monkeypatch, D.SIZE_SQL, [t], coded=count <= 256)
    _check(gpu_ctx, monkeypatch, D.SINKS["group_by"], [t], coded=True)    # (column u is coded either way)


@pytest.fixture(scope="module")
def edge_table(gpu_ctx):
    host = D.table(30_000, T.CHAR(9), D.edge_values(9, 40))
    dev = gpu_ctx.table(host)
    yield host, dev
    dev.close()


@pytest.fixture(scope="module")
def edge_table_varchar(gpu_ctx):
    host = D.table(30_000, T.VARCHAR(9), D.edge_values(9, 40), seed=2)
    dev = gpu_ctx.table(host)
    yield host, dev
    dev.close()


@pytest.mark.parametrize("name", sorted(D.PREDICATES))
def test_predicates(gpu_ctx, monkeypatch, edge_table, edge_table_varchar, name):
    for host, dev in (edge_table, edge_table_varchar):
        src, ex = _check(gpu_ctx, monkeypatch, D.PREDICATES[name], [host], [dev])
        if name in ("or_of_two_columns", "and_of_two_columns"):
            assert "s_dt[8]" in src                                       # no single-column table: one per column, combined per row
        else:
            assert "dict_bit" in src
        if name == "late_loads":
            assert "late loads" in ex and "lead_pred" in src


@pytest.mark.parametrize("name", sorted(D.SINKS))
def test_sinks(gpu_ctx, monkeypatch, edge_table, edge_table_varchar, name):
    for host, dev in (edge_table, edge_table_varchar):
        _check(gpu_ctx, monkeypatch, D.SINKS[name], [host], [dev])


@pytest.mark.parametrize("kind", ["CHAR", "VARCHAR"])
def test_join_on_a_coded_column_and_a_coded_payload(gpu_ctx, monkeypatch, kind):
    t, r = D.join_tables(kind)                                            # (CHAR: 'ab' and 'ab ' are two entries on both sides)
    tabs = [gpu_ctx.table(t), gpu_ctx.table(r)]
    try:
        _check(gpu_ctx, monkeypatch, D.JOIN_SQL, [t, r], tabs)
        _check(gpu_ctx, monkeypatch, D.JOIN_GROUP_SQL, [t, r], tabs)
    finally:
        for x in tabs:
            x.close()


def _concat(a, b):
    return P.Table(a.name, [P.Column(x.name, x.type, np.concatenate([x.data, y.data])) for x, y in zip(a.columns, b.columns)], a.n_rows + b.n_rows)


def _append_case(gpu_ctx, monkeypatch, first_values, more_values, coded_after):
    a, b = D.table(5_000, T.VARCHAR(9), first_values, seed=4), D.table(3_000, T.VARCHAR(9), more_values, seed=5)
    ta, tb = gpu_ctx.table(a), gpu_ctx.table(b)
    try:
        sql = D.PREDICATES["like_head"]
        q = gpu_ctx.sql_compile(sql, [ta])
        q.execute()
        assert "dict_bit" in q.source
        ta.append(tb)
        with pytest.raises(engine.EngineError) as e:
            q.execute()                                                   # compiled over the old image: refused
        assert e.value.status == 1
        q.close()
        _check(gpu_ctx, monkeypatch, sql, [_concat(a, b)], [ta], coded=coded_after)
    finally:
        ta.close()


def test_append_within_256_values_shifts_the_codes(gpu_ctx, monkeypatch):
    # the appended values sort in front of the old ones: every old value's code changes
    _append_case(gpu_ctx, monkeypatch, D.many_values(100), np.array([b"a%d" % i for i in range(50)], dtype="S9"), True)


def test_append_that_brings_the_257th_value_drops_the_image(gpu_ctx, monkeypatch):
    _append_case(gpu_ctx, monkeypatch, D.many_values(256), np.array([b"x1", b"one more"], dtype="S9"), False)


def test_refresh_stats_over_unchanged_content_keeps_compiled_statements(gpu_ctx, monkeypatch):
    t = D.table(20_000, T.CHAR(10), D.edge_values(10))
    dt = gpu_ctx.table(t)
    try:
        sql = D.GROUP_SUM
        want = orc.execute(gpu_ctx.sql_plan(sql, [dt], [t]))
        q = gpu_ctx.sql_compile(sql, [dt])
        q.execute()
        assert q.result().text == want.text and "(u32)(vc_0)" in q.source
        before = gpu_ctx.memory_stats()["column_image_bytes"]
        dt.refresh_stats()                                                # same content: the same dictionary, re-encoded in place
        assert gpu_ctx.memory_stats()["column_image_bytes"] == before
        q.execute()
        assert q.result().text == want.text
        q.close()
        _check(gpu_ctx, monkeypatch, sql, [t], [dt])
    finally:
        dt.close()


def test_refresh_that_drops_the_image_refuses_statements_compiled_before(gpu_ctx, monkeypatch):
    """no append here, and the numeric columns keep their narrow images: the dropped dictionary image alone must reach layoutVersion"""
    t = D.table(20_000, T.CHAR(10), D.edge_values(10))
    dt = gpu_ctx.table(t)
    try:
        q = gpu_ctx.sql_compile(D.GROUP_SUM, [dt])
        q.execute()
        assert "(u32)(vc_0)" in q.source
        before = gpu_ctx.memory_stats()["column_image_bytes"]
        monkeypatch.setenv("RSQ_DICT_SCANS", "0")
        dt.refresh_stats()                                                # no dictionary image any more: the old one is freed
        monkeypatch.setenv("RSQ_DICT_SCANS", "1")
        assert gpu_ctx.memory_stats()["column_image_bytes"] == before - (20_000 + 256 * 10 + 16) - (20_000 + 256 * 6 + 16)
        with pytest.raises(engine.EngineError) as e:
            q.execute()                                                   # ... and a statement that held it is refused
        assert e.value.status == 1
        q.close()
        _check(gpu_ctx, monkeypatch, D.GROUP_SUM, [t], [dt], coded=False)  # (the table stays wide until its statistics are refreshed again)
        dt.refresh_stats()
        _check(gpu_ctx, monkeypatch, D.GROUP_SUM, [t], [dt])
    finally:
        dt.close()


def test_memory_stats_account_for_the_images(gpu_ctx):
    before = gpu_ctx.memory_stats()["column_image_bytes"]
    t = D.table(10_000, T.CHAR(25), D.edge_values(25))
    dt = gpu_ctx.table(t)
    grown = gpu_ctx.memory_stats()["column_image_bytes"] - before
    # s and u: a code per row (rounded up to 16 bytes) and 256 entries + 16 bytes each; a: two bytes per row; k: two as well
    assert grown == 2 * 10_000 + (256 * 25 + 16) + (256 * 6 + 16) + 2 * 10_000 + 2 * 10_000
    dt.close()
    assert gpu_ctx.memory_stats()["column_image_bytes"] == before


def test_borrowed_columns_stay_wide(gpu_ctx, monkeypatch):
    import torch
    t = D.table(10_000, T.CHAR(10), D.edge_values(10))
    cols = [torch.from_numpy(np.frombuffer(c.data.tobytes(), dtype=np.uint8).copy()).to("cuda:0") for c in t.columns]
    dt = gpu_ctx.table_from_device("t", t.n_rows, [(c.name, c.type, x.data_ptr()) for c, x in zip(t.columns, cols)])
    try:
        src, ex = _check(gpu_ctx, monkeypatch, D.GROUP_SUM, [t], [dt], coded=False)
        assert "B/row stored" not in ex
    finally:
        dt.close()
        del cols


def test_tpch_statements_at_sf1_switch_on_and_off(monkeypatch):
    db = tpch_full.database(1)
    answers = {}
    for sw in ("0", "1"):
        monkeypatch.setenv("RSQ_DICT_SCANS", sw)
        ctx = engine.Context(device=0)
        try:
            tabs = [ctx.table(db[k]) for k in sorted(db)]
            for name, sql in sorted(tpch_full.QUERIES.items()):
                q = ctx.sql_compile(sql, tabs)
                q.execute()
                r = q.result()
                answers.setdefault(name, []).append((r.text, r.tuples, "(u32)(vc_" in q.source))
                q.close()
            for t in tabs:
                t.close()
        finally:
            ctx.close()
    assert len(answers) == 8
    for name, (off, on) in answers.items():
        assert off[:2] == on[:2], name
        assert not off[2], name
    for name in ("q12", "q14", "q19"):
        assert answers[name][1][2], name


def test_shards_with_different_dictionaries_under_rsq_multi():
    """three shards of one table: the second lacks a value of s, the third holds 300 values in s and so scans it wide; every shard
    codes u.  The shards share one partial-table layout and the answer is the oracle's on the whole table, twice."""
    vals = D.edge_values(9, 20)
    parts = [D.table(4_000, T.VARCHAR(9), vals, seed=11), D.table(4_000, T.VARCHAR(9), vals[1:], seed=12),
             D.table(4_000, T.VARCHAR(9), np.concatenate([vals, D.many_values(280)]), seed=13)]
    whole = _concat(_concat(parts[0], parts[1]), parts[2])
    sql = "select s, u, sum(a), count(*) from t where s like 'x%' or s = 'ab' group by s, u"
    srcs = []
    cc = engine.Context(device=-1)
    try:
        for p in parts:
            dt = cc.table(p)
            q = cc.sql_compile(sql, [dt])
            srcs.append(q.source)
            q.close()
            dt.close()
        plan_tab = cc.table(whole)
        plan = cc.sql_plan(sql, [plan_tab], [whole])
        plan_tab.close()
    finally:
        cc.close()
    assert "const char* d0;" in srcs[0] and "const char* d0;" in srcs[1] and "const char* d0;" not in srcs[2] and "const char* d1;" in srcs[2]
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
        for _ in range(2):
            q.execute()
            got = q.result()
            assert got.text == want.text and got.tuples == want.tuples
        q.close()
        for tb in tabs:
            tb.close()
    finally:
        m.close()
