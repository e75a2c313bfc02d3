"""GROUP BY over dictionary-coded strings across shards (MultiContext with ENGINE_DICT_MULTI): the shards of a table receive one
dictionary per coded column - the union of theirs, codes rewritten in place by k_dict_recode - so every shard plans the statement dense
by the code and the shards' tables merge as dense partial tables.  Three shards on one GPU whose dictionaries differ (A holds every
value, B lacks the first, C holds a strict subset), 2 000 to 6 000 rows each; every answer is the oracle's over the whole table, text and
tuples, emission order included; every statement is executed twice."""
import os
import sys

import numpy as np
import pytest

from resql_amd import engine, plan as P, tpch_full
from oracle import orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dictcases as D  # noqa: E402
import dictgroupcases as G  # noqa: E402
import dictmulticases as M  # noqa: E402

pytestmark = pytest.mark.gpu
T = P.TypeInit
FLAG = engine.ENGINE_DICT_MULTI
DENSE = "dense partial tables"


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


def _close(tabs):
    for t in tabs:
        t.close()


def _answer(q, want, what, executions=2):
    for _ in range(executions):
        q.execute()
        got = q.result()
        assert got.text == want.text and got.tuples == want.tuples, what
    return got


# ---- 1. the recode kernel, through unify_shard_dictionaries on real tables ---------------------------------------------------------
@pytest.fixture(scope="module")
def plain():
    m = engine.MultiContext([0, 0, 0])
    yield m
    m.close()


def _images(tb):
    return tb.read_image("s", 1).tobytes(), tb.read_image("s", 2).tobytes(), tb.read_image("u", 1).tobytes(), tb.read_image("u", 2).tobytes()


def _decodes(tb, part, col="s"):
    """entries[codes[r]] are the stored bytes of row r"""
    w, n = tb.widths[col], part.n_rows
    raw = tb.read_column(col, np.uint8, n * w).reshape(n, w)
    codes = tb.read_image(col, 2)
    assert len(codes) == n and np.array_equal(M.entries(tb, col)[codes], raw)


@pytest.mark.parametrize("kind,w", M.RECODE_TYPES)
@pytest.mark.parametrize("rows", M.RECODE_ROWS)
def test_recoded_shards_decode_to_their_rows(plain, rows, kind, w):
    parts = M.shards(getattr(T, kind)(w), D.edge_values(w), rows)
    tabs = M.place(plain.shards, parts)
    try:
        for tb, p in zip(tabs, parts):
            _decodes(tb, p)
        old_codes = [tb.read_image("s", 2) for tb in tabs]
        engine.unify_shard_dictionaries(tabs)
        want = M.sorted_union(parts)
        for tb, p in zip(tabs, parts):
            assert np.array_equal(M.entries(tb), want)                    # all shards hold the same entries
            _decodes(tb, p)
            _decodes(tb, p, "u")
        if len(want) > 1:
            assert any(not np.array_equal(o, tb.read_image("s", 2)) for o, tb in zip(old_codes, tabs))      # some shard's codes moved
        before = [_images(tb) for tb in tabs]
        engine.unify_shard_dictionaries(tabs)                             # a second call changes no byte
        assert [_images(tb) for tb in tabs] == before
    finally:
        _close(tabs)


def test_statements_around_the_unification(plain):
    parts = M.shards(T.VARCHAR(9), D.edge_values(9, 12), 3_000)
    tabs = M.place(plain.shards, parts)
    ctx = plain.shards[1]                                                 # shard B: its dictionary lacks the first entry, every code moves
    try:
        want = orc.execute(M.plan_over(G.SUMS, [parts[1]]))
        before = ctx.sql_compile(G.SUMS, [tabs[1]])
        _answer(before, want, "before")
        assert "by dictionary code (10 entries)" in before.explain
        engine.unify_shard_dictionaries(tabs)
        with pytest.raises(engine.EngineError) as e:
            before.execute()                                              # compiled over the old dictionary: refused
        assert e.value.status == 1 and "compile it again" in str(e.value)
        before.close()
        after = ctx.sql_compile(G.SUMS, [tabs[1]])
        assert "by dictionary code (12 entries)" in after.explain
        _answer(after, want, "after")
        engine.unify_shard_dictionaries(tabs)
        _answer(after, want, "after a second call")                       # nothing moved: the statement stands
        after.close()
    finally:
        _close(tabs)


# ---- 2. statements over three differing shards ------------------------------------------------------------------------------------
STATEMENTS = {"sums": G.SUMS, "two_coded": G.TWO_CODED, "mixed": G.MIXED, "late": G.LATE, "hbm": G.HBM, "hbm_top": G.HBM_TOP, "join_own": G.JOIN_OWN}


@pytest.fixture(scope="module")
def three():
    """the three shards of t and r on every shard, on a handle with the flag, on one without, and cut in two for a peer-copy handle"""
    parts = M.random_shards(T.CHAR(9), D.edge_values(9, 12))
    r = G.join_tables()[1]
    whole = M.concat(parts)
    made = {}
    for name, devices, flags, split in (("on", [0, 0, 0], FLAG, parts), ("off", [0, 0, 0], 0, parts),
                                        ("two", [0, 0], FLAG, [parts[0], M.concat(parts[1:])])):
        m = engine.MultiContext(devices, merge=engine.MERGE_PEER_COPY, engine_flags=flags)
        made[name] = (m, [[t, sh.table(r)] for t, sh in zip(M.place(m.shards, split), m.shards)])
    yield whole, r, made
    for m, tabs in made.values():
        m.close()


@pytest.mark.parametrize("name", sorted(STATEMENTS))
def test_statements_merge_as_dense_partial_tables(three, name):
    whole, r, made = three
    plan = M.plan_over(STATEMENTS[name], [whole, r])
    want = orc.execute(plan)
    answers = {}
    for which, (m, tabs) in made.items():
        q = m.compile(plan, tabs)
        try:
            got = _answer(q, want, (name, which))
            answers[which] = (got.text, got.tuples)
            with pytest.raises(IndexError):
                q.explain(m.n)
            if which == "off":
                # the parent's behaviour, kept without the flag: this is the assertion that fails there for the other two handles
                assert DENSE not in q.merge_name and all(G.NOTE not in q.explain(i) for i in range(m.n))
            else:
                assert DENSE in q.merge_name, q.merge_name
                assert all(G.NOTE in q.explain(i) and "(12 entries)" in q.explain(i) for i in range(m.n))
        finally:
            q.close()
    assert answers["on"] == answers["off"] == answers["two"]


# ---- 3. first rows are numbered over the whole table ----------------------------------------------------------------------------
def test_first_rows_decide_the_order_whatever_shard_holds_them():
    """shard 2 holds the table's FIRST rows and shard 0 its last: a group first occurs in shard 2 although shard 0 holds later rows of it,
    and one group's only rows are in the last shard; no ORDER BY, the oracle's emission order"""
    vals = np.sort(D.edge_values(9, 12))
    first = G.table(2_000, T.VARCHAR(9), vals[:9], seed=50)               # the table's rows in order: these, ...
    mid = G.table(2_200, T.VARCHAR(9), vals[3:10], seed=51)
    last = G.table(2_400, T.VARCHAR(9), vals[2:], seed=52)                # ... and vals[10:] occur here alone
    want = orc.execute(M.plan_over(G.SUMS, [M.concat([first, mid, last])]))
    for order in ([2, 1, 0], [0, 1, 2]):                                  # shard i holds part order[i]
        m = engine.MultiContext([0, 0, 0], engine_flags=FLAG)
        try:
            parts, row0 = [first, mid, last], [0, 2_000, 4_200]
            tabs = []
            for i, p in enumerate(order):
                tb = m.shards[i].table(parts[p])
                tb.set_row0(row0[p])
                tabs.append(tb)
            q = m.compile(M.plan_over(G.SUMS, [M.concat([first, mid, last])]), [[tb] for tb in tabs])
            assert DENSE in q.merge_name and G.NOTE in q.explain(0)
            _answer(q, want, order)
            q.close()
        finally:
            m.close()


# ---- 4. CHAR(9): entries equal up to trailing spaces in different shards ------------------------------------------------------------
@pytest.mark.parametrize("tail", ["host", "device"])
@pytest.mark.parametrize("spelling", [b"ab", b"ab "])
def test_entries_equal_up_to_trailing_spaces_in_different_shards_are_one_group(monkeypatch, tail, spelling):
    vals = D.edge_values(9, 12)
    assert b"ab" in vals and b"ab " in vals
    other = b"ab " if spelling == b"ab" else b"ab"
    a = G.table(2_000, T.CHAR(9), vals[vals != other], seed=60)           # the first rows spell it `spelling` ...
    b = G.table(2_000, T.CHAR(9), vals[vals != spelling], seed=61)        # ... the later ones the other way
    whole = M.concat([a, b])
    plan = M.plan_over(G.SUMS, [whole])
    want = orc.execute(plan)
    assert sum(1 for l in want.text.splitlines() if l.split("|")[0].rstrip() == "ab") == 1      # one merged group
    if tail == "device":
        monkeypatch.setenv("RSQ_DEVICE_TAIL_MIN", "1")
    m = engine.MultiContext([0, 0], engine_flags=FLAG)
    try:
        tabs = M.place(m.shards, [a, b])
        q = m.compile(plan, [[tb] for tb in tabs])
        assert DENSE in q.merge_name and "(12 entries)" in q.explain(1)
        _answer(q, want, (tail, spelling))
        q.close()
    finally:
        m.close()


# ---- 5. a key from a join's build side (RSQ_DICT_SCANS=2) ------------------------------------------------------------------------
def test_a_build_side_key_is_dense_by_the_replicated_tables_dictionary(monkeypatch):
    monkeypatch.setenv("RSQ_DICT_SCANS", "2")
    parts = M.random_shards(T.CHAR(9), D.edge_values(9, 12), seed=70)
    whole, r = M.concat(parts), G.join_tables()[1]
    plan = M.plan_over(G.JOIN_PAYLOAD, [whole, r])
    want = orc.execute(plan)
    m = engine.MultiContext([0, 0, 0], engine_flags=FLAG)
    try:
        ts = M.place(m.shards, parts)
        rs = [sh.table(r) for sh in m.shards]
        q = m.compile(plan, [[t, x] for t, x in zip(ts, rs)])
        assert DENSE in q.merge_name and all("key ru by dictionary code of r.ru (4 entries)" in q.explain(i) for i in range(3))
        _answer(q, want, "t sharded, r replicated")
        q.close()
        # t replicated too: every shard would scan the same rows - the hash form, as before the feature
        whole_ts = [sh.table(parts[0]) for sh in m.shards]
        plan0 = M.plan_over(G.JOIN_PAYLOAD, [parts[0], r])
        q = m.compile(plan0, [[t, x] for t, x in zip(whole_ts, rs)])
        assert DENSE not in q.merge_name and all("the statement runs on several shards" in q.explain(i) for i in range(3))
        q.close()
    finally:
        m.close()


def test_copies_of_the_build_side_that_differ_keep_the_hash_form(monkeypatch):
    """one row of r has a key outside t's values, and on ONE shard's copy a value of ru that occurs nowhere else: nothing the statistics
    compare differs, the dictionaries do - the key is dense on no shard, and the answer is the oracle's"""
    monkeypatch.setenv("RSQ_DICT_SCANS", "2")
    parts = M.random_shards(T.CHAR(9), D.edge_values(9, 12), seed=70)
    whole, r, odd = M.concat(parts), G.join_tables()[1], G.join_tables()[1]
    for x in (r, odd):
        x.col("ra").data[-1] = 5000
    odd.col("ru").data[-1] = b"EXTRA"
    plan = M.plan_over(G.JOIN_PAYLOAD, [whole, r])
    want = orc.execute(plan)
    m = engine.MultiContext([0, 0, 0], engine_flags=FLAG)
    try:
        ts = M.place(m.shards, parts)
        rs = [m.shards[0].table(r), m.shards[1].table(r), m.shards[2].table(odd)]
        assert [x.image_info("ru")[2] for x in rs] == [4, 4, 5]
        q = m.compile(plan, [[t, x] for t, x in zip(ts, rs)])
        assert DENSE not in q.merge_name and all(G.NOTE + " of" not in q.explain(i) for i in range(3))
        _answer(q, want, "one copy of r differs")
        q.close()
    finally:
        m.close()


# ---- 6. what is not unified takes the hash form and the oracle's answer ------------------------------------------------------------
@pytest.mark.parametrize("case", ["union_of_257", "one_shard_of_300"])
def test_fallbacks_keep_the_hash_form(case):
    if case == "union_of_257":
        parts = [G.table(2_000, T.VARCHAR(9), G.values(129, 9, b"a"), seed=80), G.table(2_000, T.VARCHAR(9), G.values(128, 9, b"b"), seed=81)]
    else:
        parts = [G.table(2_000, T.VARCHAR(9), G.values(7), seed=82), G.table(2_000, T.VARCHAR(9), G.values(300), seed=83)]
    plan = M.plan_over(G.SUMS, [M.concat(parts)])
    want = orc.execute(plan)
    m = engine.MultiContext([0, 0], engine_flags=FLAG)
    try:
        tabs = M.place(m.shards, parts)
        q = m.compile(plan, [[tb] for tb in tabs])
        assert DENSE not in q.merge_name and all("hash aggregation" in q.explain(i) and G.NOTE not in q.explain(i) for i in range(2))
        _answer(q, want, case)
        q.close()
    finally:
        m.close()


def test_two_statements_in_a_row_both_keep_executing(three):
    whole, r, made = three
    m, tabs = made["on"]
    plans = [M.plan_over(sql, [whole, r]) for sql in (G.SUMS, G.COUNT)]
    first = m.compile(plans[0], tabs)
    second = m.compile(plans[1], tabs)                                    # unifies again: nothing moves, the first statement stands
    try:
        for q, plan in ((first, plans[0]), (second, plans[1]), (first, plans[0])):
            assert DENSE in q.merge_name
            _answer(q, orc.execute(plan), "two statements", executions=1)
    finally:
        first.close()
        second.close()


# ---- 7. TPC-H Q12 and Q5 at SF 0.01 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,switch", [("q12", "1"), ("q5", "2")])
def test_tpch_statements_with_lineitem_sharded(monkeypatch, name, switch):
    monkeypatch.setenv("RSQ_DICT_SCANS", switch)
    db = tpch_full.database(0.01)
    names = sorted(db)
    host = [db[k] for k in names]
    plan = M.plan_over(tpch_full.QUERIES[name], host)
    want = orc.execute(plan)
    li = db["lineitem"]
    m = engine.MultiContext([0, 0, 0], engine_flags=FLAG)
    try:
        per = []
        for i, sh in enumerate(m.shards):
            r0, nr = m.shard_rows(li.n_rows, i)
            part = P.Table("lineitem", [P.Column(c.name, c.type, c.data[r0:r0 + nr]) for c in li.columns], nr)
            tabs = []
            for k in names:
                tb = sh.table(part if k == "lineitem" else db[k])
                if k == "lineitem":
                    tb.set_row0(r0)
                tabs.append(tb)
            per.append(tabs)
        q = m.compile(plan, per)
        assert DENSE in q.merge_name, q.merge_name
        assert all(G.NOTE in q.explain(i) for i in range(3))
        _answer(q, want, name)
        q.close()
    finally:
        m.close()


def test_a_shard_without_rows_plans_and_merges_like_its_siblings():
    parts = M.random_shards(T.CHAR(9), D.edge_values(9, 12), rows=(2_000, 0, 2_100), seed=90)
    plan = M.plan_over(G.TWO_CODED, [M.concat(parts)])
    want = orc.execute(plan)
    m = engine.MultiContext([0, 0, 0], engine_flags=FLAG)
    try:
        tabs = M.place(m.shards, parts)
        q = m.compile(plan, [[tb] for tb in tabs])
        assert DENSE in q.merge_name and all(G.NOTE in q.explain(i) for i in range(3))
        assert tabs[1].image_info("s")[2] == 12 and len(tabs[1].read_image("s", 2)) == 0      # the union, and no codes
        _answer(q, want, "an empty shard")
        q.close()
    finally:
        m.close()


def test_timing_a_pass_leaves_the_codes_as_they_were(gpu_ctx):
    t = G.table(G.ROWS, T.VARCHAR(9), D.edge_values(9, 12), seed=91)
    tb = gpu_ctx.table(t)
    try:
        before = _images(tb)
        assert tb.time_dictionary_pass("s", 0) > 0 and tb.time_dictionary_pass("s", 1) > 0
        assert _images(tb) == before
        with pytest.raises(engine.EngineError):
            tb.time_dictionary_pass("a", 0)                               # not a coded column
    finally:
        tb.close()
