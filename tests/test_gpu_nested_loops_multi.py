"""Nested-loops joins across shards (rsq_multi_* with RSQ_ENGINE_NESTED_LOOPS): the pair space is split by the outer side's rows,
every shard sees the whole inner side (computed locally where its tables are replicated, all-gathered where one table is sharded).
Shards list device 0 several times, as tests/test_gpu_multi.py does; every answer is the reference's recorded one and the bytes of
one flagged context over the whole tables."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

from resql_amd import engine, tpch_full
from resql_amd import plan as P

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import shardlayouts  # noqa: E402
from test_gpu_nested_loops import JIT_CAST, NO_ROW_IN_REFERENCE, _source_answer  # noqa: E402

with open(os.path.join(HERE, "golden", "nlj_reference.json")) as f:
    GOLD = json.load(f)

pytestmark = pytest.mark.gpu
N = 3
FLAG = engine.ENGINE_NESTED_LOOPS


# ---- plan roles: which table a nested-loops join's outer and inner pipelines scan (codegen.cpp Walker::produce) ----------------
def _chain_scan(plan, op):
    while plan.ops[op].tag != "SCAN":
        o = plan.ops[op]
        op = o.children[1] if o.tag in ("HASHJOIN", "NESTEDLOOPSJOIN") else o.children[0]
    return op


def _subtree(plan, op, out):
    out.append(op)
    for c in plan.ops[op].children:
        _subtree(plan, c, out)
    return out


def _roles(plan):
    """(outer table, inner source table, [build-side / nested-inner tables of the inner side], [build tables of the outer side])"""
    inner_ops = []
    for i, o in enumerate(plan.ops):
        if o.tag == "NESTEDLOOPSJOIN":
            _subtree(plan, o.children[0], inner_ops)
    top = [i for i, o in enumerate(plan.ops) if o.tag == "NESTEDLOOPSJOIN" and i not in inner_ops]
    assert len(top) == 1
    nlj = plan.ops[top[0]]
    outer, inner = _chain_scan(plan, nlj.children[1]), _chain_scan(plan, nlj.children[0])
    inner_side = _subtree(plan, nlj.children[0], [])
    others_in = [plan.ops[o].table for o in inner_side if plan.ops[o].tag == "SCAN" and o != inner]
    others_out = [plan.ops[o].table for o in _subtree(plan, nlj.children[1], []) if plan.ops[o].tag == "SCAN" and o != outer]
    return plan.ops[outer].table, plan.ops[inner].table, others_in, others_out


# ---- tables ---------------------------------------------------------------------------------------------------------------------
_slice = shardlayouts.slice_rows


def _cuts(n, kind):
    # explicit cuts: region and nation put rows on every shard; "late" leaves shard 0 empty
    return {"spread": [0, n // 5, 3 * n // 5, n], "late": [0, 0, n // 2, n]}[kind]


def Shards(m, db):
    """the database's tables over m's three shards, under the cuts above"""
    return shardlayouts.Shards(m, db, lambda t, kind, n: _cuts(t.n_rows, kind))


@pytest.fixture(scope="module")
def db():
    return tpch_full.database(GOLD["sf"])


@pytest.fixture(scope="module")
def single(db):
    """one flagged context over the whole tables: the plans and the bytes every sharded run must give"""
    ctx = engine.Context(device=0, engine_flags=FLAG)
    tabs = [ctx.table(db[k]) for k in GOLD["tables"]]
    yield ctx, tabs
    for t in tabs:
        t.close()
    ctx.close()


@pytest.fixture(scope="module")
def multi(db):
    m = engine.MultiContext([0] * N, engine_flags=FLAG)
    s = Shards(m, db)
    yield m, s
    s.close()
    m.close()


def _run_single(ctx, tabs, plan):
    q = ctx.compile(plan, tabs)
    try:
        q.execute()
        return q.result()
    finally:
        q.close()


def _run_multi(m, plan, per_shard, times=1):
    q = m.compile(plan, per_shard)
    try:
        for _ in range(times):
            q.execute()
        return q.result(), q.merge_name, q.report()
    finally:
        q.close()


LAYOUTS = ["replicated", "outer", "inner", "both", "late_outer"]


def _cut_of(layout, outer, inner):
    return {"replicated": {}, "outer": {outer: "spread"}, "inner": {inner: "spread"}, "both": {outer: "spread", inner: "spread"},
            "late_outer": {outer: "late", inner: "spread"}}[layout]


def _check_answer(c, res, db):
    if c["sql"] in NO_ROW_IN_REFERENCE:
        assert res.text.splitlines()[0] == c["result"].splitlines()[0]
        rows = [tuple(v.rstrip(b" ") if isinstance(v, bytes) else v for v in r) for r in res.rows()]
        assert sorted(rows) == _source_answer(c["sql"], db)
    else:
        assert res.text == c["result"], c["sql"]


@pytest.mark.parametrize("i", range(len(GOLD["cases"])))
def test_statement_over_three_shards_in_every_layout(single, multi, db, i):
    c = GOLD["cases"][i]
    ctx, tabs = single
    m, shards = multi
    names = GOLD["tables"]
    if "refused" in c:
        with pytest.raises(engine.EngineError) as e:
            plan = ctx.sql_plan(c["sql"], tabs, [db[k] for k in names])
            _run_multi(m, plan, shards.layout(names, {}))
        assert e.value.status == 2 and c["refused"].replace("ResqlError: ", "") in str(e.value)
        return
    if c["sql"] in JIT_CAST:        # (the JIT's own cast: contexts of their own)
        ctx = engine.Context(device=0, engine_flags=FLAG, compat_flags=engine.COMPAT_JIT_INT16_CAST)
        tabs = [ctx.table(db[k]) for k in names]
        m = engine.MultiContext([0] * N, engine_flags=FLAG, compat_flags=engine.COMPAT_JIT_INT16_CAST)
        shards = Shards(m, db)
    try:
        plan = ctx.sql_plan(c["sql"], tabs, [db[k] for k in names])
        want = _run_single(ctx, tabs, plan)
        _check_answer(c, want, db)
        outer, inner, others_in, others_out = _roles(plan)
        for layout in LAYOUTS:
            if outer == inner and layout in ("outer", "inner", "late_outer"):
                continue
            got, merge, _ = _run_multi(m, plan, shards.layout(names, _cut_of(layout, outer, inner)))
            assert got.tuples == want.tuples and got.text == want.text, (layout, c["sql"])
            _check_answer(c, got, db)
            assert ("gathered" in merge) == (layout in ("inner", "both", "late_outer")), merge
        # outside the contract: a sharded build side or nested inner table, named in the refusal
        for t in others_in + others_out:
            with pytest.raises(engine.EngineError) as e:
                _run_multi(m, plan, shards.layout(names, {t: "spread"}))
            assert e.value.status == 3 and f"table {t} is sharded" in str(e.value), str(e.value)
        if others_in:
            with pytest.raises(engine.EngineError) as e:             # two sharded tables under the inner side
                _run_multi(m, plan, shards.layout(names, {inner: "spread", others_in[0]: "spread"}))
            assert e.value.status == 3 and others_in[0] in str(e.value) and "two sharded tables" in str(e.value)
    finally:
        if c["sql"] in JIT_CAST:
            shards.close()
            m.close()
            for t in tabs:
                t.close()
            ctx.close()


def test_every_layout_kind_is_exercised(single, db):
    """the fixtures hold hash-join pieces on the inner and on the outer side and a nested inner side, so the refusals above run"""
    ctx, tabs = single
    seen_in = seen_out = 0
    for c in GOLD["cases"]:
        if "refused" in c:
            continue
        _, _, others_in, others_out = _roles(ctx.sql_plan(c["sql"], tabs, [db[k] for k in GOLD["tables"]]))
        seen_in += bool(others_in)
        seen_out += bool(others_out)
    assert seen_in >= 2 and seen_out >= 1


def test_shards_of_the_gathered_table_must_ascend(single, multi, db):
    ctx, tabs = single
    m, _ = multi
    names = GOLD["tables"]
    plan = ctx.sql_plan("select r_name, n_name from region, nation", tabs, [db[k] for k in names])
    per = [[m.shards[i].table(db[k]) for k in names] for i in range(N)]
    cut = _cuts(5, "spread")
    r = names.index("region")
    for i in range(N):                           # shard i holds rows of region in reverse shard order
        per[i][r].close()
        j = N - 1 - i
        per[i][r] = m.shards[i].table(_slice(db["region"], cut[j], cut[j + 1]))
        per[i][r].set_row0(cut[j])
    try:
        with pytest.raises(engine.EngineError) as e:
            m.compile(plan, per)
        assert e.value.status == 3 and "table region" in str(e.value) and "increasing row ranges" in str(e.value)
    finally:
        for ts in per:
            for t in ts:
                t.close()


# ---- DESIGN §4's shapes at SF1, against numpy -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sf1():
    return tpch_full.database(1.0, fill_unused=False)


def _shard_rows(m, n):
    return [m.shard_rows(n, i) for i in range(m.n)]


@pytest.mark.parametrize("n_shards", [2, 4])
def test_lineitem_outer_over_shards(sf1, n_shards):
    db = sf1
    names = ["nation", "lineitem"]
    m = engine.MultiContext([0] * n_shards, engine_flags=FLAG)
    per = []
    try:
        for i, (r0, nr) in enumerate(_shard_rows(m, db["lineitem"].n_rows)):
            li = m.shards[i].table(_slice(db["lineitem"], r0, r0 + nr))
            li.set_row0(r0)
            per.append([m.shards[i].table(db["nation"]), li])
        plan = m.shards[0].sql_plan("select count(*) from nation, lineitem where l_quantity < n_nationkey * 2", per[0], [db[k] for k in names])
        got, merge, (rep, _) = _run_multi(m, plan, per)
        assert "inner side replicated" in merge and f"outer rows over {n_shards} shards" in merge
        qty = np.asarray(db["lineitem"].col("l_quantity").data).astype(np.int64)
        scale = 10 ** db["lineitem"].col("l_quantity").type.scale
        want = sum(int((qty < int(k) * 2 * scale).sum()) for k in np.asarray(db["nation"].col("n_nationkey").data))
        assert [tuple(int(v) for v in r) for r in got.rows()] == [(want,)]
    finally:
        for ts in per:
            for t in ts:
                t.close()
        m.close()


@pytest.mark.parametrize("n_shards", [2, 4])
def test_orders_inner_gathered_over_shards(sf1, n_shards):
    db = dict(sf1)
    od = db["orders"]          # (no TPC-H statement reads o_totalprice: the test gives it values, DECIMAL(12,2) hundredths)
    price = np.random.default_rng(7).integers(90_000, 50_000_000, od.n_rows, dtype=np.int64)
    db["orders"] = P.Table(od.name, [P.Column(c.name, c.type, price if c.name == "o_totalprice" else c.data) for c in od.columns], od.n_rows)
    names = ["orders", "supplier"]
    K = 120_000
    m = engine.MultiContext([0] * n_shards, engine_flags=FLAG)
    per = []
    try:
        for i, (r0, nr) in enumerate(_shard_rows(m, db["orders"].n_rows)):
            od = m.shards[i].table(_slice(db["orders"], r0, r0 + nr))
            od.set_row0(r0)
            per.append([od, m.shards[i].table(db["supplier"])])
        # (the pieces fold in the creation order of their roots: a selection on each side keeps orders the inner one)
        sql = (f"select s_nationkey, count(*) from orders, supplier where o_orderkey < {K} and o_totalprice < s_acctbal * 10 "
               "and s_suppkey > 0 group by s_nationkey")
        plan = m.shards[0].sql_plan(sql, per[0], [db[k] for k in names])
        assert _roles(plan)[:2] == ("supplier", "orders")
        got, merge, _ = _run_multi(m, plan, per)
        assert "inner side gathered" in merge and "bytes)" in merge
        ok = np.asarray(db["orders"].col("o_orderkey").data).astype(np.int64)
        price = np.sort(np.asarray(db["orders"].col("o_totalprice").data).astype(np.int64)[ok < K])
        acct = np.asarray(db["supplier"].col("s_acctbal").data).astype(np.int64)
        nk = np.asarray(db["supplier"].col("s_nationkey").data).astype(np.int64)
        per_supp = np.searchsorted(price, acct * 10, side="left")          # orders with o_totalprice < s_acctbal * 10
        want = {}
        for k, c in zip(nk, per_supp):
            want[int(k)] = want.get(int(k), 0) + int(c)
        assert len(price) > 1000
        assert sorted(tuple(int(v) for v in r) for r in got.rows()) == sorted((k, c) for k, c in want.items() if c > 0)
    finally:
        for ts in per:
            for t in ts:
                t.close()
        m.close()


# ---- a group key from the gathered inner side never proves the shards disjoint ----------------------------------------------------
def test_inner_group_key_with_order_by_limit(single, multi, db):
    ctx, tabs = single
    m, shards = multi
    names = GOLD["tables"]
    sql = ("select o_orderkey, o_custkey, count(*) from orders, supplier where o_totalprice < s_acctbal * 30 and s_suppkey < 5 "
           "group by o_orderkey, o_custkey order by o_orderkey desc limit 5")            # (two keys: a hash aggregation)
    plan = ctx.sql_plan(sql, tabs, [db[k] for k in names])
    outer, inner, _, _ = _roles(plan)
    assert (outer, inner) == ("supplier", "orders")
    want = _run_single(ctx, tabs, plan)
    keys = np.asarray(db["orders"].col("o_orderkey").data)
    cut = _cuts(db["orders"].n_rows, "spread")
    ranges = [(keys[cut[i]:cut[i + 1]].min(), keys[cut[i]:cut[i + 1]].max()) for i in range(N)]
    assert all(ranges[i][1] < ranges[i + 1][0] for i in range(N - 1))      # the orders shards are disjoint in o_orderkey
    got, merge, _ = _run_multi(m, plan, shards.layout(names, {"orders": "spread"}))
    assert "ordered merge" not in merge and "gathered" in merge, merge
    assert got.n_rows == 5 and got.tuples == want.tuples and got.text == want.text


# ---- the pair budget bounds the statement ------------------------------------------------------------------------------------------
def test_budget_counts_the_whole_statement(db):
    names = GOLD["tables"]
    sql = "select r_name, n_name from region, nation"            # 25 outer (nation) x 5 inner (region) = 125 pairs
    for cap, refused in ((124, True), (125, False)):
        one = engine.Context(device=0, engine_flags=FLAG, nested_loops_max_pairs=cap)
        one_tabs = [one.table(db[k]) for k in names]
        m = engine.MultiContext([0] * N, engine_flags=FLAG, nested_loops_max_pairs=cap)
        shards = Shards(m, db)
        try:
            plan = one.sql_plan(sql, one_tabs, [db[k] for k in names])
            assert _roles(plan)[:2] == ("nation", "region")
            per = shards.layout(names, {"nation": "spread", "region": "spread"})
            if refused:
                with pytest.raises(engine.EngineError):
                    _run_single(one, one_tabs, plan)
                q = m.compile(plan, per)
                with pytest.raises(engine.EngineError) as e:
                    q.execute()
                assert e.value.status == 3
                assert "25 outer rows x 5 inner rows" in str(e.value) and "nested_loops_max_pairs (124 pairs)" in str(e.value)
                refused_kernels = q.report()[0].num_kernels
                q.close()
                inner_plan = one.sql_plan("select * from region", one_tabs, [db[k] for k in names])
                _, _, (rep, _) = _run_multi(m, inner_plan, per)            # the inner side's own query over the same shards
                assert refused_kernels == rep.num_kernels > 0              # every shard ran its inner part; no pair kernel did
            else:
                want = _run_single(one, one_tabs, plan)
                got, _, _ = _run_multi(m, plan, per)
                assert got.n_rows == 125 and got.tuples == want.tuples
        finally:
            shards.close()
            m.close()
            for t in one_tabs:
                t.close()
            one.close()


def test_without_the_flag_a_multi_handle_refuses(single, db):
    ctx, tabs = single
    names = GOLD["tables"]
    plan = ctx.sql_plan("select count(*) from region, nation", tabs, [db[k] for k in names])
    m = engine.MultiContext([0, 0])
    per = [[m.shards[i].table(db[k]) for k in names] for i in range(2)]
    try:
        with pytest.raises(engine.EngineError) as e:
            m.compile(plan, per)
        assert e.value.status == 3 and "a nested-loops join is not executed across GPUs" in str(e.value)
    finally:
        for ts in per:
            for t in ts:
                t.close()
        m.close()


@pytest.mark.parametrize("layout", ["replicated", "inner"])
def test_two_executions_give_identical_bytes(single, multi, db, layout):
    ctx, tabs = single
    m, shards = multi
    names = GOLD["tables"]
    plan = ctx.sql_plan("select s_name, r_name, s_acctbal from supplier, region where s_suppkey < 40", tabs, [db[k] for k in names])
    outer, inner, _, _ = _roles(plan)
    q = m.compile(plan, shards.layout(names, _cut_of(layout, outer, inner)))
    try:
        q.execute()
        a = q.result().tuples
        q.execute()
        b = q.result().tuples
        assert a == b and len(a) > 0 and a == _run_single(ctx, tabs, plan).tuples
        assert ("inner side gathered" if layout == "inner" else "inner side replicated") in q.merge_name, q.merge_name
        if layout == "inner":
            assert q.collective_ms >= 0 and "bytes)" in q.merge_name
    finally:
        q.close()


def _visible_gpus():
    for name in ("libamdhip64.so", "libamdhip64.so.6", "libamdhip64.so.7"):
        try:
            hip = ctypes.CDLL(name)
        except OSError:
            continue
        n = ctypes.c_int(0)
        return n.value if hip.hipGetDeviceCount(ctypes.byref(n)) == 0 else 0
    return 0


def test_gathered_inner_side_over_distinct_devices(single, db):
    n_gpus = _visible_gpus()
    if n_gpus < 2:
        pytest.skip("one GPU visible")
    ctx, tabs = single
    names = GOLD["tables"]
    devices = list(range(min(n_gpus, 4)))
    plan = ctx.sql_plan("select r_name, count(*) from supplier, region where s_nationkey < r_regionkey * 5 group by r_name", tabs,
                        [db[k] for k in names])
    want = _run_single(ctx, tabs, plan)
    m = engine.MultiContext(devices, engine_flags=FLAG)
    shards = Shards(m, db)
    try:
        n = db["supplier"].n_rows
        per = []
        for i in range(m.n):
            lo, hi = i * n // m.n, (i + 1) * n // m.n
            row = [shards.get(i, k) if k != "supplier" else None for k in names]
            sp = m.shards[i].table(_slice(db["supplier"], lo, hi))
            sp.set_row0(lo)
            shards.made[(i, "supplier", "rows")] = sp
            row[names.index("supplier")] = sp
            per.append(row)
        got, merge, _ = _run_multi(m, plan, per)
        assert "inner side gathered" in merge and got.tuples == want.tuples
    finally:
        shards.close()
        m.close()


# ---- the gather moves exactly the inner side's bound columns, once to every other shard ----------------------------------------------
def _attributes(plan, e, out):
    if plan.exprs[e].tag == "ATTRIBUTE":
        out.add(plan.exprs[e].symbol)
    for c in plan.exprs[e].children:
        _attributes(plan, c, out)
    return out


def _bound_width(plan, inner_table):
    """bytes of one inner row in the pair loop: the inner table's columns that the join or an operator above it names
    (codegen.cpp consumeNestedLoops; what only the inner side's own operators read stays there)"""
    top = [o for o in plan.ops if o.tag == "NESTEDLOOPSJOIN"]
    assert len(top) == 1 and not plan.request_all
    inner_ops = set(_subtree(plan, top[0].children[0], []))
    named = set()
    for i, o in enumerate(plan.ops):
        if i not in inner_ops:
            for e in o.exprs + o.exprs2:
                _attributes(plan, e, named)
    return sum(c.type.width for c in inner_table.columns if c.name in named)


@pytest.mark.parametrize("cut,below", [("spread", 40), ("late", 40), ("spread", 0)])
def test_gathered_bytes_are_the_inner_rows_times_the_bound_widths(single, multi, db, cut, below):
    """every shard takes the other two shards' parts: 2 x (inner rows over all shards) x (widths of the bound columns); below = 0: no inner
    row passes, nothing moves"""
    ctx, tabs = single
    m, shards = multi
    names = GOLD["tables"]
    sql = f"select s_name, r_name, s_acctbal from supplier, region where s_suppkey < {below} and r_regionkey >= 0"
    plan = ctx.sql_plan(sql, tabs, [db[k] for k in names])
    assert _roles(plan)[:2] == ("region", "supplier")
    inner_rows = int((np.asarray(db["supplier"].col("s_suppkey").data) < below).sum())
    width = _bound_width(plan, db["supplier"])
    assert width == 25 + 8 and inner_rows == (39 if below else 0)          # s_name CHAR(25), s_acctbal DECIMAL; s_suppkey stays below
    want = _run_single(ctx, tabs, plan)
    got, merge, _ = _run_multi(m, plan, shards.layout(names, {"supplier": cut}), times=2)
    assert f"inner side gathered (peer copies, {2 * inner_rows * width} bytes)" in merge, merge
    assert got.tuples == want.tuples and got.text == want.text and got.n_rows == 5 * inner_rows


def test_one_shard_with_the_peer_copy_merge(single, db):
    """a handle of one shard asked for peer copies: nothing to gather, the one context's bytes"""
    ctx, tabs = single
    names = GOLD["tables"]
    plan = ctx.sql_plan("select r_name, count(*) from supplier, region where s_nationkey < r_regionkey * 5 group by r_name", tabs,
                        [db[k] for k in names])
    want = _run_single(ctx, tabs, plan)
    m = engine.MultiContext([0], merge=engine.MERGE_PEER_COPY, engine_flags=FLAG)
    shards = Shards(m, db)
    try:
        got, merge, _ = _run_multi(m, plan, shards.layout(names, {}), times=2)
        assert got.tuples == want.tuples and got.text == want.text and got.n_rows > 0
        assert "outer rows over 1 shard, inner side replicated" in merge and "bytes" not in merge, merge
    finally:
        shards.close()
        m.close()
