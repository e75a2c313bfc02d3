"""Derived aggregations across shards (rsq_multi_* with ENGINE_DERIVED_MULTI): every derived table is built on every shard, locally where
its sub-query reads replicated tables only, merged across the shards where one table is sharded and is the source of its aggregating
pipeline; a derived table the last pipeline scans is scanned slice by slice.  Shards list device 0 several times, as
tests/test_gpu_nested_loops_multi.py does; every answer is the reference's recorded one (tests/golden/derived_agg_reference.json) and
the bytes of one context over the whole tables."""
import hashlib
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import derivedcases as D  # noqa: E402
import shardlayouts  # noqa: E402
from resql_amd import dist, engine, tpch_full  # noqa: E402
from resql_amd import plan as P  # noqa: E402

with open(os.path.join(HERE, "golden", "derived_agg_reference.json")) as f:
    GOLD = json.load(f)

pytestmark = pytest.mark.gpu
N = 3
FLAG = engine.ENGINE_DERIVED_MULTI


# ---- plan roles (engine.cpp compileDerived, engine_derived_multi.cpp) ------------------------------------------------------------
def _parents(plan):
    par = {}
    for i, o in enumerate(plan.ops):
        for c in o.children:
            par[c] = i
    return par


def _is_derived(plan, par, op):
    if plan.ops[op].tag != "AGGREGATION":
        return False
    a = par.get(op)
    while a is not None:
        if plan.ops[a].tag not in ("PROJECTION", "MATERIALIZE", "ORDERBY"):
            return True
        a = par.get(a)
    return False


def _scans(plan, par, op, out):
    """the scans of op's subtree, and the derived aggregations directly below it (their subtrees belong to them)"""
    o = plan.ops[op]
    if o.tag == "SCAN":
        out[0].append(op)
        return out
    for c in o.children:
        if _is_derived(plan, par, c):
            out[1].append(c)
        else:
            _scans(plan, par, c, out)
    return out


def _chain_source(plan, par, op):
    """what the pipeline through `op` scans: a table's scan or a derived aggregation (codegen.cpp Walker::produce)"""
    if _is_derived(plan, par, op):
        return op
    while plan.ops[op].tag != "SCAN":
        o = plan.ops[op]
        op = o.children[1] if o.tag in ("HASHJOIN", "NESTEDLOOPSJOIN") else o.children[0]
        if _is_derived(plan, par, op):
            return op
    return op


def _classify(plan, sharded):
    """(None, merged: any derived table merged, last: source of the last pipeline) or (refused table name, ...)"""
    par = _parents(plan)
    merged = [False]

    def derived(agg):
        child = plan.ops[agg].children[0]
        scans, below = ([], [child]) if _is_derived(plan, par, child) else _scans(plan, par, child, ([], []))
        for b in below:
            r = derived(b)
            if r:
                return r
        hot = [plan.ops[s].table for s in scans if plan.ops[s].table in sharded]
        if not hot:
            return None
        src = _chain_source(plan, par, plan.ops[agg].children[0])
        if plan.ops[src].tag != "SCAN" or plan.ops[src].table != hot[0] or len(hot) > 1:
            return hot[0]
        merged[0] = True
        return None

    scans, below = _scans(plan, par, plan.root, ([], []))
    for b in below:
        r = derived(b)
        if r:
            return r, False, None
    last = _chain_source(plan, par, plan.root)
    for s in scans:
        if plan.ops[s].table in sharded and s != last:
            return plan.ops[s].table, False, None
    return None, merged[0], ("derived" if plan.ops[last].tag != "SCAN" else plan.ops[last].table)


# ---- tables ---------------------------------------------------------------------------------------------------------------------
_slice = shardlayouts.slice_rows


def _cuts(t: P.Table, kind, n):
    rows = t.n_rows
    if kind == "spread":
        return [0] + [rows * (2 * i + 1) // (2 * n) for i in range(1, n)] + [rows]
    if kind == "late":                                  # shard 0 holds no row
        return [0, 0] + [rows * i // (n - 1) for i in range(1, n - 1)] + [rows]
    if kind == "on_key":                                # no l_orderkey on two shards
        key = t.col("l_orderkey").data
        cuts = [dist.shard_rows_on_key(rows, n, i, lambda r: int(key[r]))[0] for i in range(n)]
        return cuts + [rows]
    raise ValueError(kind)


def Shards(m, tables):
    return shardlayouts.Shards(m, {t.name: t for t in tables}, _cuts)


LAYOUTS = {"replicated": {}, "lineitem": {"lineitem": "spread"}, "lineitem_late": {"lineitem": "late"},
           "lineitem_on_key": {"lineitem": "on_key"}, "orders": {"orders": "spread"}, "customer": {"customer": "spread"}}
LITERAL_LAYOUTS = {"replicated": {}, "emp": {"emp": "spread"}, "emp_late": {"emp": "late"}}


@pytest.fixture(scope="module")
def db():
    return tpch_full.database(GOLD["sf"])


@pytest.fixture(scope="module")
def single(db):
    ctx = engine.Context(device=0)
    tabs = [ctx.table(db[k]) for k in D.TABLES]
    yield ctx, tabs
    for t in tabs:
        t.close()
    ctx.close()


@pytest.fixture(scope="module")
def multi(db):
    m = engine.MultiContext([0] * N, engine_flags=FLAG)
    s = Shards(m, [db[k] for k in D.TABLES])
    yield m, s
    s.close()
    m.close()


def _run(q, times=1):
    try:
        for _ in range(times):
            q.execute()
        return q.result(), q.merge_name if hasattr(q, "merge_name") else None, q.report()
    finally:
        q.close()


def _matches_reference(case, text):
    g = GOLD["cases"][case]
    if "text" in g:
        assert text == g["text"]
    assert hashlib.sha256(text.encode()).hexdigest() == g["sha256"]


@pytest.mark.parametrize("case", [f.__name__ for f in D.CASES])
def test_statement_over_three_shards_in_every_layout(single, multi, db, case, monkeypatch):
    ctx, tabs = single
    m, shards = multi
    plan = getattr(D, case)(db)
    literal = case in D.LITERAL
    if literal:                 # (the two literal tables: shards of their own)
        names = [t.name for t in plan.tables]
        tabs = [ctx.table(t) for t in plan.tables]
        shards = Shards(m, plan.tables)
        layouts = LITERAL_LAYOUTS
    else:
        names = list(D.TABLES)
        layouts = LAYOUTS
    last0 = _classify(plan, set())[2]
    if last0 != "derived":        # (the last pipeline's ordinary source sharded: the caller's shard, as every rsq_multi_* plan has it)
        layouts = dict(layouts, last_source={last0: "spread"})
    try:
        want = _run(ctx.compile(plan, tabs))[0]
        _matches_reference(case, want.text)
        ran = 0
        for layout, cut_of in layouts.items():
            refused, merged, last = _classify(plan, set(cut_of))
            if refused is None and last != "derived" and last not in cut_of:
                # the last pipeline scans an ordinary table every shard holds whole: under the rsq_multi_* contract that table is the
                # caller's shard, so every row would be counted once per shard - not a layout this statement can run in
                continue
            if refused is not None:
                with pytest.raises(engine.EngineError) as e:
                    m.compile(plan, shards.layout(names, cut_of)).close()
                assert e.value.status == 3 and f"table {refused} is sharded" in str(e.value), (layout, str(e.value))
                continue
            # both kernel tiers; and the device path of the merge across shards (devtail.hip k_gm_*) for every group count
            for tier, env in (("full", None), ("generic", ("RSQ_FORCE_GENERIC", "1")), ("device_merge", ("RSQ_DEVICE_TAIL_MIN", "1"))):
                if env:
                    monkeypatch.setenv(*env)
                try:
                    got, merge, _ = _run(m.compile(plan, shards.layout(names, cut_of)))
                finally:
                    if env:
                        monkeypatch.delenv(env[0], raising=False)
                assert got.tuples == want.tuples and got.text == want.text, (layout, tier)
                _matches_reference(case, got.text)
                assert (" merged on the " in merge) == merged, merge
                assert ("sliced" in merge) == (last == "derived"), merge
            ran += 1
        assert ran > 0
    finally:
        if literal:
            shards.close()
            for t in tabs:
                t.close()


def test_every_split_is_exercised(db):
    """the layouts above reach local, merged, sliced, whole and refused derived tables"""
    seen = set()
    for f in D.CASES:
        if f.__name__ in D.LITERAL:
            continue
        plan = f(db)
        for cut_of in LAYOUTS.values():
            refused, merged, last = _classify(plan, set(cut_of))
            seen.add("refused" if refused else ("merged" if merged else "local") + ("_sliced" if last == "derived" else "_whole"))
    assert {"refused", "merged_sliced", "merged_whole", "local_sliced"} <= seen, seen


@pytest.fixture(scope="module")
def sf1():
    return tpch_full.database(1.0, fill_unused=False)


@pytest.mark.parametrize("n_shards", [2, 4])
def test_q18_sf1_device_and_host_merge(sf1, n_shards, monkeypatch, capfd):
    plan = D.q18(sf1, threshold=300)
    ctx = engine.Context(device=0)
    tabs = [ctx.table(sf1[k]) for k in D.TABLES]
    m = engine.MultiContext([0] * n_shards, engine_flags=FLAG)
    li = sf1["lineitem"]
    shards = []
    try:
        want = _run(ctx.compile(plan, tabs))[0]
        assert want.text.count("\n") - 1 == 79
        for i in range(n_shards):
            row = []
            for k in D.TABLES:
                if k == "lineitem":
                    r0, nr = dist.shard_rows(li.n_rows, n_shards, i)
                    t = m.shards[i].table(_slice(li, r0, r0 + nr))
                    t.set_row0(r0)
                else:
                    t = m.shards[i].table(sf1[k])
                row.append(t)
            shards.append(row)
        monkeypatch.setenv("RSQ_TRACE", "1")
        for path, env in (("device", None), ("host", "0")):
            if env is not None:
                monkeypatch.setenv("RSQ_DEVICE_TAIL", env)
            capfd.readouterr()
            got, merge, _ = _run(m.compile(plan, shards))
            err = capfd.readouterr().err
            assert got.tuples == want.tuples and got.text == want.text, path
            line = [l for l in err.splitlines() if l.startswith("[rsq trace] derived0: ") and " merged " in l]
            assert len(line) == 1 and f"merged on the {path}" in line[0] and f"over {n_shards} shards" in line[0], err[-3000:]
            assert f"derived0 merged on the {path}" in merge and "whole" in merge, merge
    finally:
        for row in shards:
            for t in row:
                t.close()
        m.close()
        for t in tabs:
            t.close()
        ctx.close()


@pytest.mark.parametrize("case,layout", [("having_hash_key", "lineitem"), ("agg_over_agg", "lineitem_late"), ("agg_three_deep", "orders"),
                                         ("two_derived_sides", "customer"), ("probe_side", "replicated")])
def test_three_executions_identical(single, multi, db, case, layout):
    ctx, tabs = single
    m, shards = multi
    plan = getattr(D, case)(db)
    q = ctx.compile(plan, tabs)
    try:
        q.execute()
        want, rep1 = q.result(), q.report()
    finally:
        q.close()
    mq = m.compile(plan, shards.layout(list(D.TABLES), LAYOUTS[layout]))
    try:
        outs, reps = [], []
        for _ in range(3):
            mq.execute()
            outs.append(mq.result().tuples)
            reps.append(mq.report()[0])
        merge = mq.merge_name
    finally:
        mq.close()
    assert outs[0] == outs[1] == outs[2] == want.tuples
    assert reps[1].num_kernels == reps[2].num_kernels        # (a first execution may size its tables with passes of its own)
    assert reps[0].num_kernels >= rep1.num_kernels and reps[0].bytes_read >= rep1.bytes_read
    assert merge.startswith("derived tables: ") and "derived0 " in merge
    if layout == "replicated":
        assert "derived0 local, sliced" in merge, merge
    else:
        assert " merged on the " in merge and f"over {N} shards (" in merge and " bytes)" in merge, merge


def test_refusals_that_stay(db, single):
    ctx, tabs = single
    # without the flag: the old refusal and its words
    m0 = engine.MultiContext([0] * N)
    sh0 = Shards(m0, [db[k] for k in D.TABLES])
    try:
        with pytest.raises(engine.EngineError) as e:
            m0.compile(D.having_hash_key(db), sh0.layout(list(D.TABLES), {"lineitem": "spread"}))
        assert e.value.status == 3 and "a multi-GPU compile (rsq_multi_query_compile) of a plan with the derived aggregation" in str(e.value)
    finally:
        sh0.close()
        m0.close()
    # with it: a derived aggregation inside a nested-loops plan
    m1 = engine.MultiContext([0] * N, engine_flags=FLAG | engine.ENGINE_NESTED_LOOPS)
    sh1 = Shards(m1, [db[k] for k in D.TABLES])
    try:
        p = D._plan(db)
        c = p.count(p.star())
        a = p.aggregation([c], [p.attr("s_nationkey")], p.scan("supplier"))
        j = p.nestedloopsjoin(a, p.scan("region"))
        plan = p.set_root(p.materialize(p.projection([p.attr("r_name"), c], j)), request_all=True)
        with pytest.raises(engine.EngineError) as e:
            m1.compile(plan, sh1.layout(list(D.TABLES), {}))
        assert e.value.status == 3 and "derived aggregation" in str(e.value)
    finally:
        sh1.close()
        m1.close()
    # partial and asynchronous execution of a derived plan, on one context (the flag belongs to multi-GPU handles only)
    with pytest.raises(engine.EngineError) as e:
        engine.Context(device=0, engine_flags=FLAG)
    assert e.value.status == 1 and "multi-GPU handles" in str(e.value)
    c2 = engine.Context(device=0)
    t2 = [c2.table(db[k]) for k in D.TABLES]
    try:
        for call in ("execute_partial", "execute_partial_async"):
            q = c2.compile(D.having_ungrouped(db), t2)
            try:
                with pytest.raises(engine.EngineError) as e:
                    getattr(q, call)()
                assert e.value.status == 3 and "derived aggregation" in str(e.value)
            finally:
                q.close()
    finally:
        for t in t2:
            t.close()
        c2.close()


# ---- a merged derived table without a single group -------------------------------------------------------------------------------------
def _no_group(db, key):
    """groups of the suppliers no supplier is among, counted by size"""
    p = D._plan(db)
    c = p.count(p.star())
    none = p.selection(p.gt(p.attr("s_acctbal"), p.constant("99999999.00", P.DECIMAL)), p.scan("supplier"))
    a = p.aggregation([c], [p.attr(key)], none)
    return p.set_root(p.materialize(p.aggregation([p.count(p.star())], [c], a)), request_all=True)


@pytest.mark.parametrize("form,key", [("dense", "s_nationkey"), ("hash", "s_name")])
def test_merged_table_without_a_group(single, multi, db, form, key):
    ctx, tabs = single
    m, shards = multi
    plan = _no_group(db, key)
    assert _classify(plan, {"supplier"})[:2] == (None, True)
    want = _run(ctx.compile(plan, tabs))[0]
    mq = m.compile(plan, shards.layout(list(D.TABLES), {"supplier": "spread"}))
    try:
        outs, kernels = [], []
        for _ in range(2):
            mq.execute()
            outs.append(mq.result())
            kernels.append(mq.report()[0].num_kernels)
        merge = mq.merge_name
    finally:
        mq.close()
    assert all(o.tuples == want.tuples and o.text == want.text for o in outs) and want.n_rows == 0
    assert kernels[0] == kernels[1] > 0
    assert "derived0 merged on the " in merge and f"over {N} shards (" in merge, merge
    assert ("dense partial tables" in merge) == (form == "dense"), merge


def test_one_shard_with_the_peer_copy_merge(single, db):
    """a handle of one shard asked for peer copies: every derived table is built locally, the one context's bytes"""
    ctx, tabs = single
    plan = D.having_dense_key(db)
    want = _run(ctx.compile(plan, tabs))[0]
    m = engine.MultiContext([0], merge=engine.MERGE_PEER_COPY, engine_flags=FLAG)
    shards = Shards(m, [db[k] for k in D.TABLES])
    try:
        got, merge, _ = _run(m.compile(plan, shards.layout(list(D.TABLES), {})), times=2)
        assert got.tuples == want.tuples and got.text == want.text and got.n_rows > 0
        assert "derived0 local" in merge and "bytes" not in merge, merge
    finally:
        shards.close()
        m.close()
