"""Nested-loops joins whose launch splits the inner rows across workgroups (rsq_config.nested_loops_inner_slices): every slice count
gives the bytes the unsplit launch gives - the reference's answers for the aggregating statements of tests/golden/nlj_reference.json,
numpy models at SF1 sizes with whole tiles, tail rows, remainder-only and empty slices - and what Query.nested_loops_slices() reports."""
import json
import os

import numpy as np
import pytest

from resql_amd import engine, tpch_full
from resql_amd import plan as P

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "nlj_reference.json")) as f:
    GOLD = json.load(f)

pytestmark = pytest.mark.gpu

FLAG = engine.ENGINE_NESTED_LOOPS
SLICES = (0, 1, 3, 64)
AGGREGATED = [i for i, c in enumerate(GOLD["cases"]) if "refused" not in c and "AGGREGATION" in c["plan"]]
# (as tests/test_gpu_nested_loops.py: for these the reference's JIT prints the schema and no row, where its source specifies one row
# per group; the engine's rows are checked against a computation in Python)
NO_ROW_IN_REFERENCE = {
    "select min(s_acctbal), max(s_acctbal), sum(s_acctbal), count(*) from supplier, region where r_regionkey < 3",
    "select count(*) from nation, region where n_name = 'GERMANY' and r_name = 'EUROPE'",
    "select r_name, count(*) from region, nation, supplier where n_nationkey = s_nationkey group by r_name",
    "select count(*) from region, nation, supplier where r_regionkey < 2 and n_nationkey < 3 and s_suppkey < 5",
}


def _source_answer(sql, db):
    def col(t, c):
        return [int(v) for v in np.asarray(db[t].col(c).data)]
    def names(t, c):
        d = np.asarray(db[t].col(c).data)
        return [bytes(np.asarray(v).tobytes()).split(b"\0", 1)[0].rstrip(b" ") for v in d]
    if sql.startswith("select min(s_acctbal)"):
        a = col("supplier", "s_acctbal")
        k = sum(1 for r in col("region", "r_regionkey") if r < 3)
        return [(min(a), max(a), sum(a) * k, len(a) * k)]
    if sql.startswith("select count(*) from nation, region where n_name"):
        return [(names("nation", "n_name").count(b"GERMANY") * names("region", "r_name").count(b"EUROPE"),)]
    if sql.startswith("select r_name, count(*)"):
        nk = set(col("nation", "n_nationkey"))
        m = sum(1 for s in col("supplier", "s_nationkey") if s in nk)
        return sorted((n, m) for n in names("region", "r_name"))
    if sql.startswith("select count(*) from region, nation, supplier"):
        return [(sum(1 for r in col("region", "r_regionkey") if r < 2) * sum(1 for n in col("nation", "n_nationkey") if n < 3) *
                 sum(1 for x in col("supplier", "s_suppkey") if x < 5),)]
    raise KeyError(sql)


@pytest.fixture(scope="module")
def small_db():
    return tpch_full.database(GOLD["sf"])


@pytest.fixture(scope="module")
def small(small_db):
    """per slice setting: a flagged context and the fixtures' tables on it"""
    made = {}
    for s in SLICES:
        ctx = engine.Context(device=0, engine_flags=FLAG, nested_loops_inner_slices=s)
        made[s] = (ctx, [ctx.table(small_db[k]) for k in GOLD["tables"]])
    yield made
    for ctx, tabs in made.values():
        for t in tabs:
            t.close()
        ctx.close()


@pytest.fixture(scope="module")
def sf1():
    """SF1 supplier (78 whole tiles + 16 tail rows) and nation (25 rows: tail rows only) on contexts with 0, 1, 4 and 7 slices"""
    db = tpch_full.database(1.0, fill_unused=False)
    made = {}
    for s in (0, 1, 4, 7):
        ctx = engine.Context(device=0, engine_flags=FLAG, nested_loops_inner_slices=s)
        made[s] = (ctx, {k: ctx.table(db[k]) for k in ("supplier", "nation")})
    yield db, made
    for ctx, tabs in made.values():
        for t in tabs.values():
            t.close()
        ctx.close()


def _run(ctx, tabs, stmt, text=True):
    q = ctx.sql_compile(stmt, tabs) if isinstance(stmt, str) else ctx.compile(stmt, tabs)
    try:
        q.execute()
        return q.result(text=text), q.nested_loops_slices(), q.report().num_kernels
    finally:
        q.close()


def test_fixtures_hold_aggregating_statements_over_5_and_25_inner_rows():
    assert len(AGGREGATED) >= 8
    sqls = [GOLD["cases"][i]["sql"] for i in AGGREGATED]
    assert NO_ROW_IN_REFERENCE <= set(sqls)
    # FROM's first table is the inner side: 25 rows (nation) and 5 rows (region) in 64 slices of whole blocks are remainder-only slices
    # and empty ones
    assert any(s.split(" from ")[1].startswith("nation,") for s in sqls) and any(s.split(" from ")[1].startswith("region,") for s in sqls)


@pytest.mark.parametrize("slices", SLICES)
@pytest.mark.parametrize("i", AGGREGATED)
def test_aggregating_statement_matches_the_reference(small, small_db, i, slices):
    c = GOLD["cases"][i]
    ctx, tabs = small[slices]
    res, used, _ = _run(ctx, tabs, c["sql"])
    assert used >= 1 and (slices == 0 or used == slices)
    if c["sql"] in NO_ROW_IN_REFERENCE:
        assert c["result"].count("\n") == 1             # the reference: the schema line only
        assert res.text.splitlines()[0] == c["result"].splitlines()[0]
        rows = [tuple(v.rstrip(b" ") if isinstance(v, bytes) else v for v in r) for r in res.rows()]
        assert sorted(rows) == _source_answer(c["sql"], small_db)
    else:
        assert res.text == c["result"], c["sql"]


def _raw(col):
    return np.asarray(col.data).astype(np.int64)


def _supplier_x_nation_plan(db):
    p = P.Plan([db["nation"], db["supplier"]])
    cond = p.lt(p.attr("s_acctbal"), p.mul(p.attr("n_nationkey"), p.constant("100", P.BIGINT)))
    nlj = p.nestedloopsjoin(p.scan("nation"), p.scan("supplier"), cond)
    g = p.attr("n_regionkey")
    a = p.attr("s_acctbal")
    aggs = [p.count(p.star()), p.sum(a), p.min(a), p.max(a)]
    p.set_root(p.materialize(p.projection([g] + aggs, p.aggregation(aggs, [g], nlj))))
    return p


def test_10000_outer_x_25_inner_with_remainder_and_empty_slices(sf1):
    """78 whole tiles and 16 tail rows of the outer side meet 25 inner rows in 1, 4 and 7 slices of whole blocks (4 slices: 8, 8, 8 and 1
    rows; 7 slices end in a remainder-only slice, or in empty ones where a block is 8 rows): counts, sums, minima and maxima against
    numpy, and the same bytes - the groups in first-pair order - whatever the slice count"""
    db, made = sf1
    plan = _supplier_x_nation_plan(db)
    got = {}
    for s in (1, 4, 7):
        ctx, tabs = made[s]
        res, used, _ = _run(ctx, [tabs["nation"], tabs["supplier"]], plan, text=False)
        assert used == s
        got[s] = res
    acct = _raw(db["supplier"].col("s_acctbal"))              # DECIMAL(12, 2): hundredths
    nk = _raw(db["nation"].col("n_nationkey"))
    rk = _raw(db["nation"].col("n_regionkey"))
    assert len(acct) == 10000 and len(acct) >> 7 == 78 and len(acct) & 127 == 16 and len(nk) == 25
    want = {}
    for j in range(len(nk)):
        m = acct < nk[j] * 100 * 100
        if not m.any():
            continue
        c, sm, lo, hi = want.get(int(rk[j]), (0, 0, None, None))
        v = acct[m]
        want[int(rk[j])] = (c + int(m.sum()), sm + int(v.sum()), int(v.min()) if lo is None else min(lo, int(v.min())),
                            int(v.max()) if hi is None else max(hi, int(v.max())))
    assert len(want) == 5
    rows = sorted(tuple(int(x) for x in r) for r in got[1].rows())
    assert rows == sorted((k,) + v for k, v in want.items())
    assert got[1].tuples == got[4].tuples == got[7].tuples and len(got[1].tuples) > 0


def test_25_outer_x_10000_inner_grouped_by_a_string(sf1):
    """tail rows only on the outer side, a string key in the hash form; the launch chooses the slices itself"""
    db, made = sf1
    sql = "select n_name, count(*), sum(s_acctbal) from supplier, nation where s_acctbal < n_nationkey * 100 group by n_name"
    ctx, tabs = made[0]
    res, used, _ = _run(ctx, [tabs["nation"], tabs["supplier"]], sql, text=False)
    # one workgroup's worth of outer rows, thousands of workgroups allowed: the floor on inner rows per slice decides
    assert used == engine.nested_loops_slices(1, 1024, 10000, 0) and used >= 2
    acct = _raw(db["supplier"].col("s_acctbal"))
    nk = _raw(db["nation"].col("n_nationkey"))
    nn = [bytes(np.asarray(v).tobytes()).split(b"\0", 1)[0].rstrip(b" ") for v in np.asarray(db["nation"].col("n_name").data)]
    want = []
    for j in range(len(nk)):
        m = acct < nk[j] * 100 * 100
        if m.any():
            want.append((nn[j], int(m.sum()), int(acct[m].sum())))
    assert len(want) >= 20
    assert sorted((a.rstrip(b" "), int(b), int(c)) for a, b, c in res.rows()) == sorted(want)
    one, used1, _ = _run(made[1][0], [made[1][1]["nation"], made[1][1]["supplier"]], sql, text=False)
    assert used1 == 1 and one.tuples == res.tuples


def test_probe_below_a_split_pair_loop(small, small_db):
    """the outer side is a hash join's probe pipeline: every slice probes for every outer row, and pairs its matches with its inner rows"""
    sql = ("select r_name, count(*), sum(s_acctbal) from region, supplier, nation where s_nationkey = n_nationkey and n_nationkey < 9 "
           "group by r_name")
    sk = _raw(small_db["supplier"].col("s_nationkey"))
    acct = _raw(small_db["supplier"].col("s_acctbal"))
    rn = [bytes(np.asarray(v).tobytes()).split(b"\0", 1)[0].rstrip(b" ") for v in np.asarray(small_db["region"].col("r_name").data)]
    want = sorted((n, int((sk < 9).sum()), int(acct[sk < 9].sum())) for n in rn)
    assert want[0][1] > 10
    tuples = set()
    for s in SLICES:
        res, used, _ = _run(*small[s], sql, text=False)
        assert used == (s or 1)                          # (5 inner rows: the launch that chooses does not split)
        assert sorted((a.rstrip(b" "), int(b), int(c)) for a, b, c in res.rows()) == want
        tuples.add(res.tuples)
    assert len(tuples) == 1


def test_accessor_for_pipelines_that_are_not_split(small):
    ctx, tabs = small[64]
    res, used, _ = _run(ctx, tabs, "select r_name, n_name from region, nation")
    assert res.n_rows == 125 and used == 1               # a materialisation keeps the whole range
    res, used, _ = _run(ctx, tabs, "select count(*) from nation")
    assert used == 0                                     # no nested-loops join in the plan


def test_slices_do_not_add_launches(small):
    sql = GOLD["cases"][AGGREGATED[0]]["sql"]
    kernels = {s: _run(*small[s], sql)[2] for s in (1, 3)}
    assert kernels[1] == kernels[3] > 0


def test_two_executions_give_identical_bytes(small):
    ctx, tabs = small[3]
    q = ctx.sql_compile("select r_name, count(*) from supplier, region where s_nationkey < r_regionkey * 5 group by r_name", tabs)
    try:
        q.execute()
        a = q.result(text=False).tuples
        q.execute()
        b = q.result(text=False).tuples
        assert a == b and len(a) > 0 and q.nested_loops_slices() == 3
    finally:
        q.close()


def test_shards_slice_their_own_launches(small, small_db):
    """two shards on one GPU, every table replicated: each shard pairs its slice of the outer rows with the inner rows in 3 slices"""
    sql = "select r_name, count(*) from supplier, region where s_nationkey < r_regionkey * 5 group by r_name"
    ctx, tabs = small[1]
    want, _, _ = _run(ctx, tabs, sql)
    host = [small_db[k] for k in GOLD["tables"]]
    plan = ctx.sql_plan(sql, tabs, host)
    m = engine.MultiContext([0, 0], engine_flags=FLAG, nested_loops_inner_slices=3)
    try:
        per = [[m.shards[i].table(t) for t in host] for i in range(2)]
        q = m.compile(plan, per)
        q.execute()
        got = q.result()
        q.close()
        assert got.text == want.text and got.tuples == want.tuples
        assert want.text == next(c["result"] for c in GOLD["cases"] if c["sql"] == sql)
    finally:
        m.close()
