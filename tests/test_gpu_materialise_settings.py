"""The three device tails of a materialisation under every combination of their setters (Context.set_order_limit, set_order_sort,
set_result_pack; engine_mattail.cpp runMaterializeDeviceTail).  The precedence - order_limit decides first, then order_sort, then
result_pack - is spelt out here once, in Python, and every combination's reports and launch count are derived from the three runs with
one setter on: nothing expected is written by hand.  Five statements of tests/ordersortcases.py, one per way the decision can go; every
answer is held against the CPU oracle's."""
import itertools

import pytest

from resql_amd import engine
from oracle import orc

import ordersortcases as S

pytestmark = pytest.mark.gpu

# (statement, table): sort decides; order_limit decides; order_limit overflows and sort decides; sort's TIES; SMALL for sort and pack
CASES = [S.DEVICE[0][:2], S.DEVICE[8][:2], S.DEVICE[9][:2], S.HOST[0][:2], S.HOST[4][:2]]
IDS = ["sort", "limit", "overflow", "ties", "small"]
OFF = (0, 0, 0)


@pytest.fixture(scope="module")
def world(gpu_ctx):
    names = sorted({name for _, name in CASES})
    host = {k: S.TABLES[k]() for k in names}
    tabs = {k: gpu_ctx.table(v) for k, v in host.items()}
    yield gpu_ctx, tabs, host
    for t in tabs.values():
        t.close()


@pytest.fixture(autouse=True)
def setters_back_at_the_default(gpu_ctx):
    yield
    gpu_ctx.set_order_sort(engine.ORDER_SORT_HOST)          # (the context is the session's)
    gpu_ctx.set_order_limit(engine.ORDER_LIMIT_HOST)
    gpu_ctx.set_result_pack(engine.RESULT_PACK_HOST)


def run(ctx, q, settings):
    """one execution under (order_limit, order_sort, result_pack) -> (result, the three reports, launches)"""
    limit, sort, pack = settings
    ctx.set_order_limit(limit)
    ctx.set_order_sort(sort)
    ctx.set_result_pack(pack)
    q.execute()
    return q.result(), (q.order_limit_report(), q.order_sort_report(), q.result_pack_report()), q.report().num_kernels


def decision(rep):
    return rep["path"], rep["fallback_reason"]


def without_times(rep):
    return {k: v for k, v in rep.items() if not k.endswith("_ms")}


@pytest.mark.parametrize("sql,name", CASES, ids=IDS)
def test_every_combination_follows_the_precedence(world, sql, name):
    ctx, tabs, host = world
    want = orc.execute(ctx.sql_plan(sql, [tabs[name]], [host[name]]))
    q = ctx.sql_compile(sql, [tabs[name]])
    try:
        run(ctx, q, OFF)          # (every execution measured below is warm)
        got, off, kernels0 = run(ctx, q, OFF)
        assert got.text == want.text and got.tuples == want.tuples
        assert [decision(r) for r in off] == [(0, 0)] * 3
        alone, launches = [], []          # of the run with this one setter on: its report's decision, its launches
        for stage in range(3):
            got, reps, kernels = run(ctx, q, tuple(int(s == stage) for s in range(3)))
            assert got.text == want.text and got.tuples == want.tuples, (sql, stage)
            assert [decision(r) for s, r in enumerate(reps) if s != stage] == [(0, 0)] * 2
            alone.append(decision(reps[stage]))
            launches.append(kernels - kernels0)
        assert all(n >= 0 for n in launches)
        for limit, sort, pack in itertools.product((0, 1), repeat=3):
            got, (rl, rs, rp), kernels = run(ctx, q, (limit, sort, pack))
            assert got.text == want.text and got.tuples == want.tuples, (sql, limit, sort, pack)
            # the precedence: order_limit decides first, then order_sort, then result_pack
            limit_decided = bool(limit) and alone[0][0] == 1
            sort_ran = bool(sort) and not limit_decided
            sort_decided = sort_ran and alone[1][0] == 1
            pack_ran = bool(pack) and not limit_decided and not sort_decided
            want_limit = alone[0] if limit else (0, engine.ORDER_LIMIT_FALLBACK_NONE)
            want_sort = (0, engine.ORDER_SORT_FALLBACK_NONE) if not sort else (0, engine.ORDER_SORT_FALLBACK_ORDER_LIMIT) if limit_decided else alone[1]
            want_pack = ((0, engine.RESULT_PACK_FALLBACK_NONE) if not pack else (0, engine.RESULT_PACK_FALLBACK_ORDER_LIMIT) if limit_decided else
                         (0, engine.RESULT_PACK_FALLBACK_SHAPE) if sort_decided else alone[2])
            assert (decision(rl), decision(rs), decision(rp)) == (want_limit, want_sort, want_pack), (sql, limit, sort, pack, rl, rs, rp)
            if pack and sort_decided:          # the relation the sort's path made
                assert (rp["rows"], rp["tuple_bytes"]) == (want.n_rows, len(want.tuples))
            assert kernels == kernels0 + limit * launches[0] + sort_ran * launches[1] + pack_ran * launches[2], (sql, limit, sort, pack)
    finally:
        q.close()


@pytest.mark.parametrize("sql,name", CASES, ids=IDS)
def test_an_execution_with_all_off_reports_as_if_none_had_been_on(world, sql, name):
    ctx, tabs, _ = world
    used, fresh = ctx.sql_compile(sql, [tabs[name]]), ctx.sql_compile(sql, [tabs[name]])
    try:
        run(ctx, used, (1, 1, 1))
        _, after, _ = run(ctx, used, OFF)
        _, never, _ = run(ctx, fresh, OFF)
        assert [without_times(r) for r in after] == [without_times(r) for r in never]
        assert all(v == 0 for r in after + never for k, v in r.items() if k.endswith("_ms"))
    finally:
        used.close()
        fresh.close()
