"""The texts the code generator gives the register aggregation's 32-bit partial sums since they fold into the workgroup's LDS image
(tests/ldsfoldcases.py): no i64 register for such an accumulator, the image filled in front of the tile loop, every other accumulator
and every text without partial sums as before, the launch bound only where the statement's registers leave room for it, and TPC-H
Q1's kernel within 128 VGPRs without scratch memory."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from resql_amd import plan as P, tpch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import narrowcases as N  # noqa: E402
import typedcases as X  # noqa: E402
import ldsfoldcases as L  # noqa: E402

T = P.TypeInit
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FORMS = ("(u64)(i64)st.p32_", "RSQ_MIN_WG 4")
hipcc = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc is missing")


@pytest.fixture(scope="module")
def ctx(tmp_path_factory):
    from resql_amd import engine
    c = engine.Context(device=-1, cache_dir=str(tmp_path_factory.mktemp("kcache_lds_fold")))
    yield c
    c.close()


def _source(ctx, plan):
    tabs = [ctx.table(t) for t in plan.tables]
    q = ctx.compile(plan, tabs)
    try:
        return q.source, q.explain
    finally:
        q.close()
        for t in tabs:
            t.close()


def _isa(tmp_path, name, src):
    (tmp_path / (name + ".hip")).write_text(src)
    out = subprocess.run([os.path.join(ROOT, "tools", "isa.sh"), str(tmp_path / (name + ".hip")), str(tmp_path / (name + ".s"))],
                         capture_output=True, text=True, check=True).stdout
    return {k: int(re.search(k + r": (\d+)", out).group(1)) for k in ("ScratchSize", "NumVgprs", "Occupancy")}


def _loop_at(src):
    return src.index("    for (i64 t = wave * tstep; t < ntiles;")


# ---- the fold ---------------------------------------------------------------------------------------------------------------------
def test_partial_sums_fold_into_the_lds_image(ctx):
    """FOLD_MIXED: sum(c) and the count take partial sums (accumulators 1 and 3), sum(e) is one bit past the bound (accumulator 2)"""
    src, ex = _source(ctx, N.plan(N.FOLD_MIXED, [N.fold_table(4 * N.TILE + 77, "pos", 3)]))
    assert "in registers, 32-bit partial sums folded every 32 tiles" in ex
    for w in (1, 3):
        for g in range(3):
            cell = (w * 3 + g) * 64                                       # (the blocks of this statement stand in accumulator order)
            assert f"rsq::lds_merge<0>(&s_lane[{cell} + (threadIdx.x & 63)], (u64)(i64)st.p32_{w}_{g}); st.p32_{w}_{g} = 0;" in src
            assert f"i32 p32_{w}_{g} = 0;" in src
            assert f"acc_{w}_{g}" not in src                              # neither the register nor its merge in the epilogue
    # the period and its counter are what they were; the fold stands behind every tile of the loop and once behind the tail rows
    fold = re.findall(r"^ +(?:if \(\+\+st\.fold_n == 32\) \{ st\.fold_n = 0; )?rsq::lds_merge<0>\(&s_lane\[192 .*$", src, re.M)
    assert len(fold) == 3 and sum("++st.fold_n == 32" in f for f in fold) == 2 and "int fold_n = 0;" in src
    tail_fold = src.index(fold[-1])
    assert tail_fold > src.index("r < a.n_rows; r += (i64)gridDim.x * blockDim.x") and "fold_n" not in fold[-1]
    # sum(e) and the first rows keep their registers and their merges
    assert "i64 acc_2_0 = (i64)0ull;" in src and "st.acc_2_0 = rsq::add(st.acc_2_0, in2);" in src
    assert "rsq::lds_merge<0>(&s_lane[384 + (threadIdx.x & 63)], (u64)st.acc_2_0);" in src
    assert "rsq::lds_merge<2>(&s_lane[0 + (threadIdx.x & 63)], (u64)st.acc_0_0);" in src
    assert src.index("(u64)st.acc_2_0);") > tail_fold


def test_the_image_is_filled_behind_a_barrier_in_front_of_the_tile_loop(ctx):
    src, _ = _source(ctx, N.plan(L.MINMAX, [L.minmax_table(300)]))
    decl = src.index("__shared__ u64 s_lane[1920];")                      # 5 blocks x 6 groups x 64 lanes
    fill = src.index("s_lane[i] = blk < 2 ? 0x7fffffffffffffffull : blk < 3 ? 0x8000000000000000ull : 0ull;")
    barrier = src.index("__syncthreads();", fill)
    assert decl < fill < barrier < _loop_at(src) < src.index("if (++st.fold_n == 32)")
    assert src.count("__shared__ u64 s_lane[") == 1 and src.count("s_lane[i] = ") == 1
    # min and max keep their identities in the image until the epilogue merges their registers
    for w, op in ((3, 2), (4, 3)):
        for g in range(6):
            assert f"i64 acc_{w}_{g} = (i64)" in src
            assert re.search(rf"rsq::lds_merge<{op}>\(&s_lane\[\d+ \+ \(threadIdx\.x & 63\)\], \(u64\)st\.acc_{w}_{g}\);", src)
    assert "acc_1_" not in src and "acc_2_" not in src
    assert src.index("(u64)st.acc_3_0);") > src.index("r < a.n_rows; r += (i64)gridDim.x * blockDim.x")


def test_the_late_load_form_folds_the_same_way_and_keeps_its_grid(ctx):
    src, ex = _source(ctx, N.plan(N.late_statement(), [N.late_table(40_000)]))
    assert "late loads" in ex and "(u64)(i64)st.p32_" in src and "RSQ_MIN_WG 4" not in src
    assert src.index("s_lane[i] = ") < src.index("    for (i64 t = wave * tstep;")


# ---- where nothing changes --------------------------------------------------------------------------------------------------------
def test_texts_without_partial_sums_have_none_of_the_new_forms(ctx, monkeypatch):
    def old_form(src):
        assert not [f for f in NEW_FORMS if f in src] and "p32_" not in src
        assert src.index("__shared__ u64 s_lane[") > _loop_at(src)      # the image is the epilogue's alone
    # an accumulator past 24 bits on its own (no count): no partial sum in the statement
    t = N.fold_table(4 * N.TILE + 77, "pos", 3)
    old_form(_source(ctx, N.plan(N.Statement([("sum", "e"), ("min", "c")], ["b"]), [t]))[0])
    # behind a wave compaction and over a derived table (tests/test_typed_arith_codegen.py's statements)
    pt = N.p32_table(0, N.P32_MAX)
    r = P.Table("r", [P.Column("rk", T.BIGINT(), np.arange(0, 2000, 2, dtype=np.int64))], 1000)
    p = P.Plan([r, pt])
    probe = p.selection(p.lt(p.attr("a"), p.constant("30", P.BIGINT)), p.scan("t"))
    j = p.hashjoin([p.eq(p.attr("rk"), p.attr("a"))], p.scan("r"), probe, single_match=True)
    sc, cn = p.sum(p.attr("c")), p.count(p.star())
    p.set_root(p.materialize(p.projection([p.attr("b"), p.as_("s", sc), p.as_("n", cn)], p.aggregation([sc, cn], [p.attr("b")], j))))
    src, ex = _source(ctx, p)
    assert "wave compaction" in ex and "in registers" in ex
    old_form(src.split("// generated by")[-1])
    p = P.Plan([pt])
    cnt = p.count(p.star())
    inner = p.aggregation([cnt], [p.attr("a")], p.scan("t"))
    p.set_root(p.materialize(p.aggregation([p.sum(cnt), p.count(p.star())], [], inner)), request_all=True)
    src, ex = _source(ctx, p)
    assert "scan derived0" in ex and "in registers" in ex
    old_form(src.split("// generated by")[-1])
    # narrow scans off
    monkeypatch.setenv("RSQ_NARROW_SCANS", "0")
    for plan in (N.plan(N.FOLD_MIXED, [t]), tpch.q1_plan(tpch.lineitem_table(0.01, tpch.Q1_COLUMNS))):
        src, ex = _source(ctx, plan)
        assert "in registers" in ex and "partial sums" not in ex
        old_form(src)


def test_max_grid_changes_no_text(ctx, monkeypatch):
    plans = [tpch.q1_plan(tpch.lineitem_table(0.01, tpch.Q1_COLUMNS)), N.plan(L.MINMAX, [L.minmax_table(300)]),
             N.plan(N.FOLD_GROUPED, [N.fold_table(4 * N.TILE + 77, "neg", 3)])]
    for plan in plans:
        texts = []
        for g in (None, "1", "4"):
            if g:
                monkeypatch.setenv("RSQ_MAX_GRID", g)
            else:
                monkeypatch.delenv("RSQ_MAX_GRID", raising=False)
            texts.append(_source(ctx, plan)[0])
        monkeypatch.delenv("RSQ_MAX_GRID", raising=False)
        assert len(set(texts)) == 1 and "#define RSQ_BLOCK_THREADS 512" in texts[0]


# ---- registers ----------------------------------------------------------------------------------------------------------------------
@hipcc
def test_q1_fits_two_workgroups_per_cu_without_scratch(ctx, tmp_path):
    src, ex = _source(ctx, tpch.q1_plan(tpch.lineitem_table(0.01, tpch.Q1_COLUMNS)))
    assert "const i64 nt = tt0 + nwaves" in src and "#define RSQ_MIN_WG 4\n" in src      # the pipelined loop, held to four waves per SIMD
    assert "(u64)(i64)st.p32_1_0)" in src and "acc_1_0" not in src and "i64 acc_3_0 = (i64)0ull;" in src
    r = _isa(tmp_path, "q1", src)
    assert r["ScratchSize"] == 0 and r["NumVgprs"] <= 128 and r["Occupancy"] >= 4


def _grouped(groups, aggs, n=3000):
    """b: `groups` groups by row; c: the 24-bit envelope, both signs; d: 0..999"""
    rng = np.random.default_rng(1)
    t = P.Table("t", [P.Column("b", T.BIGINT(), (np.arange(n) % groups).astype(np.int64)),
                      P.Column("c", T.BIGINT(), rng.integers(-N.P32_MAX, N.P32_MAX + 1, n).astype(np.int64)),
                      P.Column("d", T.BIGINT(), rng.integers(0, 1000, n).astype(np.int64))], n)
    return N.plan(N.Statement(aggs, ["b"]), [t])


@hipcc
@pytest.mark.parametrize("groups,aggs,tiles", [
    (8, [("sum", "c"), ("sum", "d"), ("count", None), ("min", "c")], 2),      # 48 + 2 x 2 x 6 + 32 = 104: exactly at the limit
    (11, [("sum", "c"), ("sum", "d"), ("count", None)], 1),                   # 112 with two tiles: gives one up, 100
], ids=["g8_4acc", "g11_3acc"])
def test_statements_at_the_limit_of_the_rule_take_the_bound_without_scratch(ctx, tmp_path, groups, aggs, tiles):
    """the other side of the margin: the largest statements the register rule still gives the launch bound fit 128 VGPRs"""
    src, _ = _source(ctx, _grouped(groups, aggs))
    assert "#define RSQ_MIN_WG 4\n" in src and f"t += nwaves * tstep * {tiles})" in src
    r = _isa(tmp_path, "limit", src)
    assert r["ScratchSize"] == 0 and r["NumVgprs"] <= 128 and r["Occupancy"] >= 4


@hipcc
@pytest.mark.parametrize("name", ["cells64", "g9_5acc", "g16_sums"])
def test_no_statement_pays_scratch_for_the_launch_bound(ctx, tmp_path, name):
    """statements whose registers leave no room for four waves per SIMD: held to 128 VGPRs they would spill (9 groups x 5 accumulators
    did, by 12 bytes, under a looser rule); they get the fold, no bound, and keep their grid"""
    if name == "cells64":
        plan = N.plan(L.CELLS64, [L.cells64_table(300)])
    else:
        plan = _grouped(*{"g9_5acc": (9, [("sum", "c"), ("sum", "d"), ("count", None), ("min", "c"), ("max", "d")]),
                          "g16_sums": (16, [("sum", "c"), ("sum", "d"), ("count", None)])}[name])
    src, _ = _source(ctx, plan)
    assert "(u64)(i64)st.p32_" in src and "RSQ_MIN_WG 4" not in src
    if name == "cells64":
        assert "__shared__ u64 s_lane[4096];" in src                      # 64 cells: 32 KB
    assert _isa(tmp_path, name, src)["ScratchSize"] == 0
