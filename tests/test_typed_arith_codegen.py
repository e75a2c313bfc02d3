"""tests/typedcases.py before any kernel runs, and the texts the code generator gives the register aggregation over narrow scan
columns: i32 decode exactly where the envelope fits 31 bits, each product at the width its envelope proves (32-bit, 24-bit builtin,
widening 32 x 32 -> 64, or the i64 rsq::mul of before), one text per envelope class, today's text without narrow scans, behind a wave
compaction and over a derived table, the i64 first-row tracker from 2^32 - 1 rows on, and TPC-H Q1's register count."""
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

from oracle import orc
from resql_amd import plan as P, tpch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import narrowcases as N  # noqa: E402
import typedcases as X  # noqa: E402

T = P.TypeInit
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FORMS = ("i32 n_", "fr_0", "__umul24", "__mul24", "(u64)(u32)", "const i32 in", "(i64)(n_")


@pytest.fixture(scope="module")
def ctx(tmp_path_factory):
    from resql_amd import engine
    c = engine.Context(device=-1, cache_dir=str(tmp_path_factory.mktemp("kcache_typed_arith")))
    yield c
    c.close()


def _source(ctx, plan, prepare=None):
    tabs = [ctx.table(t) for t in plan.tables]
    if prepare:
        prepare(tabs)
    q = ctx.compile(plan, tabs)
    try:
        return q.source, q.explain
    finally:
        q.close()
        for t in tabs:
            t.close()


def _table(n=600, seed=1, **ranges):
    """g: three groups; every other column DECIMAL(15, 2), random over its (lo, hi) with both ends present"""
    rng = np.random.default_rng(seed)
    cols = [P.Column("g", T.BIGINT(), rng.integers(0, 3, n).astype(np.int64))]
    for name, (lo, hi) in ranges.items():
        v = [lo + int(x) for x in rng.integers(0, hi - lo + 1, n, dtype=np.uint64)]
        v[0], v[1] = lo, hi
        cols.append(P.Column(name, X.DEC, X._dec(v)))
    return P.Table("t", cols, n)


def _input(src, w=1):
    return re.search(r"const (i32|i64) in%d = (.*);" % w, src).group(1, 2)


# ---- decode type ------------------------------------------------------------------------------------------------------------------
M31 = (1 << 31) - 1


@pytest.mark.parametrize("lo,hi,narrow", [(M31 - 200, M31, True), (M31 - 199, M31 + 1, False), (-M31, -M31 + 200, True), (-M31 - 1, -M31 + 199, False)])
def test_decode_type_at_the_i32_boundary(ctx, lo, hi, narrow):
    src, _ = _source(ctx, X.plan([X.col("c")], _table(c=(lo, hi))))
    assert "const u8* c1;" in src                                         # a one-byte image either way
    if narrow:
        assert ", i32 n_1)" in src and "rsq::dec<i32>(a.c1[r], a.fb1)" in src and "const i64 v_1 = (i64)n_1;" in src
    else:
        assert ", i64 v_1)" in src and "rsq::dec<i64>(a.c1[r], a.fb1)" in src and "n_1" not in src
    assert ", i32 n_0" in src and "rsq::ld2n(a.c0 + b, a.fb0" in src      # (the group column: two bits)


# ---- product classes --------------------------------------------------------------------------------------------------------------
def _bits(b, negative=False):
    m = (1 << b) - 1
    return (-m if negative else 0, m)


def test_products_that_fit_32_bits(ctx):
    src, _ = _source(ctx, X.plan([X.ONE_PRODUCT], _table(c=_bits(24), d=_bits(7))))
    ty, text = _input(src)
    # 1.00 - d is between -27 and 100: a signed factor, so no unsigned 24-bit multiply, and c is past 23 bits: no signed one either
    assert ty == "i64" and text == "((i64)((n_1 * (((i32)100) - n_2))))"
    src, _ = _source(ctx, X.plan([X.mul(X.col("c"), X.col("d"))], _table(c=_bits(24), d=_bits(7))))
    assert _input(src)[1] == "((i64)(((i32)__umul24((u32)(n_1), (u32)(n_2)))))"
    src, _ = _source(ctx, X.plan([X.mul(X.col("c"), X.col("d"))], _table(c=_bits(23, True), d=_bits(7, True))))
    assert _input(src)[1] == "((i64)(__mul24(n_1, n_2)))"
    src, _ = _source(ctx, X.plan([X.mul(X.col("c"), X.col("d"))], _table(c=_bits(24, True), d=_bits(7, True))))
    assert _input(src)[1] == "((i64)((n_1 * n_2)))"


@pytest.mark.parametrize("c_bits,d_bits", [(24, 8), (25, 7)])
def test_products_one_bit_past_32_widen(ctx, c_bits, d_bits):
    src, _ = _source(ctx, X.plan([X.ONE_PRODUCT], _table(c=_bits(c_bits), d=_bits(d_bits))))
    assert _input(src) == ("i64", "((i64)(n_1) * (i64)((((i32)100) - n_2)))")                  # signed: 1.00 - d may be negative
    src, _ = _source(ctx, X.plan([X.mul(X.col("c"), X.col("d"))], _table(c=_bits(c_bits), d=_bits(d_bits))))
    assert _input(src) == ("i64", "((i64)((u64)(u32)(n_1) * (u64)(u32)(n_2)))")                # both non-negative: unsigned


def test_second_product_widens_the_first(ctx):
    src, _ = _source(ctx, X.plan([X.TWO_PRODUCTS], _table(c=_bits(24), d=_bits(7), e=_bits(7))))
    assert _input(src) == ("i64", "((i64)((n_1 * (((i32)100) - n_2))) * (i64)((((i32)100) + n_3)))")
    assert "rsq::mul(" not in src


def test_a_33_bit_operand_keeps_the_i64_multiply(ctx):
    src, _ = _source(ctx, X.plan([X.mul(X.col("c"), X.col("w"))], _table(c=_bits(24), w=((1 << 32) - 100, 1 << 32))))
    assert ", i32 n_1, i64 v_2)" in src
    assert _input(src) == ("i64", "rsq::mul(((i64)(n_1)), v_2)")


def test_inputs_of_partial_sums_are_i32_and_of_i64_accumulators_keep_their_type(ctx):
    src, ex = _source(ctx, X.plan([X.col("c"), X.col("w")], _table(c=_bits(24), w=_bits(25))))
    assert _input(src, 1) == ("i32", "n_1") and "i32 p32_1_0 = 0;" in src
    assert _input(src, 2) == ("i64", "((i64)(n_2))") and "p32_2_" not in src and "st.acc_2_0 = rsq::add(st.acc_2_0, in2);" in src
    assert "32-bit partial sums folded every 32 tiles" in ex


# ---- one text per envelope class --------------------------------------------------------------------------------------------------
def test_same_text_across_statistics_of_one_class(ctx):
    a = _table(n=600, seed=1, c=_bits(24), d=_bits(7), e=_bits(7))
    b = _table(n=5000, seed=2, c=((1 << 23) + 5, (1 << 24) - 3), d=(3, 100), e=(64, 90))
    for exprs in X.STATEMENTS.values():
        assert _source(ctx, X.plan(exprs, a))[0] == _source(ctx, X.plan(exprs, b))[0]


# ---- where nothing changes --------------------------------------------------------------------------------------------------------
def test_wide_sources_have_none_of_the_new_forms(ctx, monkeypatch):
    t = X.product_table(24, 7, 7, False, n=300)
    assert all(f in _source(ctx, X.plan([X.TWO_PRODUCTS, X.mul(X.col("c"), X.col("d")), X.col("d")], t))[0] for f in NEW_FORMS if f not in ("__mul24", "(u64)(u32)", "(i64)(n_"))
    monkeypatch.setenv("RSQ_NARROW_SCANS", "0")
    for exprs in list(X.STATEMENTS.values()) + [[X.mul(X.col("c"), X.col("d"))]]:
        src, _ = _source(ctx, X.plan(exprs, t))
        assert not [f for f in NEW_FORMS if f in src]
        assert "st.acc_0_0 = row < st.acc_0_0 ? row : st.acc_0_0;" in src and "rsq::mul(v_1, " in src


def test_behind_a_wave_compaction_and_over_a_derived_table(ctx):
    t = N.p32_table(0, N.P32_MAX)
    r = P.Table("r", [P.Column("rk", T.BIGINT(), np.arange(0, 2000, 2, dtype=np.int64))], 1000)
    p = P.Plan([r, t])                                                    # select b, sum(c * a), count(*) from r, t where rk = a and a < 30 group by b
    probe = p.selection(p.lt(p.attr("a"), p.constant("30", P.BIGINT)), p.scan("t"))
    j = p.hashjoin([p.eq(p.attr("rk"), p.attr("a"))], p.scan("r"), probe, single_match=True)
    sc, cn = p.sum(p.mul(p.attr("c"), p.attr("a"))), p.count(p.star())
    p.set_root(p.materialize(p.projection([p.attr("b"), p.as_("s", sc), p.as_("n", cn)], p.aggregation([sc, cn], [p.attr("b")], j))))
    src, ex = _source(ctx, p)
    assert "wave compaction" in ex and "in registers" in ex and not [f for f in NEW_FORMS if f in src]
    p = P.Plan([t])
    cnt = p.count(p.star())
    inner = p.aggregation([cnt], [p.attr("a")], p.scan("t"))
    p.set_root(p.materialize(p.aggregation([p.sum(cnt), p.count(p.star())], [], inner)), request_all=True)
    src, ex = _source(ctx, p)
    outer = src.split("// generated by")[-1]                             # (the pipeline over the derived table)
    assert "scan derived0" in ex and "in registers" in ex and not [f for f in NEW_FORMS if f in outer]


# ---- the reference ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("cid,c_bits,d_bits,e_bits", X.PRODUCT_CASES, ids=[c[0] for c in X.PRODUCT_CASES])
def test_reference_is_the_oracle_on_the_products(cid, c_bits, d_bits, e_bits, negative):
    t = X.product_table(c_bits, d_bits, e_bits, negative)
    for exprs in X.STATEMENTS.values():
        want = orc.execute(X.plan(exprs, t))
        assert sorted(want.rows()) == X.reference(exprs, t) and want.n_rows == 3


@pytest.mark.parametrize("n", X.FIRST_ROW_N)
def test_reference_is_the_oracle_on_the_first_row_tables(n):
    t = X.first_row_table(n)
    want = orc.execute(X.plan(X.FIRST_ROWS, t))
    assert sorted(want.rows()) == X.reference(X.FIRST_ROWS, t) and want.n_rows == 5      # (group 3 is absent)


# ---- the first-row tracker's row-count class --------------------------------------------------------------------------------------
def test_first_row_tracker_is_i64_from_2_to_the_32_minus_1_rows(ctx):
    """a shard that plans as a table of 2^32 + n rows (the row count rsq_table_unify_shard_stats takes from the shards' blobs)"""
    t = X.first_row_table(300)
    src, _ = _source(ctx, X.plan(X.FIRST_ROWS, t))
    assert "u32 fr_0 = 0xffffffffu;" in src and "st.fr_5 = (u32)lr < st.fr_5 ? (u32)lr : st.fr_5;" in src
    assert "st.acc_0_5 = st.fr_5 == 0xffffffffu ? (i64)0x7fffffffffffffffull : a.row0 + (i64)st.fr_5;" in src

    def huge(tabs):
        own = tabs[0].stats_blob()
        other = bytearray(own)
        struct.pack_into("<qq", other, 16, t.n_rows, 1 << 32)            # [magic | columns | row0 | rows]: the rows behind this shard
        tabs[0].unify_shard_stats([own, bytes(other)])
        assert tabs[0].total_rows >= (1 << 32) - 1
    big, _ = _source(ctx, X.plan(X.FIRST_ROWS, t), huge)
    assert "fr_" not in big and "st.acc_0_5 = row < st.acc_0_5 ? row : st.acc_0_5;" in big
    assert ", i32 n_1)" in big                                           # (the arithmetic stays typed)


# ---- TPC-H Q1 at the ISA level ----------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc is missing")
def test_q1_compiles_without_scratch_in_no_more_registers_than_before(ctx, tmp_path):
    li = tpch.lineitem_table(0.01, tpch.Q1_COLUMNS)
    src, _ = _source(ctx, tpch.q1_plan(li))
    assert "const i64 nt = tt0 + nwaves" in src                           # the software-pipelined loop
    (tmp_path / "q1.hip").write_text(src)
    out = subprocess.run([os.path.join(ROOT, "tools", "isa.sh"), str(tmp_path / "q1.hip"), str(tmp_path / "q1.s")],
                         capture_output=True, text=True, check=True).stdout
    assert int(re.search(r"ScratchSize: (\d+)", out).group(1)) == 0
    assert int(re.search(r"NumVgprs: (\d+)", out).group(1)) <= 216


def test_a_case_input_keeps_its_text_and_its_truth_tables(ctx, monkeypatch):
    """an input that is not +, -, * over columns and constants alone is emitted once, as before: the truth tables over a
    dictionary-coded column that answer a CASE condition exist only during that first emission"""
    import dictcases as D
    monkeypatch.setenv("RSQ_DICT_SCANS", "1")
    host = D.table(3000, T.CHAR(9), D.edge_values(9, 40))
    dt = ctx.table(host)
    try:
        q = ctx.sql_compile(D.PREDICATES["case"], [dt])
        src = q.source
        q.close()
    finally:
        dt.close()
    assert "dict_bit" in src and "in registers" in src.split("\n")[2] and "i32 n_" in src
