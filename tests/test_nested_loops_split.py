"""Inner-range slices of a nested-loops join's pair loop: the policy (rsq_nested_loops_slices), the configuration field
(rsq_config.nested_loops_inner_slices), and what the generated text and the explain line hold - for an aggregating statement, whose
launch splits the inner rows across workgroups, and for a materialising one, which keeps the whole range.  No GPU needed."""
import json
import os

import pytest

from resql_amd import engine, tpch_full

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "nlj_reference.json")) as f:
    GOLD = json.load(f)

AGGREGATING = "select r_name, count(*) from supplier, region where s_nationkey < r_regionkey * 5 group by r_name"
MATERIALISING = "select r_name, n_name from region, nation"
NOTE = " [inner range split across workgroups at launch]"
FLOOR = engine.NLJ_MIN_SLICE_ROWS


def _header_floor():
    import re
    with open(os.path.join(os.path.dirname(HERE), "include", "resql_hip.h")) as f:
        return int(re.search(r"#define\s+RSQ_NLJ_MIN_SLICE_ROWS\s+(\d+)", f.read()).group(1))


def test_the_binding_knows_the_headers_floor():
    assert FLOOR == _header_floor() and FLOOR >= 1


@pytest.mark.parametrize("base, inner, configured, want", [
    (1, 1_500_000, 0, 2048),
    (20, 1_500_000, 0, 102),
    (2048, 1_500_000, 0, 1), (2048, 1, 0, 1),
    (5000, 1_500_000, 0, 1), (5000, 0, 0, 1),
    (1, 25, 0, 1),
    (1, 0, 0, 1),
    (1, FLOOR + 1, 0, 2),
    (1, 1_500_000, 1, 1), (20, 25, 1, 1), (5000, 0, 1, 1),
    (1, 1_500_000, 7, 7), (20, 25, 7, 7), (5000, 0, 7, 7),
    (1, 1_500_000, 4096, 2048), (5000, 25, 4096, 2048),
])
def test_policy(base, inner, configured, want):
    assert engine.nested_loops_slices(base, 2048, inner, configured) == want


def test_policy_floor_is_the_exported_constant():
    """one more inner row than the floor is worth a second slice, the floor itself is not"""
    assert engine.nested_loops_slices(1, 2048, FLOOR, 0) == 1
    assert engine.nested_loops_slices(1, 2048, FLOOR + 1, 0) == 2
    assert engine.nested_loops_slices(1, 2048, 3 * FLOOR, 0) == 3


@pytest.mark.parametrize("bad", [-1, 4097])
def test_slices_outside_the_range_are_invalid(bad):
    with pytest.raises(engine.EngineError) as e:
        engine.Context(device=-1, engine_flags=engine.ENGINE_NESTED_LOOPS, nested_loops_inner_slices=bad)
    assert e.value.status == 1
    assert "nested_loops_inner_slices" in str(e.value)


def test_old_size_config_reads_the_slices_as_zero():
    """a host built against the header before nested_loops_inner_slices: the field is not read (0: chosen per execution)"""
    cfg = engine.rsq_config.make(-1, engine_flags=engine.ENGINE_NESTED_LOOPS, nested_loops_inner_slices=-5)
    cfg.struct_size = engine.rsq_config.nested_loops_inner_slices.offset
    L = engine.lib()
    h = engine.C.c_void_p()
    assert L.rsq_ctx_create(engine.C.byref(cfg), engine.C.byref(h)) == 0
    L.rsq_ctx_destroy(h)


def _texts(slices):
    """(source, explain) of the two statements on a compile-only context with this nested_loops_inner_slices"""
    ctx = engine.Context(device=-1, engine_flags=engine.ENGINE_NESTED_LOOPS, nested_loops_inner_slices=slices)
    db = tpch_full.database(GOLD["sf"])
    tabs = [ctx.table(db[k]) for k in GOLD["tables"]]
    out = {}
    try:
        for sql in (AGGREGATING, MATERIALISING):
            q = ctx.sql_compile(sql, tabs)
            out[sql] = (q.source, q.explain)
            assert q.nested_loops_slices() == 0          # (never executed)
            q.close()
    finally:
        for t in tabs:
            t.close()
        ctx.close()
    return out


@pytest.fixture(scope="module")
def texts():
    return {s: _texts(s) for s in (0, 1, 7)}


def test_aggregating_statement_takes_the_slice_count_as_an_argument(texts):
    source, explain = texts[0][AGGREGATING]
    assert "    i64 nlj0_s;\n" in source[source.index("struct Args {"):source.index("};", source.index("struct Args {"))]
    # the virtual workgroup and the slice, from the real indices and the argument ...
    assert "const u32 nlj_s = (u32)a.nlj0_s;" in source
    assert "nlj_vb = blockIdx.x / nlj_s, nlj_slice = blockIdx.x - nlj_vb * nlj_s, nlj_vg = gridDim.x / nlj_s;" in source
    # ... the outer side's tiles and tail rows dealt to the virtual ones, the pair loop over the slice, the ordinal as it was
    assert "const i64 wave = (i64)nlj_vb * (blockDim.x >> 6) + (threadIdx.x >> 6);" in source
    assert "const i64 nwaves = (i64)nlj_vg * (blockDim.x >> 6);" in source
    assert "(i64)nlj_vb * blockDim.x + threadIdx.x; r < a.n_rows; r += (i64)nlj_vg * blockDim.x" in source
    assert "nlj0_j != st.nlj0_hi; nlj0_j++" in source and "= st.nlj0_lo;" in source
    assert "const i64 row = nlj0_orow * a.nlj0_n + nlj0_j;" in source
    assert NOTE in explain


def test_aggregating_statement_loads_inner_rows_in_blocks(texts):
    source, _ = texts[0][AGGREGATING]
    assert "rsq::nlj_ld_block<i32, " in source and "#pragma unroll" in source
    assert "rsq::nlj_ld(a.nlj0_c0, nlj0_j)" in source            # the remainder loop of single rows


def test_materialising_statement_keeps_the_whole_range(texts):
    source, explain = texts[0][MATERIALISING]
    assert "nlj0_s" not in source and "nlj_vb" not in source
    assert "for (i64 nlj0_j = 0; nlj0_j < a.nlj0_n; nlj0_j++) {" in source
    assert "(i64)blockIdx.x * (blockDim.x >> 6)" in source
    assert NOTE not in explain


@pytest.mark.parametrize("sql", [AGGREGATING, MATERIALISING])
def test_text_does_not_depend_on_the_slice_count(texts, sql):
    """the slice count is a launch argument: one kernel text, one code object, whatever the context asks for"""
    assert texts[0][sql][0] == texts[1][sql][0] == texts[7][sql][0]
    assert texts[0][sql][1] == texts[1][sql][1] == texts[7][sql][1]
