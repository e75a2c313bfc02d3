"""The two forms of the register aggregation in one text (resql_amd/csrc/codegen_agg.cpp, row_cells.h): TPC-H Q1 and two relatives carry
form 1 - rows into per-lane LDS cells - under #if RSQ_ROW_CELLS; form 0 is the text a context that generates no second form gets, line for
line; statements outside the family have none of it; form 1 compiles for gfx950 without scratch memory inside its launch bound."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from resql_amd import engine, plan as P, tpch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import narrowcases as N  # noqa: E402
import ldsfoldcases as L  # noqa: E402
import rowcellscases as R  # noqa: E402

T = P.TypeInit
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
hipcc = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc is missing")
GUARD = "#ifndef RSQ_ROW_CELLS\n#define RSQ_ROW_CELLS 0\n#endif\n"


@pytest.fixture(scope="module")
def ctxs(tmp_path_factory):
    """(the default context, one that generates no second form)"""
    both = engine.Context(device=-1, cache_dir=str(tmp_path_factory.mktemp("kcache_cells")))
    off = engine.Context(device=-1, cache_dir=str(tmp_path_factory.mktemp("kcache_cells_off")))
    off.set_row_cells(0)
    yield both, off
    both.close()
    off.close()


def _source(ctx, plan):
    tabs = [ctx.table(t) for t in plan.tables]
    q = ctx.compile(plan, tabs)
    try:
        return q.source, q.explain
    finally:
        q.close()
        for t in tabs:
            t.close()


def _form(src, cells):
    """the text the preprocessor leaves of `src` with RSQ_ROW_CELLS = cells: only the lines about that macro are evaluated"""
    out, keep = [], [True]
    for line in src.split("\n"):
        if line in ("#if !RSQ_ROW_CELLS", "#if RSQ_ROW_CELLS"):
            keep.append(keep[-1] and (("!" in line) != bool(cells)))
        elif line == "#else" and len(keep) > 1:
            keep[-1] = keep[-2] and not keep[-1]
        elif line == "#endif" and len(keep) > 1:
            keep.pop()
        elif keep[-1]:
            out.append(line)
    assert keep == [True]
    return "\n".join(out)


def _family():
    return {"q1": tpch.q1_plan(tpch.lineitem_table(0.01, tpch.Q1_COLUMNS)),
            "minmax": N.plan(L.MINMAX, [L.minmax_table(300)]),
            "packed": N.plan(R.PACKED, [R.packed_table(4 * N.TILE + 77)])}


@pytest.mark.parametrize("name", ["q1", "minmax", "packed"])
def test_the_family_carries_both_forms_and_form_0_is_the_earlier_text(ctxs, name):
    both, off = ctxs
    src, ex = _source(both, _family()[name])
    old, old_ex = _source(off, _family()[name])
    assert "RSQ_ROW_CELLS" not in old and "second form" not in old_ex and "#define RSQ_MIN_WG 4\n" in old
    assert src.startswith(GUARD) and "[second form: rows into per-lane LDS cells" in ex
    # (RSQ_LAZY's and RSQ_MIN_WG's #if lines of other families would confuse _form: this family has neither an #else nor another #if inside its own)
    assert _form(src[len(GUARD):], 0) == old
    one = _form(src, 1)
    # form 1: no accumulator state, no folds, no register merges; one cell pointer and one update per word
    assert not re.search(r"\b(acc_\d+_\d+|fr_\d+|p32_\d+_\d+|fold_n)\b", one)
    assert "    u64* cells;" in one and "    st.cells = s_lane + (threadIdx.x & 63);\n" in one and "    u64* cell = st.cells + gid * 64;\n" in one
    assert "atomicMin(reinterpret_cast<u32*>(cell + 0), (u32)lr);" in one
    assert "if (gid == 0) {" not in one and "&s_lane[" not in one.split("__shared__ u64 s_acc[")[0].split("row_fn")[1]
    # the image, its fill and the epilogue from the barrier on are shared
    for text in (src, one, old):
        assert text.count("__shared__ u64 s_lane[") == 1 and text.count("s_lane[i] = ") == 1 and text.count("rsq::wave_reduce_to_lane63<0>(v)") == 1


def test_q1_packs_quantity_count_and_discount_into_one_word(ctxs):
    one = _form(_source(ctxs[0], _family()["q1"])[0], 1)
    assert "rsq::lds_merge<0>(cell + 384, (u64)(u32)in1 | (u64)(u32)in5 << 21 | (u64)(u32)in6 << 42);" in one
    for at, w in ((768, 2), (1152, 3), (1536, 4)):
        assert f"rsq::lds_merge<0>(cell + {at}, (u64)(i64)in{w});" in one
    assert one.count("rsq::lds_merge<0>(cell + ") == 4
    # the epilogue takes the fields apart per lane, in front of the wave reduction
    take = one.index("if (c >= 30 && c < 36) v = (s_lane[(c - 24) * 64 + (threadIdx.x & 63)] >> 21) & 2097151ull;")
    assert one.index("if (c < 6) v = (u32)v == 0xffffffffu ? 0x7fffffffffffffffull : (u64)(a.row0 + (i64)(u32)v);") < take < one.index("wave_reduce_to_lane63<2>(v)")
    assert "if (c >= 36 && c < 42) v = (s_lane[(c - 30) * 64 + (threadIdx.x & 63)] >> 42) & 2097151ull;" in one


def test_signed_inputs_and_min_max_keep_words_of_their_own(ctxs):
    one = _form(_source(ctxs[0], _family()["packed"])[0], 1)
    # blocks: first row, min(c) | max(c) | sum(a), sum(s), count, sum(d); a, the count and d share a's word, s is signed
    assert "rsq::lds_merge<0>(cell + 1152, (u64)(u32)in1 | (u64)(u32)in3 << 21 | (u64)(u32)in4 << 42);" in one
    assert "rsq::lds_merge<0>(cell + 1536, (u64)(i64)in2);" in one
    assert "rsq::lds_merge<2>(cell + 384, (u64)in5);" in one and "rsq::lds_merge<3>(cell + 768, (u64)in6);" in one
    one = _form(_source(ctxs[0], _family()["minmax"])[0], 1)      # sum(c) spans both signs at 24 bits: nothing shares a word
    assert " | (u64)(u32)in" not in one and "rsq::lds_merge<0>(cell + 1152, (u64)(i64)in1);" in one


def test_statements_outside_the_family_have_no_second_form(ctxs, monkeypatch):
    both = ctxs[0]
    t = N.fold_table(4 * N.TILE + 77, "pos", 3)
    outside = [N.plan(N.Statement([("sum", "e"), ("min", "c")], ["b"]), [t]),                    # no partial sum
               N.plan(N.late_statement(), [N.late_table(40_000)]),                                # the late-load form
               N.plan(L.CELLS64, [L.cells64_table(300)])]                                         # partial sums, but no room for four waves per SIMD
    for plan in outside:
        src, ex = _source(both, plan)
        assert "RSQ_ROW_CELLS" not in src and "second form" not in ex and "\x01" not in src
    monkeypatch.setenv("RSQ_NARROW_SCANS", "0")
    src, _ = _source(both, _family()["q1"])
    assert "RSQ_ROW_CELLS" not in src and "\x01" not in src


def test_max_grid_changes_no_text(ctxs, monkeypatch):
    for name, plan in _family().items():
        texts = []
        for g in (None, "1", "4"):
            if g:
                monkeypatch.setenv("RSQ_MAX_GRID", g)
            else:
                monkeypatch.delenv("RSQ_MAX_GRID", raising=False)
            texts.append(_source(ctxs[0], plan)[0])
        monkeypatch.delenv("RSQ_MAX_GRID", raising=False)
        assert len(set(texts)) == 1, name


@hipcc
@pytest.mark.parametrize("name", ["q1", "packed"])
def test_form_1_fits_its_launch_bound_without_scratch(ctxs, tmp_path, name):
    src, _ = _source(ctxs[0], _family()[name])
    (tmp_path / "k.hip").write_text(src)
    out = subprocess.run([os.path.join(ROOT, "tools", "isa.sh"), str(tmp_path / "k.hip"), str(tmp_path / "k.s"), "-DRSQ_ROW_CELLS=1"],
                         capture_output=True, text=True, check=True).stdout
    r = {k: int(re.search(k + r": (\d+)", out).group(1)) for k in ("ScratchSize", "NumVgprs", "Occupancy")}
    # four waves per SIMD (RSQ_MIN_WG 4) leave 128 VGPRs; the form holds no accumulators and stays far below
    assert r["ScratchSize"] == 0 and r["NumVgprs"] <= 128 and r["Occupancy"] >= 4
    asm = (tmp_path / "k.s").read_text()
    assert "ds_add_u64" in asm and "ds_min_u32" in asm and "flat_atomic" not in asm      # the cell updates are LDS operations
