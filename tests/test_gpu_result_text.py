"""A result relation's '.tbl' text written on the device (resql_amd/csrc/result_text.hip; rsq_query_result_text, rsq_ctx_set_result_text)
against the host's: rsq_result_serialize of the same view, byte for byte.  Tables are made from host columns, so the edge values of
tests/cpp/result_text_test.cpp stand in cells (tests/resulttextcases.py); row counts sit on both sides of a workgroup's 256 rows and
chunk seams fall inside a workgroup, at its edge and nowhere; spans of text on both sides of the 48 KiB LDS tile; the reference's own
goldens; the fallbacks; the statement loop's `tofile`; and what the call leaves behind (the view, the statement, the arenas)."""
import ctypes as C
import os
import sys

import pytest

from resql_amd import engine, plan as P

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import goldens  # noqa: E402
import resulttextcases as R  # noqa: E402

pytestmark = pytest.mark.gpu
TILE = 49152          # result_text.hip TEXT_TILE_BYTES


def host_text(q) -> bytes:
    """rsq_result_serialize of the statement's result view"""
    L = engine.lib()
    v = P.rsq_result_view()
    q.ctx._check(L.rsq_query_result(q.h, C.byref(v)))
    p = L.rsq_result_serialize(C.byref(v))
    assert p
    try:
        return C.string_at(p)
    finally:
        L.rsq_free(p)


def _used(ctx):
    m = ctx.memory_stats()
    return m["device_used_bytes"], m["pinned_used_bytes"]


def _executed(ctx, stmt, host):
    tabs = [ctx.table(t) for t in host]
    q = ctx.sql_compile(stmt, tabs) if isinstance(stmt, str) else ctx.compile(stmt, tabs)
    q.execute()
    return q, tabs


def _close(q, tabs):
    q.close()
    for t in tabs:
        t.close()


@pytest.mark.parametrize("n", R.ROW_COUNTS)
def test_row_counts_and_chunk_seams(gpu_ctx, n):
    q, tabs = _executed(gpu_ctx, R.EDGE_SQL, [R.edge_table(n)])
    try:
        want = host_text(q)
        assert want.count(b"\n") == n
        if n > 7:          # the quirks are in the cells: INT_MIN, INT64_MIN as DECIMAL(15,2) with its two signs, the dates 0xFFFFFFFF and 0
            assert b"-2147483648|" in want and b"--92233720368547758.08|" in want and b"429496/72/95|" in want and b"0/00/00|" in want
        for chunk_rows in (0, 100, 256):
            got, rep = q.result_text(mode=engine.TEXT_DEVICE, chunk_rows=chunk_rows)
            assert got == want, (n, chunk_rows)
            assert rep["path"] == 1 and rep["fallback_reason"] == engine.TEXT_FALLBACK_NONE and rep["tuples_from_device"] == 0
            assert rep["text_bytes"] == len(got) and rep["rows"] == n
            per = chunk_rows or max(n, 1)
            assert rep["chunks"] == (n + per - 1) // per
    finally:
        _close(q, tabs)


def test_spans_on_both_sides_of_the_lds_tile(gpu_ctx):
    """512 rows: the first workgroup's span (short values) fits the tile and is staged, the second one's (full-length values) is longer
    than the tile and goes straight to global memory.  Both strings are VARCHARs there: a CHAR(200) prints 200 characters whatever it
    holds, and 256 rows of them are more than 48 KiB.  That is the second table: 300 rows with a CHAR(200) column, so that both of its
    workgroups, the partly filled one too, write to global memory"""
    q, tabs = _executed(gpu_ctx, R.STRINGS_SQL, [R.short_then_full_table()])
    try:
        want = host_text(q)
        lines = want.split(b"\n")
        assert sum(len(l) + 1 for l in lines[:256]) <= TILE - 16 and sum(len(l) + 1 for l in lines[256:512]) > TILE
        for chunk_rows in (0, 256, 300):
            got, rep = q.result_text(mode=engine.TEXT_DEVICE, chunk_rows=chunk_rows)
            assert got == want and rep["path"] == 1 and rep["text_bytes"] == len(want)
    finally:
        _close(q, tabs)
    q, tabs = _executed(gpu_ctx, R.STRINGS_SQL, [R.padded_table()])
    try:
        want = host_text(q)
        lines = want.split(b"\n")
        assert sum(len(l) + 1 for l in lines[:256]) > TILE and len(lines) == 301
        got, rep = q.result_text(mode=engine.TEXT_DEVICE)
        assert got == want and rep["path"] == 1 and rep["chunks"] == 1
    finally:
        _close(q, tabs)


@pytest.mark.parametrize("name", ["q1_sf0.01", "q3_sf0.01", "q3_nolimit_sf0.05"])
def test_the_references_goldens_from_the_device(gpu_ctx, name):
    plan = goldens.golden_plan(name)
    q, tabs = _executed(gpu_ctx, plan, plan.tables)
    try:
        res = q.result(text=False)
        schema = "#schema " + "".join(f"{n}:{t}|" for n, t in zip(res.names, res.types)) + "\n"
        got, rep = q.result_text(mode=engine.TEXT_DEVICE, chunk_rows=1000)
        assert rep["path"] == 1 and rep["rows"] == res.n_rows and rep["chunks"] == (res.n_rows + 999) // 1000
        assert schema + got.decode("latin1") == goldens.golden_text(name)
    finally:
        _close(q, tabs)


def test_tuples_a_device_tail_wrote(gpu_ctx, monkeypatch, capfd):
    """a dense aggregation over dictionary codes whose tail runs on the device (tests/dicttailcases.py): the tuples lie in pinned memory and
    in the tail's device buffer.  Reading that buffer in place is not built: the tuples are uploaded (tuples_from_device == 0), the text is the host's"""
    import dicttailcases as D
    monkeypatch.setenv("RSQ_DICT_SCANS", "1")
    monkeypatch.setenv("RSQ_DEVICE_TAIL_MIN", "1")
    monkeypatch.setenv("RSQ_TRACE", "1")
    capfd.readouterr()
    q, tabs = _executed(gpu_ctx, D.HBM, [D.replay_table()])
    try:
        assert "device tail" in capfd.readouterr().err
        monkeypatch.delenv("RSQ_TRACE")
        want = host_text(q)
        got, rep = q.result_text(mode=engine.TEXT_DEVICE, chunk_rows=777)
        assert got == want and want.count(b"\n") > 4096
        assert rep["path"] == 1 and rep["tuples_from_device"] == 0 and rep["rows"] == want.count(b"\n")
    finally:
        _close(q, tabs)


def test_fallbacks_return_the_hosts_bytes(gpu_ctx):
    n = 10
    q, tabs = _executed(gpu_ctx, R.ALL_COLUMNS_SQL, [R.wide_table(n)])
    try:
        got, rep = q.result_text(mode=engine.TEXT_DEVICE)
        assert got == host_text(q) and got.count(b"|") == 65 * n
        assert rep["path"] == 0 and rep["fallback_reason"] == engine.TEXT_FALLBACK_SCHEMA and rep["text_bytes"] == len(got) and rep["rows"] == n
    finally:
        _close(q, tabs)
    q, tabs = _executed(gpu_ctx, R.EDGE_SQL, [R.edge_table(300)])
    try:
        got, rep = q.result_text(mode=engine.TEXT_DEVICE, max_device_bytes=1)
        assert got == host_text(q)
        assert rep["path"] == 0 and rep["fallback_reason"] == engine.TEXT_FALLBACK_DOES_NOT_FIT and rep["chunks"] == 0
        # a budget that holds a few rows at a time: the chunk shrinks until it fits
        got, rep = q.result_text(mode=engine.TEXT_DEVICE, max_device_bytes=16384)
        assert got == host_text(q) and rep["path"] == 1 and rep["chunks"] > 4
    finally:
        _close(q, tabs)


def test_the_statement_loop_writes_the_same_file(gpu_ctx, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)                                   # tofile writes "qres.tbl" into the working directory
    files, paths = [], []
    other = engine.Context(device=0)
    try:
        other.set_result_text(1)
        for ctx in (gpu_ctx, other):
            db = engine.Database(ctx)
            try:
                db.add_table(ctx.table(R.edge_table(1000)))
                db.execute("tofile=true")
                res = db.execute(R.EDGE_SQL)
                assert res.n_rows == 1000
                with open("qres.tbl", "rb") as f:
                    files.append(f.read())
                rep = db.result_text_report
                assert rep["rows"] == 1000 and rep["text_bytes"] == len(files[-1])
                paths.append(rep["path"])
                os.remove("qres.tbl")
            finally:
                db.close()
    finally:
        other.close()
    assert files[0] == files[1] and files[0].count(b"\n") == 1000
    assert paths == [0, 1]


def test_what_a_device_text_leaves_behind(gpu_ctx, tmp_path):
    q, tabs = _executed(gpu_ctx, R.EDGE_SQL, [R.edge_table(700)])
    try:
        before = q.result(text=False)
        want = host_text(q)
        used = _used(gpu_ctx)
        got, rep = q.result_text(mode=engine.TEXT_DEVICE, chunk_rows=300)
        assert got == want and rep["chunks"] == 3
        assert _used(gpu_ctx) == used
        rep = q.write_result_text(str(tmp_path / "out.tbl"), mode=engine.TEXT_DEVICE, chunk_rows=256)
        assert rep["path"] == 1 and rep["text_bytes"] == len(want) and open(tmp_path / "out.tbl", "rb").read() == want
        assert _used(gpu_ctx) == used
        after = q.result(text=False)
        assert after.tuples == before.tuples and after.n_rows == before.n_rows and host_text(q) == want
        q.execute()
        assert host_text(q) == want and q.result_text(mode=engine.TEXT_DEVICE)[0] == want
    finally:
        _close(q, tabs)
