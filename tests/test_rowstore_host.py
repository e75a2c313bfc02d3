"""The row-store bridge on the host: the rule of a cell (resql_amd/csrc/rowstore.h) and the host loop (rowstore.cpp) under the address
and undefined-behaviour sanitizers, through a C++ driver built with g++ (tests/cpp/rowstore_test.cpp); and the device bridge's public
interface (rsq_table_from_rowstore_ex, rsq_ctx_set_rowstore_bridge) where there is no device: a compile-only context takes the host
path and says why, settings are validated, and the struct_size of options and report is honoured."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from resql_amd import engine, plan as P

import rowstorecases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cell_rule_and_host_loop_under_sanitizers(tmp_path):
    exe = str(tmp_path / "rowstore_test")
    src = os.path.join(ROOT, "resql_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + src, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "rowstore_test.cpp"),
                           os.path.join(src, "rowstore.cpp"), os.path.join(src, "expr.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "rowstore_test ok" in out.stdout


def _raw_bridge(ctx, schema, blocks, opt, rep_buf):
    keep = []
    d = P.Table(schema.name, [P.Column(c.name, c.type) for c in schema.columns], 0).to_c(keep)
    ptrs = (C.c_void_p * max(1, len(blocks)))(*[b.ctypes.data for b in blocks])
    sizes = (C.c_size_t * max(1, len(blocks)))(*[b.size for b in blocks])
    h = C.c_void_p()
    L = engine.lib()
    rc = L.rsq_table_from_rowstore_ex(ctx.h, C.byref(d), ptrs, sizes, len(blocks), opt,
                                      None if rep_buf is None else C.cast(rep_buf, C.POINTER(engine.rsq_rowstore_report)), C.byref(h))
    if rc == 0:
        L.rsq_table_destroy(h)
    return rc


def test_host_fallback_and_argument_checks():
    ctx = engine.Context(device=-1)
    try:
        cols = R.edge_columns(300)
        blocks = R.pack(R.EDGE, cols, block_bytes=200)
        want = R.expected_columns(R.EDGE, cols)
        # the device is asked for and is not there: the host path, reported, with the columns of yardstick (a)
        t = ctx.from_rowstore(R.EDGE, blocks, mode=engine.ROWSTORE_DEVICE)
        host = ctx.from_rowstore(R.EDGE, blocks, mode=engine.ROWSTORE_HOST)
        rep = t.bridge_report
        assert rep["path"] == 0 and rep["fallback_reason"] == engine.ROWSTORE_FALLBACK_NO_DEVICE
        assert rep["rows"] == 300 == t.n_rows and rep["tuple_bytes"] == 300 * 61 and rep["chunks"] == 0 and rep["total_ms"] > 0
        assert host.bridge_report["path"] == 0 and host.bridge_report["fallback_reason"] == engine.ROWSTORE_FALLBACK_NONE
        assert R.columns_of(t, R.EDGE) == want
        assert R.columns_of(host, R.EDGE) == want
        assert t.stats_blob() == host.stats_blob()
        # the context's setting: validated, and followed by mode 0
        with pytest.raises(engine.EngineError) as e:
            ctx.set_rowstore_bridge(2)
        assert e.value.status == 1 and "rowstore_bridge" in str(e.value)
        ctx.set_rowstore_bridge(1)
        assert ctx.from_rowstore(R.EDGE, blocks).bridge_report["fallback_reason"] == engine.ROWSTORE_FALLBACK_NO_DEVICE
        ctx.set_rowstore_bridge(0)
        assert ctx.from_rowstore(R.EDGE, blocks).bridge_report["fallback_reason"] == engine.ROWSTORE_FALLBACK_NONE
        # options: every bad value is RSQ_ERR_INVALID with a message that names the field
        for kw, field in (({"mode": 3}, "mode"), ({"chunk_bytes": -1}, "chunk_bytes"), ({"chunk_bytes": (1 << 30) + 1}, "chunk_bytes")):
            with pytest.raises(engine.EngineError) as e:
                ctx.from_rowstore(R.EDGE, blocks, **kw)
            assert e.value.status == 1 and "rsq_rowstore_options." + field in str(e.value), str(e.value)
        ctx.from_rowstore(R.EDGE, blocks, chunk_bytes=1 << 30).close()
        # struct_size: 4 is refused in options and report; a short report is written no further than it reaches
        full = C.sizeof(engine.rsq_rowstore_report)
        assert full == 88 and C.sizeof(engine.rsq_rowstore_options) == 16
        L = engine.lib()
        assert _raw_bridge(ctx, R.EDGE, blocks, C.byref(engine.rsq_rowstore_options(4, 0, 0)), None) == 1
        assert "rsq_rowstore_options.struct_size" in L.rsq_last_error(ctx.h).decode()
        buf = (C.c_uint8 * full)(*([0xEE] * full))
        C.cast(buf, C.POINTER(C.c_uint32))[0] = 4
        assert _raw_bridge(ctx, R.EDGE, blocks, None, buf) == 1
        assert "rsq_rowstore_report.struct_size" in L.rsq_last_error(ctx.h).decode()
        C.cast(buf, C.POINTER(C.c_uint32))[0] = 24
        assert _raw_bridge(ctx, R.EDGE, blocks, C.byref(engine.rsq_rowstore_options(8, engine.ROWSTORE_DEVICE, -5)), buf) == 0      # (chunk_bytes is not read)
        raw = bytes(buf)
        assert raw[24:] == b"\xee" * (full - 24)
        assert np.frombuffer(raw[:16], dtype=np.int32).tolist() == [24, 0, engine.ROWSTORE_FALLBACK_NO_DEVICE, 0] and np.frombuffer(raw[16:24], dtype=np.int64)[0] == 300
        # a type no column holds: the host path's error, whichever path is asked for
        bad = R.bare("bad", [("a", P.TypeInit.INT()), ("f", P.SqlType(P.FLOAT))])
        for mode in (engine.ROWSTORE_HOST, engine.ROWSTORE_DEVICE):
            with pytest.raises(engine.EngineError) as e:
                ctx.from_rowstore(bad, [np.zeros(24, dtype=np.uint8)], mode=mode)
            assert e.value.status == 1 and "unsupported column type" in str(e.value)
    finally:
        ctx.close()
