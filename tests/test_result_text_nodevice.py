"""The device result text's public interface (rsq_query_result_text / _write, rsq_ctx_set_result_text, rsq_db_result_text_report) where
there is no device: a compile-only context writes on the host and says why, settings are validated, the struct_size of options and
report is honoured, and rsq_config has not grown."""
import ctypes as C

import numpy as np
import pytest

from resql_amd import engine, tpch


@pytest.fixture(scope="module")
def unexecuted(compile_ctx):
    """a compiled statement that has not been executed (a compile-only context cannot): a relation of no rows"""
    li = tpch.lineitem_table(0.01, tpch.Q6_COLUMNS, n_rows=1000)
    t = compile_ctx.table(li)
    q = compile_ctx.compile(tpch.q6_plan(li), [t])
    yield q
    q.close()
    t.close()


def test_the_setting_is_validated():
    ctx = engine.Context(device=-1)
    try:
        for bad in (2, -1):
            with pytest.raises(engine.EngineError) as e:
                ctx.set_result_text(bad)
            assert e.value.status == 1 and "result_text" in str(e.value)
        ctx.set_result_text(1)
        ctx.set_result_text(0)
    finally:
        ctx.close()


def test_a_query_without_a_result_answers_as_rsq_query_result_does(compile_ctx, unexecuted, tmp_path):
    from resql_amd import plan as P
    v = P.rsq_result_view()
    assert engine.lib().rsq_query_result(unexecuted.h, C.byref(v)) == 0 and v.n_rows == 0
    text, rep = unexecuted.result_text()
    assert text == b"" and rep["path"] == 0 and rep["fallback_reason"] == engine.TEXT_FALLBACK_NONE and rep["rows"] == 0 and rep["text_bytes"] == 0
    text, rep = unexecuted.result_text(mode=engine.TEXT_DEVICE)          # the device is asked for, and is not there
    assert text == b"" and rep["path"] == 0 and rep["fallback_reason"] == engine.TEXT_FALLBACK_NO_DEVICE and rep["tuples_from_device"] == 0
    path = str(tmp_path / "out.tbl")
    rep = unexecuted.write_result_text(path, mode=engine.TEXT_DEVICE)
    assert rep["path"] == 0 and rep["fallback_reason"] == engine.TEXT_FALLBACK_NO_DEVICE and open(path, "rb").read() == b""


def test_mode_0_follows_the_context():
    ctx = engine.Context(device=-1)
    try:
        li = tpch.lineitem_table(0.01, tpch.Q6_COLUMNS, n_rows=1000)
        t = ctx.table(li)
        q = ctx.compile(tpch.q6_plan(li), [t])
        assert q.result_text()[1]["fallback_reason"] == engine.TEXT_FALLBACK_NONE
        ctx.set_result_text(1)
        assert q.result_text()[1]["fallback_reason"] == engine.TEXT_FALLBACK_NO_DEVICE
        assert q.result_text(mode=engine.TEXT_HOST)[1]["fallback_reason"] == engine.TEXT_FALLBACK_NONE
        db = engine.Database(ctx)
        assert db.result_text_report["rows"] == 0 and db.result_text_report["path"] == 0
    finally:
        ctx.close()


def _raw_text(q, opt, rep_buf):
    L = engine.lib()
    p, n = C.c_void_p(), C.c_int64(-1)
    rc = L.rsq_query_result_text(q.h, opt, C.cast(rep_buf, C.POINTER(engine.rsq_result_text_report)) if rep_buf is not None else None, C.byref(p), C.byref(n))
    if rc == 0:
        assert n.value == 0 and C.string_at(p) == b""
        L.rsq_free(p)
    else:
        assert not p.value
    return rc


def test_report_and_options_honour_struct_size(unexecuted):
    full = C.sizeof(engine.rsq_result_text_report)
    assert full == 72 and C.sizeof(engine.rsq_result_text_options) == 24
    assert engine.rsq_result_text_report.rows.offset == 16 and engine.rsq_result_text_report.upload_ms.offset == 40
    # a host built against a report that ends behind tuples_from_device: nothing behind its 16 bytes is written
    buf = (C.c_uint8 * full)(*([0xEE] * full))
    C.cast(buf, C.POINTER(C.c_uint32))[0] = 16
    dev = engine.rsq_result_text_options(24, engine.TEXT_DEVICE, 0, 0)
    assert _raw_text(unexecuted, C.byref(dev), buf) == 0
    raw = bytes(buf)
    assert raw[16:] == b"\xee" * (full - 16)
    assert np.frombuffer(raw[:16], dtype=np.int32).tolist() == [16, 0, engine.TEXT_FALLBACK_NO_DEVICE, 0]
    # ... a larger one than the library's: its own size stays, the rest is untouched
    big = (C.c_uint8 * (full + 16))(*([0xEE] * (full + 16)))
    C.cast(big, C.POINTER(C.c_uint32))[0] = full + 16
    assert _raw_text(unexecuted, None, big) == 0
    assert bytes(big)[full:] == b"\xee" * 16 and np.frombuffer(bytes(big)[:4], dtype=np.uint32)[0] == full + 16
    # options: a short struct leaves the later fields at their defaults; bad values are refused
    rep = (C.c_uint8 * full)()
    C.cast(rep, C.POINTER(C.c_uint32))[0] = full
    short = engine.rsq_result_text_options(8, engine.TEXT_DEVICE, -5, -5)          # (chunk_rows / max_device_bytes are not read)
    assert _raw_text(unexecuted, C.byref(short), rep) == 0
    assert np.frombuffer(bytes(rep)[:12], dtype=np.int32).tolist() == [full, 0, engine.TEXT_FALLBACK_NO_DEVICE]
    for bad in (engine.rsq_result_text_options(24, 3, 0, 0), engine.rsq_result_text_options(24, -1, 0, 0), engine.rsq_result_text_options(24, 2, -1, 0),
                engine.rsq_result_text_options(24, 2, 0, -1), engine.rsq_result_text_options(0, 0, 0, 0)):
        assert _raw_text(unexecuted, C.byref(bad), rep) == 1
        assert engine.lib().rsq_query_result_write(unexecuted.h, b"/dev/null", C.byref(bad), None) == 1
    C.cast(rep, C.POINTER(C.c_uint32))[0] = 0
    assert _raw_text(unexecuted, None, rep) == 1
    small = engine.rsq_result_text_report(4)
    assert engine.lib().rsq_db_result_text_report(None, C.byref(small)) == 1


def test_rsq_config_keeps_its_size():
    assert C.sizeof(engine.rsq_config) == 88
