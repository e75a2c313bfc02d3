"""The device ingest's public interface (rsq_table_load_tbl_ex, rsq_config.tbl_ingest) where there is no device: a compile-only context
takes the host path and says why, settings are validated, and the struct_size of options and report is honoured."""
import ctypes as C

import numpy as np
import pytest

from resql_amd import engine, plan as P

import tblcases


def _columns(dt, schema):
    return {c.name: dt.read_column(c.name, c.type.np_dtype).tobytes() for c in schema.columns}


def test_device_mode_without_a_device_takes_the_host_path(compile_ctx):
    schema = tblcases.schema_table("customer")
    host = compile_ctx.load_tbl(schema, tblcases.FILES["customer"], mode=engine.TBL_HOST)
    dev = compile_ctx.load_tbl(schema, tblcases.FILES["customer"], mode=engine.TBL_DEVICE)
    try:
        assert host.load_report["path"] == 0 and host.load_report["fallback_reason"] == engine.TBL_FALLBACK_NONE
        assert dev.load_report["path"] == 0 and dev.load_report["fallback_reason"] == engine.TBL_FALLBACK_NO_DEVICE
        assert dev.load_report["rows"] == host.load_report["rows"] == 600 and dev.load_report["text_bytes"] == 95421
        assert dev.load_report["lines_patched"] == 0 and dev.load_report["total_ms"] > 0
        assert _columns(dev, schema) == _columns(host, schema)
        assert dev.stats_blob() == host.stats_blob()
    finally:
        host.close()
        dev.close()


def test_tbl_ingest_setting_is_validated_and_followed():
    with pytest.raises(engine.EngineError) as e:
        engine.Context(device=-1, tbl_ingest=2)
    assert e.value.status == 1 and "tbl_ingest" in str(e.value)
    with pytest.raises(engine.EngineError):
        engine.Context(device=-1, tbl_ingest=-1)
    ctx = engine.Context(device=-1, tbl_ingest=1)          # mode 0 follows the context: the device is asked for, and is not there
    try:
        schema = tblcases.schema_table("orders")
        t = ctx.load_tbl(schema, tblcases.FILES["orders"])
        assert t.load_report["path"] == 0 and t.load_report["fallback_reason"] == engine.TBL_FALLBACK_NO_DEVICE and t.n_rows == 2500
        t2 = ctx.load_tbl(schema, tblcases.FILES["orders"], mode=engine.TBL_HOST)
        assert t2.load_report["fallback_reason"] == engine.TBL_FALLBACK_NONE
        db = engine.Database(ctx)
        db.execute("create table t (a int, b char(5), c decimal(12,2))")
        assert db.load_report["rows"] == 0
    finally:
        ctx.close()


def test_rsq_config_keeps_its_size_and_layout():
    assert C.sizeof(engine.rsq_config) == 88
    assert engine.rsq_config.tbl_ingest.offset == 84 and engine.rsq_config.nested_loops_inner_slices.offset == 80
    old_host = engine.rsq_config.make(-1, tbl_ingest=7)          # a host whose header ends in front of the field: it reads as 0
    old_host.struct_size = engine.rsq_config.tbl_ingest.offset
    h = C.c_void_p()
    assert engine.lib().rsq_ctx_create(C.byref(old_host), C.byref(h)) == 0
    engine.lib().rsq_ctx_destroy(h)


def _raw_load(ctx, schema, path, opt, rep_buf):
    keep = []
    d = P.Table(schema.name, [P.Column(c.name, c.type) for c in schema.columns], 0).to_c(keep)
    h = C.c_void_p()
    L = engine.lib()
    rc = L.rsq_table_load_tbl_ex(ctx.h, C.byref(d), path.encode(), b"|", 0, opt, C.cast(rep_buf, C.POINTER(engine.rsq_tbl_load_report)), C.byref(h))
    if rc == 0:
        L.rsq_table_destroy(h)
    return rc


def test_report_and_options_honour_struct_size(compile_ctx):
    schema = tblcases.schema_table("customer")
    path = tblcases.FILES["customer"]
    full = C.sizeof(engine.rsq_tbl_load_report)
    assert full == 112 and C.sizeof(engine.rsq_tbl_load_options) == 24
    # a host built against a report that ends behind `rows`: nothing behind its 24 bytes is written
    buf = (C.c_uint8 * full)(*([0xEE] * full))
    C.cast(buf, C.POINTER(C.c_uint32))[0] = 24
    assert _raw_load(compile_ctx, schema, path, None, buf) == 0
    raw = bytes(buf)
    assert raw[24:] == b"\xee" * (full - 24)
    assert np.frombuffer(raw[:24], dtype=np.int32)[:4].tolist() == [24, 0, 0, 0] and np.frombuffer(raw[16:24], dtype=np.int64)[0] == 600
    # ... a larger one than the library's: its own size is written, the rest stays
    big = (C.c_uint8 * (full + 16))(*([0xEE] * (full + 16)))
    C.cast(big, C.POINTER(C.c_uint32))[0] = full + 16
    assert _raw_load(compile_ctx, schema, path, None, big) == 0
    assert bytes(big)[full:] == b"\xee" * 16 and np.frombuffer(bytes(big)[:4], dtype=np.uint32)[0] == full + 16
    # options: a short struct leaves the later fields at their defaults; bad values are refused
    rep = (C.c_uint8 * full)()
    C.cast(rep, C.POINTER(C.c_uint32))[0] = full
    short = engine.rsq_tbl_load_options(8, engine.TBL_DEVICE, -5, -5)          # (chunk_bytes / max_device_text_bytes are not read)
    assert _raw_load(compile_ctx, schema, path, C.byref(short), rep) == 0
    assert np.frombuffer(bytes(rep)[:12], dtype=np.int32).tolist() == [full, 0, engine.TBL_FALLBACK_NO_DEVICE]
    for bad in (engine.rsq_tbl_load_options(24, 3, 0, 0), engine.rsq_tbl_load_options(24, 2, 63, 0), engine.rsq_tbl_load_options(24, 2, 0, -1),
                engine.rsq_tbl_load_options(0, 0, 0, 0)):
        assert _raw_load(compile_ctx, schema, path, C.byref(bad), rep) == 1
    C.cast(rep, C.POINTER(C.c_uint32))[0] = 0
    assert _raw_load(compile_ctx, schema, path, None, rep) == 1
