"""A ReSQL row store transposed into columns on the device (resql_amd/csrc/rowstore_device.hip; rsq_table_from_rowstore_ex,
rsq_ctx_set_rowstore_bridge).  The device path is never compared with itself: (a) the numpy source columns the blocks were packed from,
with the NUL rule applied in numpy, and (b) the host path over the same blocks, byte for byte, statistics included."""
import numpy as np
import pytest

from resql_amd import engine, plan as P, tpch
from resql_amd.plan import TypeInit as T

import rowstorecases as R

pytestmark = pytest.mark.gpu

TS = 61
MIB2 = 2 << 20


def _chunks(n: int, chunk_bytes: int, ts: int) -> int:
    rows = max(1, (chunk_bytes or (64 << 20)) // ts)
    return -(-n // rows)


def _check(ctx, schema, cols, blocks, chunk_bytes=0, host=None):
    """bridge `blocks` on the device and hold the table against both yardsticks"""
    n, ts = len(cols[0]), R.tuple_size(schema)
    own = host is None
    if own:
        host = ctx.from_rowstore(schema, blocks, mode=engine.ROWSTORE_HOST)
    dev = ctx.from_rowstore(schema, blocks, mode=engine.ROWSTORE_DEVICE, chunk_bytes=chunk_bytes)
    try:
        rep = dev.bridge_report
        assert rep["path"] == 1 and rep["fallback_reason"] == engine.ROWSTORE_FALLBACK_NONE, rep
        assert rep["rows"] == n == dev.n_rows and rep["tuple_bytes"] == n * ts
        assert rep["chunks"] == _chunks(n, chunk_bytes, ts), rep
        assert host.bridge_report["path"] == 0 and host.n_rows == n
        want, got, ref = R.expected_columns(schema, cols), R.columns_of(dev, schema), R.columns_of(host, schema)
        for c in schema.columns:
            assert got[c.name] == want[c.name], f"{c.name}: the device bridge against the source column"
            assert got[c.name] == ref[c.name], f"{c.name}: the device bridge against the host bridge"
        assert dev.stats_blob() == host.stats_blob()
    finally:
        dev.close()
        if own:
            host.close()


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1000])
def test_tile_and_chunk_edges(gpu_ctx, n):
    cols = R.edge_columns(n)
    for block_bytes in (None, 200, MIB2):          # one block; 3 tuples and a remainder; ReSQL's 2 MiB
        blocks = R.pack(R.EDGE, cols, block_bytes=block_bytes)
        host = gpu_ctx.from_rowstore(R.EDGE, blocks, mode=engine.ROWSTORE_HOST)
        try:
            for chunk_bytes in (0, 1, TS * 3, 4096):          # 64 MiB; one tuple per chunk; three; 67
                if chunk_bytes == 1 and n > 257:
                    continue
                _check(gpu_ctx, R.EDGE, cols, blocks, chunk_bytes, host)
        finally:
            host.close()


@pytest.mark.parametrize("first_offset", [1, 7, 15])
def test_blocks_at_any_alignment(gpu_ctx, first_offset):
    cols = R.edge_columns(600)
    blocks = R.pack(R.EDGE, cols, block_bytes=200, first_offset=first_offset)
    assert blocks[0].ctypes.data % 64 == first_offset
    _check(gpu_ctx, R.EDGE, cols, blocks, 4096)
    _check(gpu_ctx, R.EDGE, cols, R.pack(R.EDGE, cols, first_offset=first_offset))


def _random_strings(rng, n, ln, edges=()):
    vals = [rng.integers(97, 123, size=int(rng.integers(0, ln + 1)), dtype=np.uint8).tobytes() for _ in range(n)]
    for i, e in enumerate(edges):
        vals[i] = e
    return R.strings(vals, ln)


def test_mid_size_tuples(gpu_ctx):
    """VARCHAR(300) + INT: tuples of 305 bytes, 161 rows per workgroup - fewer rows than lanes; two full workgroups and a ragged third"""
    schema = R.bare("mid", [("m_text", T.VARCHAR(300)), ("m_int", T.INT())])
    per_group = R.TILE_BYTES // R.tuple_size(schema)
    assert R.tuple_size(schema) == 305 and per_group == 161
    rng = np.random.default_rng(3)
    for n in (163 * 2 + 1, per_group * 2 + 1):
        cols = [_random_strings(rng, n, 300, [b"", b"x" * 300, b"ab\0cd"]), rng.integers(-2**31, 2**31, size=n, dtype=np.int64).astype(np.int32)]
        _check(gpu_ctx, schema, cols, R.pack(schema, cols, block_bytes=MIB2))


def test_a_tuple_longer_than_the_tile(gpu_ctx):
    """VARCHAR(50000) + BIGINT + CHAR(1): one tuple does not fit the LDS tile, the kernel works from global memory"""
    schema = R.bare("wide", [("w_text", T.VARCHAR(50000)), ("w_big", T.BIGINT()), ("w_code", T.CHAR(1))])
    assert R.tuple_size(schema) == 50011 > R.TILE_BYTES
    rng = np.random.default_rng(4)
    n = 5
    cols = [_random_strings(rng, n, 50000, [b"q" * 50000, b"", b"head\0tail"]), np.array([-2**63, 2**63 - 1, -1, 0, 7], dtype=np.int64),
            np.frombuffer(b"ANRFO", dtype=np.uint8).copy()]
    blocks = R.pack(schema, cols, block_bytes=MIB2)
    _check(gpu_ctx, schema, cols, blocks)
    _check(gpu_ctx, schema, cols, blocks, chunk_bytes=1)
    _check(gpu_ctx, schema, cols, blocks, chunk_bytes=50011 * 2)


def test_more_than_64_columns_take_the_host_path(gpu_ctx):
    schema = R.bare("many", [(f"c{i}", T.INT() if i % 2 else T.CHAR(3)) for i in range(65)])
    rng = np.random.default_rng(6)
    n = 40
    cols = [rng.integers(-1000, 1000, size=n).astype(np.int32) if i % 2 else _random_strings(rng, n, 3) for i in range(65)]
    t = gpu_ctx.from_rowstore(schema, R.pack(schema, cols, block_bytes=4096), mode=engine.ROWSTORE_DEVICE)
    try:
        assert t.bridge_report["path"] == 0 and t.bridge_report["fallback_reason"] == engine.ROWSTORE_FALLBACK_COLUMNS and t.n_rows == n
        assert R.columns_of(t, schema) == R.expected_columns(schema, cols)
    finally:
        t.close()
    # 64 columns are the device's
    schema64 = P.Table("many", schema.columns[:64], 0)
    _check(gpu_ctx, schema64, cols[:64], R.pack(schema64, cols[:64], block_bytes=4096))


def test_the_context_setting(gpu_ctx):
    cols = R.edge_columns(100)
    blocks = R.pack(R.EDGE, cols, block_bytes=200)
    try:
        assert gpu_ctx.from_rowstore(R.EDGE, blocks).bridge_report["path"] == 0          # the default
        gpu_ctx.set_rowstore_bridge(1)
        t = gpu_ctx.from_rowstore(R.EDGE, blocks)
        assert t.bridge_report["path"] == 1 and R.columns_of(t, R.EDGE) == R.expected_columns(R.EDGE, cols)
        assert gpu_ctx.from_rowstore(R.EDGE, blocks, mode=engine.ROWSTORE_HOST).bridge_report["path"] == 0
    finally:
        gpu_ctx.set_rowstore_bridge(0)
    assert gpu_ctx.from_rowstore(R.EDGE, blocks).bridge_report["path"] == 0


def test_a_device_bridged_tail_appended(gpu_ctx):
    """a Relation that grew: the head bridged on the host, the new tuples on the device and appended - the whole table bridged on the host"""
    cols = R.edge_columns(700)
    head, tail = [c[:450] for c in cols], [c[450:] for c in cols]
    whole = gpu_ctx.from_rowstore(R.EDGE, R.pack(R.EDGE, cols, block_bytes=MIB2), mode=engine.ROWSTORE_HOST)
    t = gpu_ctx.from_rowstore(R.EDGE, R.pack(R.EDGE, head, block_bytes=MIB2), mode=engine.ROWSTORE_HOST)
    more = gpu_ctx.from_rowstore(R.EDGE, R.pack(R.EDGE, tail, block_bytes=200, first_offset=7), mode=engine.ROWSTORE_DEVICE, chunk_bytes=4096)
    try:
        assert more.bridge_report["path"] == 1 and more.n_rows == 250
        t.append(more)
        assert t.n_rows == 700
        assert R.columns_of(t, R.EDGE) == R.columns_of(whole, R.EDGE) == R.expected_columns(R.EDGE, cols)
        assert t.stats_blob() == whole.stats_blob()
    finally:
        t.close()
        whole.close()


def _with_data(t: P.Table) -> P.Table:
    return P.Table(t.name, [c for c in t.columns if c.data is not None], t.n_rows)


def test_queries_over_bridged_tables(gpu_ctx):
    """TPC-H Q1, Q6 and Q3 at SF 0.01 over tables bridged on the device: the text of the same plans over rsq_table_create tables"""
    li = _with_data(tpch.lineitem_table(0.01, tpch.Q1_COLUMNS + ["l_orderkey"]))
    cu, od = _with_data(tpch.customer_table(0.01)), _with_data(tpch.orders_table(0.01))
    plans = [(tpch.q1_plan(li), [li]), (tpch.q6_plan(li), [li]), (tpch.q3_plan(cu, od, li), [cu, od, li])]
    created = {t.name: gpu_ctx.table(t) for t in (li, cu, od)}
    bridged = {}
    try:
        for t in (li, cu, od):
            blocks = R.pack(t, [c.data for c in t.columns], block_bytes=MIB2)
            bridged[t.name] = gpu_ctx.from_rowstore(t, blocks, mode=engine.ROWSTORE_DEVICE, chunk_bytes=1 << 20)
            assert bridged[t.name].bridge_report["path"] == 1 and bridged[t.name].n_rows == t.n_rows
            assert bridged[t.name].stats_blob() == created[t.name].stats_blob()
        for plan, tables in plans:
            want = gpu_ctx.run(plan, [created[t.name] for t in tables]).serialize()
            got = gpu_ctx.run(plan, [bridged[t.name] for t in tables]).serialize()
            assert want.count("\n") > 1
            assert got == want
    finally:
        for t in list(created.values()) + list(bridged.values()):
            t.close()
