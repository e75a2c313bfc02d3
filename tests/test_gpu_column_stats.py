"""What computeColumnStats leaves beside the columns of a table on the GPU - the statistics of k_minmax / k_byteset, the narrow image of
k_encode, the dictionary of k_dict_collect's three passes and the codes of k_dict_encode - read back and compared with the exact references
of tests/statcases.py and with what a compile-only context (hostStats, hostDictionary) makes of the same arrays.  The generated kernels trust
all of it without a check: a repeat the statistics miss is a join that silently loses rows, an extreme they miss a write outside a bitmap.
Every case is one table; the cases, and why they are where they are, are in statcases.py (tests/test_column_stats_host.py asserts that
they hold the boundaries).  The same checks then go through the other doors into the pass: append, refresh_stats over adopted columns, a
table without rows."""
import numpy as np
import pytest

from resql_amd import engine

import statcases as sc

pytestmark = pytest.mark.gpu


def _image_bytes(ctx):
    return int(ctx.memory_stats()["column_image_bytes"])


def _check(gpu_ctx, compile_ctx, cols, dict_scans=False):
    """one table on the device and one in the compile-only context over the same arrays: both equal the references, and their blobs each
    other; returns the device memory the table's images take"""
    host = sc.to_table("t", cols)
    before = _image_bytes(gpu_ctx)
    dev = gpu_ctx.table(host)
    try:
        held = _image_bytes(gpu_ctx) - before
        blob = sc.assert_table_matches(dev, cols, device=True, dict_scans=dict_scans)
        ref = compile_ctx.table(host)
        try:
            assert sc.assert_table_matches(ref, cols, device=False, dict_scans=dict_scans) == blob
            for name, _, _ in cols:
                assert ref.image_info(name) == dev.image_info(name), name
        finally:
            ref.close()
    finally:
        dev.close()
    assert _image_bytes(gpu_ctx) == before
    return held


def _expected_image_bytes(cols, dict_scans):
    """column_image_bytes of a table: images rounded up to 16 bytes; a dictionary's 256 entries + 16 bytes and its codes"""
    total = 0
    for _, t, data in cols:
        ref = sc.column_reference(data, t, dict_scans=dict_scans)
        if ref["narrow"][0]:
            total += (len(data) * ref["narrow"][0] + 15) & ~15
        if ref["dict"] is not None:
            total += sc.DICT_MAX * sc.type_width(t) + 16 + ((len(data) + 15) & ~15)
    return total


@pytest.mark.parametrize("n", sc.N_SIZES)
def test_sizes(gpu_ctx, compile_ctx, n):
    cols = sc.size_columns(n)
    assert _check(gpu_ctx, compile_ctx, cols) == _expected_image_bytes(cols, False)


@pytest.mark.parametrize("case", sc.order_cases(), ids=lambda c: c[0])
def test_order(gpu_ctx, compile_ctx, case):
    """one repeat or one descent in a strictly ascending column, wherever it lies: in the first rows, across a wave, a workgroup, the grid
    stride, in the last rows - ascending / strictlyAscending say so for INT, DATE and BIGINT"""
    _, n, flaw, pair = case
    cols = sc.order_columns(n, flaw, pair)
    _check(gpu_ctx, compile_ctx, cols)
    for _, t, col in cols:          # (the references gave what the case was built to give)
        assert sc.stats_reference(col, t)[1:3] == sc.order_expectation(n, flaw)


@pytest.mark.parametrize("case", sc.extreme_cases(), ids=lambda c: c[0])
def test_extremes(gpu_ctx, compile_ctx, case):
    """the type's smallest / largest value alone in row 0, in the first row of the second stride, in the last row; DATE is unsigned; a BIGINT
    column that holds INT64_MIN or INT64_MAX has valid statistics and no image"""
    cols = sc.extreme_columns(case[1], case[2])
    held = _check(gpu_ctx, compile_ctx, cols)
    assert held == _expected_image_bytes(cols, False)
    assert sc.narrow_reference(cols[2][2], cols[2][1])[0] == 0


@pytest.mark.parametrize("where", list(sc.SPAN_BASES))
def test_spans(gpu_ctx, compile_ctx, where):
    """max - min exactly at and one past every width's limit, from a negative base and next to either end of int64: width, base and every
    image byte; a span of 2^32 has no image and takes no memory"""
    cols = sc.span_columns(where)
    assert [sc.narrow_reference(c, t)[0] for _, t, c in cols] == sc.SPAN_WIDTHS
    assert _check(gpu_ctx, compile_ctx, cols) == _expected_image_bytes(cols, False)
    assert _check(gpu_ctx, compile_ctx, cols[-1:]) == 0


def test_byte_sets(gpu_ctx, compile_ctx):
    assert _check(gpu_ctx, compile_ctx, sc.byteset_columns()) == 0


def test_table_without_rows_and_columns_without_statistics(gpu_ctx, compile_ctx):
    """the device's nRows == 0 path: no statistics, no images, as the host says; strings without RSQ_DICT_SCANS have neither"""
    cols = [(name, t, col[:0]) for name, t, col in sc.size_columns(5)] + [("s", ("CHAR", 4), np.zeros((0, 4), dtype=np.uint8))]
    assert _check(gpu_ctx, compile_ctx, cols) == 0
    cols = [("s", ("CHAR", 4), sc.dict_spread(300, sc.dict_values(5, 4))), ("k", sc.BIGINT, np.arange(300, dtype=np.int64) << 33)]
    assert _check(gpu_ctx, compile_ctx, cols) == 0


# ---- dictionaries -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.dict_cases(), ids=lambda c: c[0])
def test_dictionaries(gpu_ctx, compile_ctx, monkeypatch, case):
    """1 to 257 values over row counts around the sample; a 257th value that only the passes behind the sample can see; columns only the
    union pass can refuse and ones that fill it exactly; values that differ in one byte, behind a NUL, in their padding; values that
    share a hash slot and ones whose probe wraps"""
    monkeypatch.setenv("RSQ_DICT_SCANS", "1")
    cols = case[1]()
    assert _check(gpu_ctx, compile_ctx, cols, dict_scans=True) == _expected_image_bytes(cols, True)


def test_slices_of_an_earlier_column_do_not_enter_the_union(gpu_ctx, compile_ctx, monkeypatch):
    """the union pass reads, of every workgroup's slice, the entries that workgroup counted and no others: what an earlier column of the
    same shape left in the recycled buffer stays out of a dictionary that is exactly full"""
    monkeypatch.setenv("RSQ_DICT_SCANS", "1")
    for n in (sc.SAMPLE, sc.LONG):
        other = sc.dict_spread(n, sc.dict_values(256, 10, seed=21), seed=5)
        cols = [("v", ("CHAR", 10), sc.dict_one_value_per_workgroup(n, 10))]
        for _ in range(2):
            _check(gpu_ctx, compile_ctx, [("v", ("CHAR", 10), other)], dict_scans=True)
            _check(gpu_ctx, compile_ctx, cols, dict_scans=True)


# ---- the other doors into computeColumnStats ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.append_cases(), ids=lambda c: c[0])
def test_append(gpu_ctx, compile_ctx, monkeypatch, case):
    """rsq_table_append gathers everything again over the joined rows: a repeat and a descent exactly on the seam, rows that widen the
    images 1 -> 2 -> 4 bytes, a dictionary that grows in front and then meets its 257th value"""
    monkeypatch.setenv("RSQ_DICT_SCANS", "1")
    parts = case[1]
    before = _image_bytes(gpu_ctx)
    dev = gpu_ctx.table(sc.to_table("t", parts[0]))
    ref = compile_ctx.table(sc.to_table("t", parts[0]))
    try:
        for k in range(len(parts)):
            if k:
                dev.append(gpu_ctx.table(sc.to_table("t", parts[k])))
                ref.append(compile_ctx.table(sc.to_table("t", parts[k])))
            cols = sc.appended(parts, k)
            blob = sc.assert_table_matches(dev, cols, device=True, dict_scans=True)
            assert sc.assert_table_matches(ref, cols, device=False, dict_scans=True) == blob
            assert _image_bytes(gpu_ctx) - before == _expected_image_bytes(cols, True), k
    finally:
        dev.close()
        ref.close()
    assert _image_bytes(gpu_ctx) == before


def test_refresh_over_adopted_columns(gpu_ctx):
    """rsq_table_create_device + rsq_table_refresh_stats: the statistics follow the content, adopted columns never get an image, and a
    CHAR(0) column - no string by its type, and no number - is not read at all"""
    import torch
    n = sc.STRIDE + 1
    types = {"i": sc.INT, "d": sc.DATE, "b": sc.BIGINT, "c": sc.CHAR1}
    host = {"i": sc.ascending(n, sc.INT), "d": sc.ascending(n, sc.DATE), "b": sc.ascending(n, sc.BIGINT), "c": np.full(n, 65, dtype=np.uint8)}
    as_torch = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a)
    dev = {k: as_torch(v).cuda() for k, v in host.items()}
    empty = torch.zeros(16, dtype=torch.uint8).cuda()
    cols = lambda: [(k, types[k], host[k]) for k in "idbc"] + [("z", ("CHAR", 0), np.zeros((n, 0), dtype=np.uint8))]
    t = gpu_ctx.table_from_device("t", n, [(k, sc.to_type(types[k]), dev[k].data_ptr()) for k in "idbc"] + [("z", sc.to_type(("CHAR", 0)), empty.data_ptr())])
    try:
        before = _image_bytes(gpu_ctx)
        sc.assert_table_matches(t, cols(), device=True, owned=False)
        # a repeat across the stride, a descent in the last rows, the unsigned maximum, a byte only the last row holds
        host["i"][sc.STRIDE] = host["i"][sc.STRIDE - 1]
        host["b"][n - 1] = host["b"][n - 2] - 1
        host["d"][0] = 0xffffffff
        host["c"][n - 1] = 0
        for k in "idbc":
            dev[k].copy_(as_torch(host[k]))
        torch.cuda.synchronize()
        t.refresh_stats()
        blob = sc.parse_blob(sc.assert_table_matches(t, cols(), device=True, owned=False))
        assert [c[1:3] for c in blob["cols"][:3]] == [(1, 0), (0, 0), (0, 0)] and blob["cols"][1][4] == 0xffffffff and blob["cols"][3][5] == [0, 65]
        assert _image_bytes(gpu_ctx) == before
    finally:
        t.close()


def test_read_image_on_a_device(gpu_ctx, monkeypatch):
    """the entry point's bounds on a context that has images: exactly the image and not a byte more"""
    import ctypes as C
    monkeypatch.setenv("RSQ_DICT_SCANS", "1")
    L = engine.lib()
    cols = [("k", sc.BIGINT, np.arange(100, dtype=np.int64) * 3 + 70_000), ("s", ("CHAR", 4), sc.dict_spread(100, sc.dict_values(3, 4)))]
    t = gpu_ctx.table(sc.to_table("t", cols))
    try:
        info = (C.c_int64 * 4)()
        buf = np.full(512, 0xAB, dtype=np.uint8)
        read = lambda name, which, nbytes: L.rsq_table_read_image(gpu_ctx.h, t.h, name, which, buf.ctypes.data, nbytes, info)
        assert read(b"k", 0, 200) == 0 and list(info) == [2, 70_000, 0, 100]
        assert bytes(buf[:200]) == sc.narrow_reference(cols[0][2], sc.BIGINT)[2] and np.all(buf[200:] == 0xAB)
        assert read(b"k", 0, 201) == 1 and read(b"k", 1, 1) == 1 and read(b"k", 2, 1) == 1
        assert read(b"s", 1, 12) == 0 and read(b"s", 1, 13) == 1 and read(b"s", 2, 100) == 0 and read(b"s", 2, 101) == 1 and read(b"s", 0, 1) == 1
        assert read(b"nosuch", 0, 0) == 1
    finally:
        t.close()
