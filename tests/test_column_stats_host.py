"""The references of tests/statcases.py are not taken on trust: each vectorised one is held against a plain Python loop over a few hundred
small random columns.  The constants it takes from the source are read from the source, and the case lists are asserted to hold the
boundaries they are there for.  Then every case goes through a compile-only context: hostStats, narrowWidth and hostDictionary - the second
implementation of the contract the device kernels implement, and the one every codegen test plans from - must agree with the references
on the statistics blob, the images' description and the dictionary's entries.  rsq_table_read_image refuses bad arguments without touching
memory, and says RSQ_ERR_UNSUPPORTED where a context without a device has nothing to copy."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from resql_amd import engine

import statcases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "resql_amd", "csrc")


# ---- the source's constants ---------------------------------------------------------------------------------------------------------
def test_constants_are_the_sources():
    aot = open(os.path.join(SRC, "aot_kernels.hip")).read()
    stats = aot[aot.index("void computeColumnStats("):aot.index("// generator (mirror of")]
    assert re.findall(r"const unsigned grid = (\d+);", stats) == [str(sc.STATS_GRID)]                  # k_minmax, k_byteset
    enc = aot[aot.index("static void launchEncode("):aot.index("static void buildNarrowImages(")]
    assert re.findall(r"const unsigned grid = (\d+);", enc) == [str(sc.STATS_GRID)]                    # k_encode
    for kernel in ("k_minmax", "k_byteset", "k_encode"):
        body = aot[aot.index(f"__launch_bounds__(256) {kernel}("):]
        assert "i < n; i += (i64)gridDim.x * blockDim.x)" in body[:body.index("\n}\n")], kernel
    assert sc.STRIDE == sc.STATS_GRID * 256
    m = re.search(r"enum \{ DICT_MAX = (\d+), DICT_SLOTS = (\d+), DICT_SAMPLE_ROWS = (\d+), DICT_COLLECT_GRID = (\d+) \};", aot)
    assert tuple(int(g) for g in m.groups()) == (sc.DICT_MAX, sc.DICT_SLOTS, sc.SAMPLE, sc.DICT_COLLECT_GRID)
    assert "unsigned h = 2166136261u;" in aot and "h = (h ^ p[i]) * 16777619u;" in aot                  # fnv_slot
    api = open(os.path.join(SRC, "api.cpp")).read()
    assert "struct StatsHead { uint64_t magic; int64_t nCols, row0, nRows; };" in api
    m = re.search(r"struct StatsCol \{ int32_t (\w+), (\w+); int64_t (\w+), (\w+); int32_t (\w+), (\w+); uint8_t (\w+)\[256\]; \};", api)
    assert list(m.groups()) == sc.COL_FIELDS
    assert int(re.search(r"STATS_MAGIC = (0x[0-9a-f]+)ull", api).group(1), 16) == sc.STATS_MAGIC
    assert sc.HEAD.size == 32 and sc.COL.size == 8 + 16 + 8 + 256


def test_case_lists_hold_the_boundaries():
    S = sc.STRIDE
    assert S == 262144 and sc.BIG == 2 * S + 1
    assert sc.N_SIZES == [1, 2, 63, 64, 65, 255, 256, 257, S - 1, S, S + 1, 2 * S + 1]
    # order: one repeat and one descent at every pair, for every element type of k_minmax; the whole-column shapes; one row
    assert sc.ORDER_PAIRS == [(0, 1), (63, 64), (255, 256), (S - 1, S), (sc.BIG - 2, sc.BIG - 1)]
    assert [t[0] for t in sc.ORDER_TYPES] == ["INT", "DATE", "BIGINT"]
    cases = sc.order_cases()
    assert {(flaw, pair) for _, n, flaw, pair in cases if pair} == {(f, p) for f in ("repeat", "descent") for p in sc.ORDER_PAIRS}
    assert all(n == sc.BIG for _, n, _, pair in cases if pair)
    assert {(flaw, n) for _, n, flaw, pair in cases if not pair} >= {("untouched", sc.BIG), ("constant", sc.BIG), ("descending", sc.BIG),
                                                                     ("untouched", 1), ("constant", 1), ("descending", 1)}
    for _, n, flaw, pair in cases:
        for name, t, col in sc.order_columns(n, flaw, pair):
            v = sc.as_int64(col, t)
            d = np.diff(v)
            assert len(v) == n
            if flaw == "repeat":
                assert list(np.flatnonzero(d <= 0)) == [pair[0]] and d[pair[0]] == 0, (name, pair)
            elif flaw == "descent":
                assert list(np.flatnonzero(d <= 0)) == [pair[0]] and d[pair[0]] < 0, (name, pair)
            elif flaw == "untouched":
                assert np.all(d > 0)
            assert sc.stats_reference(col, t)[1:3] == sc.order_expectation(n, flaw), (name, flaw, pair)
    d = sc.as_int64(sc.ascending(sc.BIG, sc.DATE), sc.DATE)
    assert d[0] < 1 << 31 < d[-1]                       # read signed, this column descends once and its minimum is negative
    # extremes
    assert sc.EXTREME_ROWS == [0, S, sc.BIG - 1]
    assert sc.EXTREME_VALUES == {"INT": (-2**31, 2**31 - 1), "DATE": (0, 2**32 - 1), "BIGINT": (-2**63, 2**63 - 1)}
    assert {(w, r) for _, w, r in sc.extreme_cases()} == {(w, r) for w in (0, 1) for r in sc.EXTREME_ROWS}
    for _, which, row in sc.extreme_cases():
        for name, t, col in sc.extreme_columns(which, row):
            v = sc.as_int64(col, t)
            want = sc.EXTREME_VALUES[t[0]][which]
            assert list(np.flatnonzero(v == want)) == [row], (name, which, row)
            assert (int(v.min()) if which == 0 else int(v.max())) == want
            if t == sc.DATE:
                assert (1 << 31) in v and int(v.min()) >= 0
            if t == sc.BIGINT:
                assert sc.stats_reference(col, t)[0] == 1 and sc.narrow_reference(col, t)[0] == 0          # valid, and no image
    assert sc.SPANS == [255, 256, 65535, 65536, 2**32 - 1, 2**32] and sc.SPAN_WIDTHS == [1, 2, 2, 4, 4, 0]
    for where in sc.SPAN_BASES:
        cols = sc.span_columns(where, n=1000)
        assert {t[0] for _, t, _ in cols} == {"BIGINT", "DECIMAL"}
        for (name, t, col), span, width in zip(cols, sc.SPANS, sc.SPAN_WIDTHS):
            mn, mx = int(col.min()), int(col.max())
            assert mx - mn == span and sc.narrow_reference(col, t)[:2] == (width, mn if width else 0), (where, name)
            assert mn == {"negative": -1000, "bottom": sc.INT64_MIN + 1, "top": sc.INT64_MAX - 1 - span}[where]
            assert (int(col[0]), int(col[-1])) == (mx, mn)
    # byte sets
    assert sc.BYTE_SETS == [[0], [255], [31, 32], [0, 255], list(range(256))]
    cols = sc.byteset_columns()
    assert all(len(c) == S + 1 for _, _, c in cols) and {t for _, t, _ in cols} == {sc.CHAR1, sc.BOOL}
    sets = {name: sc.stats_reference(c, t)[5] for name, t, c in cols}
    for k, s in enumerate(sc.BYTE_SETS):
        assert sets[f"c_set{k}"] == sets[f"o_set{k}"] == s
    by = {name: c for name, _, c in cols}
    assert list(np.flatnonzero(by["c_first"] == ord("Z"))) == [0] and list(np.flatnonzero(by["o_last"] == 7)) == [S]
    # dictionaries
    assert (sc.SAMPLE, sc.DICT_WIDTHS, sc.DICT_ROWS, sc.DICT_COUNTS) == (65536, [2, 10, 200], [1, 77, 65536, 65537, 300_000], [1, 2, 256, 257])
    grid = set(sc.dict_grid_cases())
    assert {(n, c, W) for W in (2, 10) for n in sc.DICT_ROWS for c in sc.DICT_COUNTS if c <= n} <= grid
    assert {(77, 1, 200), (65537, 256, 200), (65537, 257, 200)} <= grid
    for n, at in ((sc.SAMPLE + 1, sc.SAMPLE), (sc.LONG, sc.SAMPLE), (sc.LONG, sc.LONG - 1)):
        col = sc.dict_late_value(n, 10, at)
        assert len(np.unique(col[:at], axis=0)) == 256 and len(np.unique(col[:at + 1], axis=0)) == 257 and sc.dict_reference(col, 10) is None
    col = sc.dict_few_per_workgroup(10)
    assert len(col) == 300_000 and len(np.unique(col, axis=0)) == 293
    assert len(np.unique(col[:sc.SAMPLE], axis=0)) == 64                               # (the sample passes)
    rows = np.arange(len(col))
    wg = (rows // 256) % sc.DICT_COLLECT_GRID
    ids = rows // 1024
    assert max(len(set(ids[wg == b])) for b in range(sc.DICT_COLLECT_GRID)) <= 3      # (every workgroup passes)
    for n, shared in ((sc.SAMPLE, 1), (sc.LONG, 2)):
        col = sc.dict_one_value_per_workgroup(n, 10)
        entries, codes = sc.dict_reference(col, 10)
        grid_n = min(sc.DICT_COLLECT_GRID, (n + 255) // 256)
        wg = (np.arange(n) // 256) % grid_n
        assert len(entries) == 256
        assert all(len(set(codes[wg == b])) == 1 for b in range(grid_n))
        assert max(len(set(wg[codes == e])) for e in range(256)) == shared
    col = sc.dict_257_in_one_workgroup(10)
    wg = (np.arange(len(col)) // 256) % sc.DICT_COLLECT_GRID
    per_wg = [len(np.unique(col[wg == b], axis=0)) for b in range(sc.DICT_COLLECT_GRID)]
    assert per_wg[0] == 257 and set(per_wg[1:]) == {1} and len(np.unique(col[:sc.SAMPLE], axis=0)) == 256 and sc.dict_reference(col, 10) is None
    vals = sc.dict_bytewise_values(10)
    assert len(sc.dict_reference(vals, 10)[0]) == len(vals)
    raw = [bytes(v) for v in vals]
    assert any(a[:-1] == b[:-1] and a != b for a in raw for b in raw)                                          # the last byte alone
    assert any(a.split(b"\0")[0] == b.split(b"\0")[0] and a != b and b"\0" in a[:-1] for a in raw for b in raw)   # behind a NUL
    assert any(a.rstrip(b" \0") == b.rstrip(b" \0") and a != b for a in raw for b in raw)                       # trailing spaces
    common, wrap, landing = sc.dict_colliding_values(10)
    assert len(common) == len(wrap) == 5 and len({sc.fnv_slot(v) for v in common}) == 1 and sc.fnv_slot(common[0]) < 1023
    assert {sc.fnv_slot(v) for v in wrap} == {1023} and [sc.fnv_slot(v) for v in landing] == [0, 1]
    assert len(np.unique(np.concatenate([common, wrap, landing]), axis=0)) == 12


# ---- the references against plain loops ---------------------------------------------------------------------------------------------
def _loop_stats(values):
    mn = mx = values[0]
    asc = strict = True
    for i in range(1, len(values)):
        v, prev = values[i], values[i - 1]
        mn, mx = min(mn, v), max(mx, v)
        if v < prev:
            asc = False
        if v <= prev:
            strict = False
    return (1, int(asc), int(asc and strict), mn, mx, [])


def _random_numeric(rng, t):
    n = int(rng.integers(1, 40))
    info = np.iinfo(sc.DTYPES[t[0]])
    shape = int(rng.integers(0, 5))
    if shape == 0:                                     # anything
        col = rng.integers(info.min, info.max, n, dtype=sc.DTYPES[t[0]], endpoint=True)
    else:                                              # a small range somewhere, ends of the type's range included; often sorted
        span = int(rng.choice([0, 3, 255, 256, 65535, 65536, 2**32 - 1, 2**32]))
        span = min(span, int(info.max) - int(info.min))
        lo = int(rng.choice([int(info.min), int(info.min) + 1, -5 if info.min < 0 else 0, int(info.max) - span - 1, int(info.max) - span]))
        lo = max(int(info.min), min(lo, int(info.max) - span))
        col = np.array([lo + int(rng.integers(0, span + 1)) for _ in range(n)]).astype(sc.DTYPES[t[0]])
        if shape >= 3:
            col = np.sort(col)
        if shape == 4:
            col = np.unique(col)
    return col


def test_statistics_reference_against_a_loop():
    rng = np.random.default_rng(1)
    seen = set()
    for t in (sc.INT, sc.DATE, sc.BIGINT, sc.DECIMAL):
        for _ in range(150):
            col = _random_numeric(rng, t)
            got = sc.stats_reference(col, t)
            assert got == _loop_stats([int(v) for v in col]), (t, col)
            seen.add(got[1:3])
    assert seen == {(0, 0), (1, 0), (1, 1)}
    for t in (sc.CHAR1, sc.BOOL):
        for _ in range(100):
            col = rng.integers(0, 256, int(rng.integers(1, 300))).astype(np.uint8) if rng.integers(0, 2) else rng.choice(np.array([0, 31, 32, 255], dtype=np.uint8), 9)
            want = sorted({int(v) for v in col})
            assert sc.stats_reference(col, t) == (1, 0, 0, want[0], want[-1], want)
    assert sc.stats_reference(np.zeros((5, 3), dtype=np.uint8), ("CHAR", 3)) == sc.NO_STATS
    assert sc.stats_reference(np.zeros((5, 1), dtype=np.uint8), ("VARCHAR", 1)) == sc.NO_STATS
    assert sc.stats_reference(np.zeros((5, 0), dtype=np.uint8), ("CHAR", 0)) == sc.NO_STATS
    assert sc.stats_reference(np.zeros(0, dtype=np.int32), sc.INT) == sc.NO_STATS


def _loop_narrow(values, t):
    mn, mx = min(values), max(values)
    if mn == sc.INT64_MIN or mx == sc.INT64_MAX:
        return (0, 0, b"")
    span = mx - mn
    w = 1 if span < 2**8 else 2 if span < 2**16 else 4 if span < 2**32 else 0
    if (t[0] == "INT" and w != 1) or w == 0 or w >= sc.WIDTHS[t[0]]:
        return (0, 0, b"")
    return (w, mn, b"".join((v - mn).to_bytes(w, "little") for v in values))


def test_narrow_reference_against_a_loop():
    rng = np.random.default_rng(2)
    widths = set()
    for t in (sc.INT, sc.DATE, sc.BIGINT, sc.DECIMAL):
        for _ in range(200):
            col = _random_numeric(rng, t)
            got = sc.narrow_reference(col, t)
            assert got == _loop_narrow([int(v) for v in sc.as_int64(col, t)], t), (t, col)
            assert sc.narrow_reference(col, t, owned=False) == (0, 0, b"")
            widths.add((t[0], got[0]))
    assert widths == {("INT", 0), ("INT", 1), ("DATE", 0), ("DATE", 1), ("DATE", 2), ("BIGINT", 0), ("BIGINT", 1), ("BIGINT", 2), ("BIGINT", 4),
                      ("DECIMAL", 0), ("DECIMAL", 1), ("DECIMAL", 2), ("DECIMAL", 4)}
    assert sc.narrow_reference(np.zeros(4, dtype=np.uint8), sc.BOOL) == (0, 0, b"")


def test_dictionary_reference_and_hash_against_loops():
    rng = np.random.default_rng(3)
    for _ in range(200):
        W = int(rng.choice([1, 2, 3, 10]))
        pool = rng.integers(0, 256, (int(rng.integers(1, 300)), W)).astype(np.uint8) if rng.integers(0, 3) else \
            rng.choice(np.array([0, 32, 97], dtype=np.uint8), (int(rng.integers(1, 12)), W))          # (NULs and spaces, front and back)
        col = pool[rng.integers(0, len(pool), int(rng.integers(1, 400)))]
        rows = [bytes(r) for r in col]
        entries = sorted(set(rows))                    # (bytes compare as memcmp does)
        got = sc.dict_reference(col, W)
        if len(entries) > 256:
            assert got is None
            continue
        assert [bytes(e) for e in got[0]] == entries
        by_rows = np.unique(col, axis=0, return_inverse=True)
        assert np.array_equal(by_rows[0], got[0]) and np.array_equal(np.asarray(by_rows[1]).reshape(-1), got[1])
        assert [int(c) for c in got[1]] == [entries.index(r) for r in rows]
        assert [int(s) for s in sc.fnv_slots(col[:20])] == [sc.fnv_slot(r) for r in rows[:20]]
    assert sc.dict_reference(np.zeros((0, 4), dtype=np.uint8), 4) is None
    assert sc.fnv_slot(b"") == 2166136261 & 1023 and sc.fnv_slot(b"a") == 0xe40c292c & 1023          # FNV-1a's published offset basis and "a"


# ---- hostStats, narrowWidth, hostDictionary -----------------------------------------------------------------------------------------
def _check(ctx, cols, dict_scans=False):
    t = ctx.table(sc.to_table("t", cols))
    try:
        return sc.assert_table_matches(t, cols, device=False, dict_scans=dict_scans)
    finally:
        t.close()


@pytest.mark.parametrize("n", sc.N_SIZES)
def test_host_sizes(compile_ctx, n):
    _check(compile_ctx, sc.size_columns(n))


@pytest.mark.parametrize("case", sc.order_cases(), ids=lambda c: c[0])
def test_host_order(compile_ctx, case):
    _, n, flaw, pair = case
    _check(compile_ctx, sc.order_columns(n, flaw, pair))


@pytest.mark.parametrize("case", sc.extreme_cases(), ids=lambda c: c[0])
def test_host_extremes(compile_ctx, case):
    _check(compile_ctx, sc.extreme_columns(case[1], case[2]))


@pytest.mark.parametrize("where", list(sc.SPAN_BASES))
def test_host_spans(compile_ctx, where):
    _check(compile_ctx, sc.span_columns(where))


def test_host_byte_sets(compile_ctx):
    _check(compile_ctx, sc.byteset_columns())


def test_host_empty_table_and_columns_without_statistics(compile_ctx):
    """no rows: no statistics whatever the type; a CHAR(0) column is no string by Type::isString() and has none either"""
    _check(compile_ctx, [(name, t, col[:0]) for name, t, col in sc.size_columns(5)] + [("s", ("CHAR", 4), np.zeros((0, 4), dtype=np.uint8))])
    _check(compile_ctx, [("z", ("CHAR", 0), np.zeros((9, 0), dtype=np.uint8)), ("s", ("VARCHAR", 1), np.full((9, 1), 65, dtype=np.uint8)),
                         ("k", sc.INT, np.arange(9, dtype=np.int32))])


DICT_CASES = sc.dict_cases()


@pytest.mark.parametrize("case", DICT_CASES, ids=lambda c: c[0])
def test_host_dictionaries(compile_ctx, monkeypatch, case):
    monkeypatch.setenv("RSQ_DICT_SCANS", "1")
    _check(compile_ctx, case[1](), dict_scans=True)


def test_host_dictionaries_are_opt_in(compile_ctx, monkeypatch):
    monkeypatch.delenv("RSQ_DICT_SCANS", raising=False)
    _check(compile_ctx, [("v", ("CHAR", 10), sc.dict_spread(500, sc.dict_values(7, 10)))], dict_scans=False)


@pytest.mark.parametrize("case", sc.append_cases(), ids=lambda c: c[0])
def test_host_append_recomputes(compile_ctx, monkeypatch, case):
    """rsq_table_append on the host's side: a repeat and a descent exactly on the seam, rows that widen the images, the 257th value"""
    monkeypatch.setenv("RSQ_DICT_SCANS", "1")
    parts = case[1]
    t = compile_ctx.table(sc.to_table("t", parts[0]))
    try:
        sc.assert_table_matches(t, parts[0], device=False, dict_scans=True)
        for k in range(1, len(parts)):
            t.append(compile_ctx.table(sc.to_table("t", parts[k])))
            sc.assert_table_matches(t, sc.appended(parts, k), device=False, dict_scans=True)
    finally:
        t.close()


# ---- the entry point's arguments ----------------------------------------------------------------------------------------------------
def test_read_image_refuses_bad_arguments(compile_ctx, monkeypatch):
    monkeypatch.setenv("RSQ_DICT_SCANS", "1")
    L = engine.lib()
    vals = sc.dict_values(3, 4)
    cols = [("k", sc.BIGINT, np.arange(10, dtype=np.int64) + 5), ("s", ("CHAR", 4), sc.dict_spread(10, vals)), ("w", sc.BIGINT, np.arange(10, dtype=np.int64) << 40)]
    t = compile_ctx.table(sc.to_table("t", cols))
    try:
        info = (C.c_int64 * 4)(-1, -1, -1, -1)
        guard = np.full(64, 0xAB, dtype=np.uint8)
        buf = guard.copy()
        call = lambda ctx, tab, name, which, dst, nbytes, inf: L.rsq_table_read_image(ctx, tab, name, which, dst, nbytes, inf)
        h, th = compile_ctx.h, t.h
        INVALID, UNSUPPORTED = 1, 3
        assert call(None, th, b"k", 0, None, 0, info) == INVALID
        assert call(h, None, b"k", 0, None, 0, info) == INVALID
        assert call(h, th, None, 0, None, 0, info) == INVALID
        assert call(h, th, b"k", 0, None, 0, None) == INVALID
        assert call(h, th, b"k", 0, None, 8, info) == INVALID                     # bytes without a destination
        assert call(h, th, b"k", -1, buf.ctypes.data, 0, info) == INVALID
        assert call(h, th, b"k", 3, buf.ctypes.data, 0, info) == INVALID
        assert list(info) == [-1, -1, -1, -1]                                     # (refused before anything was written)
        assert call(h, th, b"nosuch", 1, buf.ctypes.data, 0, info) == INVALID and b"no such column" in L.rsq_last_error(h)
        # a query: info whatever `which` is
        for which in (0, 1, 2):
            assert call(h, th, b"k", which, None, 0, info) == 0 and list(info) == [1, 5, 0, 10]
            assert call(h, th, b"s", which, buf.ctypes.data, 0, info) == 0 and list(info) == [0, 0, 3, 10]
            assert call(h, th, b"w", which, None, 0, info) == 0 and list(info) == [0, 0, 0, 10]
        # the host's copy of the entries, and nothing beyond them
        assert call(h, th, b"s", 1, buf.ctypes.data, 12, info) == 0
        assert bytes(buf[:12]) == sc.dict_reference(cols[1][2], 4)[0].tobytes() and np.all(buf[12:] == 0xAB)
        buf[:] = guard
        assert call(h, th, b"s", 1, buf.ctypes.data, 13, info) == INVALID and b"beyond" in L.rsq_last_error(h)
        assert call(h, th, b"k", 1, buf.ctypes.data, 1, info) == INVALID          # (a column without a dictionary has no entries)
        # no images without a device
        assert call(h, th, b"k", 0, buf.ctypes.data, 10, info) == UNSUPPORTED and list(info) == [1, 5, 0, 10]
        assert call(h, th, b"s", 2, buf.ctypes.data, 10, info) == UNSUPPORTED
        assert call(h, th, b"w", 0, buf.ctypes.data, 1, info) == UNSUPPORTED
        assert np.all(buf == guard)
        assert t.image_info("k") == (1, 5, 0, 10) and len(t.read_image("s", 1)) == 12
    finally:
        t.close()
    other = engine.Context(device=-1)
    try:
        t = compile_ctx.table(sc.to_table("t", cols))
        assert L.rsq_table_read_image(other.h, t.h, b"k", 0, None, 0, info) == 1          # another context's table
        t.close()
    finally:
        other.close()
