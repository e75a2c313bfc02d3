"""Columns and exact references for tests/test_column_stats_host.py and tests/test_gpu_column_stats.py: what computeColumnStats
(aot_kernels.hip) leaves beside every column of every table - the statistics (k_minmax<int | unsigned | i64>, k_byteset), the narrow image
(k_encode<T, N>) and the dictionary image (k_dict_collect's sample, per-workgroup and union passes, k_dict_encode) - read back through
rsq_table_stats_export and rsq_table_read_image (include/resql_hip.h) instead of through the statements that happen to use a part of it.

The kernels are exact, so the references are: numpy comparisons of neighbours, Python integers for the extremes (a range of two int64
does not fit one), np.unique over the rows' bytes.  Nothing here calls the engine; the host test holds every vectorised reference against
a plain loop first.  The columns put the kernels' own boundaries inside a run: the wave (64), the workgroup (256), the grid stride of the
statistics kernels (1024 workgroups of 256 lanes), the dictionary's sample (65 536 rows), its 256 entries and its 1024 hash slots.

A column is a tuple (name, type, data): type is ("INT",), ("DATE",), ("BIGINT",), ("DECIMAL", p, s), ("BOOL",), ("CHAR", n) or
("VARCHAR", n); data is int32 / uint32 / int64 / int64 / uint8 / uint8 for CHAR(1), and an (n, W) uint8 array for the wider strings (a numpy
S dtype would drop trailing NULs, and the images are bytewise)."""
import struct

import numpy as np

# The kernels' geometry, in one place.  The host test reads the definitions in the source and compares.
STATS_GRID = 1024                 # workgroups of k_minmax, k_byteset and k_encode:          aot_kernels.hip  const unsigned grid = 1024
STRIDE = STATS_GRID * 256         # ... hence their grid stride: lane l of workgroup b reads rows b * 256 + l + k * STRIDE
DICT_MAX = 256                    # entries of a dictionary:                                  aot_kernels.hip  enum { DICT_MAX = 256, ...
DICT_SLOTS = 1024                 # slots of the open-addressing sets of k_dict_collect / k_dict_encode
SAMPLE = 65536                    # DICT_SAMPLE_ROWS: rows of the sample pass in front of a column longer than that
DICT_COLLECT_GRID = 512           # workgroups of the per-workgroup pass (each takes 256 rows per round)
STATS_MAGIC = 0x3174617473717372  # "rsqstat1"

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1

INT, DATE, BIGINT, DECIMAL, BOOL = ("INT",), ("DATE",), ("BIGINT",), ("DECIMAL", 15, 2), ("BOOL",)
CHAR1 = ("CHAR", 1)
NUMERIC = ("INT", "DATE", "BIGINT", "DECIMAL")
DTYPES = {"INT": np.int32, "DATE": np.uint32, "BIGINT": np.int64, "DECIMAL": np.int64, "BOOL": np.uint8}
WIDTHS = {"INT": 4, "DATE": 4, "BIGINT": 8, "DECIMAL": 8, "BOOL": 1}


def type_width(t):
    return WIDTHS.get(t[0], t[1] if t[0] in ("CHAR", "VARCHAR") else None)


def is_byte_type(t):
    return t[0] == "BOOL" or (t[0] == "CHAR" and t[1] == 1)


def is_string_type(t):          # expr.h Type::isString
    return t[0] == "VARCHAR" or (t[0] == "CHAR" and t[1] > 1)


# ---- the statistics blob (api.cpp, above exportTableStats) --------------------------------------------------------------------------
HEAD = struct.Struct("<Qqqq")                   # {u64 magic, i64 nCols, row0, nRows}
COL = struct.Struct("<iiqqii256s")              # {i32 valid, i32 ascending, i64 min, i64 max, i32 nBytes, i32 strict, u8[256]}
COL_FIELDS = ["valid", "ascending", "min", "max", "nBytes", "strict", "bytes"]


def parse_blob(blob):
    """{magic, n_cols, row0, n_rows, cols: [(valid, ascending, strict, min, max, byte set)]} - a column in the order stats_reference gives"""
    magic, n_cols, row0, n_rows = HEAD.unpack_from(blob, 0)
    assert len(blob) == HEAD.size + n_cols * COL.size, (len(blob), n_cols)
    cols = []
    for i in range(n_cols):
        valid, asc, mn, mx, n_bytes, strict, raw = COL.unpack_from(blob, HEAD.size + i * COL.size)
        assert 0 <= n_bytes <= 256 and not any(raw[n_bytes:]), (i, n_bytes)
        cols.append((valid, asc, strict, mn, mx, list(raw[:n_bytes])))
    return {"magic": magic, "n_cols": n_cols, "row0": row0, "n_rows": n_rows, "cols": cols}


# ---- references ---------------------------------------------------------------------------------------------------------------------
NO_STATS = (0, 0, 0, 0, 0, [])


def as_int64(data, t):
    """a numeric column's values as the statistics read them: INT signed, DATE unsigned, BIGINT / DECIMAL as they are"""
    return np.ascontiguousarray(data).view(DTYPES[t[0]]).astype(np.int64)


def stats_reference(data, t):
    """(valid, ascending, strict, min, max, byte set) of a column by the contract of engine.h ColumnStats: a numeric / date column has its
    extremes, `ascending` when no row is smaller than the row before it and `strict` when none is equal to it either; a BOOL / CHAR(1)
    column has its sorted distinct bytes with min / max their ends and no order flags; every other column, and every column of an empty
    table, has nothing"""
    if len(data) == 0:
        return NO_STATS
    if is_byte_type(t):
        s = np.unique(np.ascontiguousarray(data).view(np.uint8))
        return (1, 0, 0, int(s[0]), int(s[-1]), [int(v) for v in s])
    if t[0] not in NUMERIC:
        return NO_STATS
    v = as_int64(data, t)
    asc = bool(np.all(v[1:] >= v[:-1]))
    strict = bool(np.all(v[1:] > v[:-1]))
    return (1, int(asc), int(asc and strict), int(v.min()), int(v.max()), [])


def narrow_reference(data, t, owned=True):
    """(width, base, image bytes) by narrowWidth's rule: an owned numeric column whose max - min fits 1, 2 or 4 bytes - and fewer than the
    column's own - has the image (value - min) in that many bytes, little-endian; INT narrows to one byte only; a column that holds
    INT64_MIN or INT64_MAX has none"""
    none = (0, 0, b"")
    if not owned or t[0] not in NUMERIC or len(data) == 0:
        return none
    _, _, _, mn, mx, _ = stats_reference(data, t)
    if mn == INT64_MIN or mx == INT64_MAX:
        return none
    span = mx - mn                                       # (a Python integer: up to 2^64 - 3)
    w = 1 if span <= 0xff else 2 if span <= 0xffff else 4 if span <= 0xffffffff else 0
    if t[0] == "INT" and w != 1:
        return none
    if w == 0 or w >= WIDTHS[t[0]]:
        return none
    diff = as_int64(data, t).view(np.uint64) - np.uint64(mn & 0xffffffffffffffff)      # (wraps modulo 2^64, as the kernel's u64 does)
    assert int(diff.max()) == span
    return (w, mn, diff.astype({1: "<u1", 2: "<u2", 4: "<u4"}[w]).tobytes())


def dict_reference(data, W):
    """(entries in memcmp order as a (k, W) uint8 array, codes as uint8) of an (n, W) uint8 column, or None above 256 values / without rows.
    This is np.unique(rows, axis=0, return_inverse=True) with every row taken as ONE opaque W-byte item (numpy orders those as memcmp does)
    instead of as W one-byte fields: the same answer - the host test compares the two, and both with a loop - forty times sooner at W = 200"""
    rows = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1, W)
    if len(rows) == 0:
        return None
    items, codes = np.unique(rows.view(np.dtype((np.void, W))).reshape(-1), return_inverse=True)
    if len(items) > DICT_MAX:
        return None
    entries = np.frombuffer(items.tobytes(), dtype=np.uint8).reshape(len(items), W)
    return entries, np.asarray(codes).reshape(-1).astype(np.uint8)


def fnv_slot(value):
    """dictHash(value) & (DICT_SLOTS - 1): 32-bit FNV-1a over the stored bytes"""
    h = 2166136261
    for b in bytes(value):
        h = ((h ^ b) * 16777619) & 0xffffffff
    return h & (DICT_SLOTS - 1)


def fnv_slots(rows):
    """fnv_slot of every row of an (n, W) uint8 array"""
    rows = np.asarray(rows, dtype=np.uint8)
    h = np.full(len(rows), 2166136261, dtype=np.uint64)
    for i in range(rows.shape[1]):
        h = ((h ^ rows[:, i].astype(np.uint64)) * np.uint64(16777619)) & np.uint64(0xffffffff)
    return (h & np.uint64(DICT_SLOTS - 1)).astype(np.int64)


def column_reference(data, t, owned=True, dict_scans=False):
    """everything the engine keeps of one column: {"stats", "narrow", "dict"}"""
    d = dict_reference(data, type_width(t)) if (dict_scans and owned and is_string_type(t)) else None
    return {"stats": stats_reference(data, t), "narrow": narrow_reference(data, t, owned), "dict": d}


# ---- sizes --------------------------------------------------------------------------------------------------------------------------
N_SIZES = [1, 2, 63, 64, 65, 255, 256, 257, STRIDE - 1, STRIDE, STRIDE + 1, 2 * STRIDE + 1]
BIG = 2 * STRIDE + 1              # every lane of the first workgroup reads three rows, every other lane two


def ascending(n, t, start=None):
    """a strictly ascending column of n rows.  INT: steps of 3 from below 0.  DATE: steps of 2 that cross 2^31 after 500 rows (read signed,
    the column would descend there and its minimum would be negative).  BIGINT / DECIMAL: steps of 2^33 + 1 from -2^40 (no two values
    agree in their low or their high 32 bits)"""
    i = np.arange(n, dtype=np.int64)
    if t[0] == "INT":
        return ((-1000 if start is None else start) + 3 * i).astype(np.int32)
    if t[0] == "DATE":
        return (((1 << 31) - 1000 if start is None else start) + 2 * i).astype(np.uint32)
    return (-(1 << 40) if start is None else start) + ((1 << 33) + 1) * i


def size_columns(n):
    """one table per size: every statistics kernel and every width of k_encode at n rows"""
    rng = np.random.default_rng(1000 + n)
    return [
        ("i_asc", INT, ascending(n, INT)),
        ("i_small", INT, rng.integers(-100, 101, n).astype(np.int32)),                                   # (INT, one byte)
        ("d_asc", DATE, ascending(n, DATE)),
        ("d_rand", DATE, rng.integers(19920101, 19981231, n).astype(np.uint32)),                          # (DATE, two bytes once it spreads)
        ("b_asc", BIGINT, ascending(n, BIGINT)),
        ("b_byte", BIGINT, rng.integers(-7, 200, n).astype(np.int64)),                                    # (BIGINT, one byte)
        ("b_word", BIGINT, rng.integers(-(1 << 31), 1 << 31, n).astype(np.int64) * 2 + (1 << 40)),        # (BIGINT, four bytes once it spreads)
        ("m_short", DECIMAL, rng.integers(90_000, 150_000, n).astype(np.int64)),                          # (DECIMAL, two bytes)
        ("c_flag", CHAR1, rng.choice(np.frombuffer(b"ANR", dtype=np.uint8), n)),
        ("o_bool", BOOL, rng.integers(0, 2, n).astype(np.uint8)),
    ]


# ---- order --------------------------------------------------------------------------------------------------------------------------
ORDER_TYPES = [INT, DATE, BIGINT]
ORDER_PAIRS = [(0, 1), (63, 64), (255, 256), (STRIDE - 1, STRIDE), (BIG - 2, BIG - 1)]
ORDER_FLAWS = ["repeat", "descent"]
ORDER_WHOLE = ["untouched", "constant", "descending"]


def order_column(n, t, flaw, pair=None):
    """a strictly ascending column with exactly one flaw: row pair[1] equal to row pair[0] (repeat) or one below it (descent; the rows
    behind it ascend again) - or, without a pair, the whole column untouched, constant or descending"""
    col = ascending(n, t)
    if flaw == "constant":
        col[:] = col[n // 2]
    elif flaw == "descending":
        col = np.ascontiguousarray(col[::-1])
    elif flaw in ("repeat", "descent"):
        a, b = pair
        assert b == a + 1 and b < n
        col[b] = col[a] - (1 if flaw == "descent" else 0)
    else:
        assert flaw == "untouched"
    return col


def order_cases():
    """(id, rows, flaw, pair): every case is one table of three columns, one per element type of k_minmax"""
    out = [(f"{flaw}_{a}_{b}", BIG, flaw, (a, b)) for a, b in ORDER_PAIRS for flaw in ORDER_FLAWS]
    out += [(f"{flaw}_{n}", n, flaw, None) for flaw in ORDER_WHOLE for n in (BIG, 2, 1)]
    return out


def order_columns(n, flaw, pair):
    return [(f"k_{t[0].lower()}", t, order_column(n, t, flaw, pair)) for t in ORDER_TYPES]


def order_expectation(n, flaw):
    """(ascending, strict) as the case is constructed - the reference must say the same"""
    if n == 1 or flaw == "untouched":
        return (1, 1)
    return {"repeat": (1, 0), "constant": (1, 0), "descent": (0, 0), "descending": (0, 0)}[flaw]


# ---- extremes -----------------------------------------------------------------------------------------------------------------------
EXTREME_ROWS = [0, STRIDE, BIG - 1]
EXTREME_VALUES = {"INT": (INT32_MIN, INT32_MAX), "DATE": (0, (1 << 32) - 1), "BIGINT": (INT64_MIN, INT64_MAX)}
DATE_MIDDLE = 1 << 31           # every DATE column of these cases holds it: read signed it would be the minimum


def extreme_cases():
    """(id, which, row): the minimum (which 0) or the maximum (1) of each type alone in one row"""
    return [(f"{'min' if which == 0 else 'max'}_row{row}", which, row) for which in (0, 1) for row in EXTREME_ROWS]


def extreme_columns(which, row, n=BIG):
    rng = np.random.default_rng(77 + row + which)
    i = rng.integers(-5, 6, n).astype(np.int32)
    d = (DATE_MIDDLE + rng.integers(0, 7, n)).astype(np.uint32)
    d[(row + 1) % n] = DATE_MIDDLE
    b = rng.integers(-5, 6, n).astype(np.int64)
    i[row], d[row], b[row] = (EXTREME_VALUES[k][which] for k in ("INT", "DATE", "BIGINT"))
    return [("x_int", INT, i), ("x_date", DATE, d), ("x_big", BIGINT, b)]


SPANS = [255, 256, 65535, 65536, (1 << 32) - 1, 1 << 32]
SPAN_WIDTHS = [1, 2, 2, 4, 4, 0]
SPAN_BASES = {"negative": lambda span: -1000, "bottom": lambda span: INT64_MIN + 1, "top": lambda span: INT64_MAX - 1 - span}


def span_columns(where, n=STRIDE + 1):
    """BIGINT and DECIMAL columns whose max - min is exactly each of SPANS, from a negative base, from the base next to INT64_MIN and up to
    the value next to INT64_MAX; the maximum in row 0, the minimum in the last row (the first row of the second stride)"""
    cols = []
    for k, span in enumerate(SPANS):
        base = SPAN_BASES[where](span)
        rng = np.random.default_rng(500 + k)
        off = rng.integers(0, min(span, 1 << 62) + 1, n, dtype=np.uint64)
        off[0], off[-1] = span, 0
        v = (off + np.uint64(base & 0xffffffffffffffff)).view(np.int64)          # (modulo 2^64: base + off as int64)
        cols.append((f"s{k}", BIGINT if k % 2 == 0 else DECIMAL, v))
    return cols


# ---- byte sets ----------------------------------------------------------------------------------------------------------------------
BYTE_SETS = [[0], [255], [31, 32], [0, 255], list(range(256))]


def byteset_columns(n=STRIDE + 1):
    """every set as CHAR(1) and as BOOL, each value of a set in at least one row; then a value that only row 0 holds and one that only the
    last row holds"""
    cols = []
    for k, s in enumerate(BYTE_SETS):
        rng = np.random.default_rng(900 + k)
        v = rng.choice(np.array(s, dtype=np.uint8), n)
        at = rng.permutation(n)[:len(s)] if n >= len(s) else np.arange(n)
        v[at] = np.array(s, dtype=np.uint8)[:len(at)]
        cols += [(f"c_set{k}", CHAR1, v), (f"o_set{k}", BOOL, v.copy())]
    first = np.full(n, ord("A"), dtype=np.uint8)
    first[0] = ord("Z")
    last = np.full(n, 200, dtype=np.uint8)
    last[-1] = 7
    for name, v in (("first", first), ("last", last)):
        cols += [(f"c_{name}", CHAR1, v), (f"o_{name}", BOOL, v.copy())]
    return cols


# ---- dictionaries -------------------------------------------------------------------------------------------------------------------
DICT_WIDTHS = [2, 10, 200]
DICT_ROWS = [1, 77, SAMPLE, SAMPLE + 1, 300_000]
DICT_COUNTS = [1, 2, 256, 257]
LONG = 300_000


def dict_values(count, W, seed=0):
    """`count` distinct W-byte values, none of them all zero, in no particular order"""
    rng = np.random.default_rng(40 + seed)
    ids = rng.permutation(60000)[:count] + 1
    v = np.zeros((count, W), dtype=np.uint8)
    v[:, 0], v[:, W - 1] = ids & 0xff, ids >> 8          # (the first and the last byte tell them apart ...)
    if W > 2:
        v[:, 1:W - 1] = rng.integers(32, 127, (1, W - 2))          # (... and everything between is the same in all of them)
    assert len(np.unique(v, axis=0)) == count
    return v


def dict_spread(n, vals, seed=0):
    """n rows over all of `vals` (as many of them as there are rows), shuffled"""
    rng = np.random.default_rng(seed)
    return vals[rng.permutation(np.arange(n) % len(vals))]


def dict_grid_cases():
    """(rows, values, W): every row count with every number of values at W 2 and 10; at W 200 the counts around the limit at the sizes
    around the sample (a 300 000-row column of that width is 60 MB)"""
    out = [(n, c, W) for W in (2, 10) for n in DICT_ROWS for c in DICT_COUNTS if c <= n]
    out += [(n, c, 200) for n in (1, 77, SAMPLE + 1) for c in (1, 256, 257) if c <= n]
    return out


def dict_late_value(n, W, at):
    """256 values all over the column and a 257th whose first row is `at`: with at >= SAMPLE the sample pass finds a column that fits"""
    vals = dict_values(257, W, seed=5)
    col = dict_spread(n, vals[:256], seed=at)
    col[at] = vals[256]
    return col


def dict_few_per_workgroup(W, n=LONG):
    """value = row // 1024: 293 values, at most three in the rows of any workgroup (256 rows per round, rounds 512 * 256 rows apart) - no
    sample and no workgroup can refuse the column, only the union pass"""
    vals = dict_values((n + 1023) // 1024, W, seed=6)
    return vals[np.arange(n) // 1024]


def dict_one_value_per_workgroup(n, W):
    """256 values, every workgroup of the per-workgroup pass holds exactly one: the union is exactly full.  Workgroup b takes rows
    b * 256 + l + k * grid * 256.  With SAMPLE rows there are 256 workgroups of one round and no two share a value; a longer column has
    512 workgroups, more than there are values, so there workgroups b and b + 256 hold the same one."""
    grid = min(DICT_COLLECT_GRID, (n + 255) // 256)
    vals = dict_values(256, W, seed=7)
    return vals[((np.arange(n) // 256) % grid) % 256]


def dict_257_in_one_workgroup(W, n=LONG):
    """257 values of which exactly one workgroup of the per-workgroup pass sees every one - and no pass sees more: rows 0..255 hold 256
    values, row DICT_COLLECT_GRID * 256 (the same workgroup's second round, behind the sample) the 257th, every other row the first value.
    The sample finds 256.  Workgroup 0 counts 257, one past the limit and no further, and has to say so: without it the union of the others
    is a dictionary of one value"""
    vals = dict_values(257, W, seed=8)
    col = np.repeat(vals[:1], n, axis=0)
    col[:256] = vals[:256]
    col[DICT_COLLECT_GRID * 256] = vals[256]
    return col


def dict_bytewise_values(W=10):
    """values that differ only in their last byte, only behind a NUL, only in trailing spaces / NULs: all distinct entries"""
    def v(b):
        assert len(b) == W
        return np.frombuffer(b, dtype=np.uint8)
    stem = b"abcdefghijklmnopqrstuvwxyz"[:W - 1]
    raw = [stem + b"\x01", stem + b"\x02", stem + b"\xff", stem + b" ", stem + b"\x00",
           b"ab\x00" + stem[:W - 4] + b"x", b"ab\x00" + stem[:W - 4] + b"y",
           b"ab" + b" " * (W - 2), b"ab" + b" " * (W - 3) + b"\x00", b"ab" + b"\x00" * (W - 2), b"ab " + b"\x00" * (W - 3),
           b"\x00" * W, b"\x00" * (W - 1) + b"\x01", b"\xff" * W]
    out = np.stack([v(b) for b in raw])
    assert len(np.unique(out, axis=0)) == len(out)
    return out


def dict_colliding_values(W=10, group=5):
    """two groups of `group` values found by search: one whose members share a hash slot below 1023 (they probe linearly past each other),
    one whose slot is 1023 (the probe wraps to slot 0) - and one value each in slots 0 and 1, where the wrapped probes land"""
    cand = np.zeros((40000, W), dtype=np.uint8)
    text = np.array([list(f"k{i:0{W - 1}d}".encode()[:W]) for i in range(len(cand))], dtype=np.uint8) if W >= 6 else None
    if text is not None:
        cand[:] = text
    else:
        cand[:, 0], cand[:, W - 1] = np.arange(len(cand)) & 0xff, np.arange(len(cand)) >> 8
    slots = fnv_slots(cand)
    counts = np.bincount(slots, minlength=DICT_SLOTS)
    common = 2 + int(np.argmax(counts[2:DICT_SLOTS - 1] >= group))
    assert counts[common] >= group and counts[DICT_SLOTS - 1] >= group and counts[0] >= 1 and counts[1] >= 1
    pick = lambda s, k: cand[np.flatnonzero(slots == s)[:k]]
    return pick(common, group), pick(DICT_SLOTS - 1, group), np.concatenate([pick(0, 1), pick(1, 1)])


def dict_cases():
    """[(id, function that makes the table's columns)]: every dictionary case, table by table (made when asked for: some are tens of MB)"""
    out = []
    grid = dict_grid_cases()
    for W in DICT_WIDTHS:
        for n in sorted({n for n, _, w in grid if w == W}):
            counts = [c for m, c, w in grid if (m, w) == (n, W)]
            out.append((f"grid_w{W}_n{n}", lambda W=W, n=n, counts=counts: [
                (f"v{c}", ("VARCHAR" if c % 2 else "CHAR", W), dict_spread(n, dict_values(c, W, seed=c), seed=n)) for c in counts]))
    for W in (2, 10):
        for n, at in ((SAMPLE + 1, SAMPLE), (LONG, SAMPLE), (LONG, LONG - 1)):
            out.append((f"late_w{W}_n{n}_at{at}", lambda W=W, n=n, at=at: [("v", ("CHAR", W), dict_late_value(n, W, at))]))
        out.append((f"257_in_one_workgroup_w{W}", lambda W=W: [("v", ("CHAR", W), dict_257_in_one_workgroup(W))]))
        out.append((f"few_per_workgroup_w{W}", lambda W=W: [("v", ("VARCHAR", W), dict_few_per_workgroup(W))]))
        for n in (SAMPLE, LONG):
            out.append((f"one_per_workgroup_w{W}_n{n}", lambda W=W, n=n: [("v", ("CHAR", W), dict_one_value_per_workgroup(n, W))]))

    def bytewise():
        vals = dict_bytewise_values(10)
        return [("c", ("CHAR", 10), dict_spread(3000, vals, seed=1)), ("v", ("VARCHAR", 10), dict_spread(3000, vals, seed=2))]

    def collisions():
        common, wrap, landing = dict_colliding_values(10)
        fill = dict_values(200, 10, seed=9)
        return [("a", ("CHAR", 10), dict_spread(5000, np.concatenate([common, wrap, landing]), seed=3)),
                ("b", ("CHAR", 10), dict_spread(5000, np.concatenate([wrap, landing, common, fill]), seed=4))]
    return out + [("bytewise", bytewise), ("collisions", collisions)]


# ---- appends ------------------------------------------------------------------------------------------------------------------------
def append_cases():
    """[(id, [columns of the table, columns of the first append, ...])]: the seam between a table and the rows appended to it lies between
    rows STRIDE - 1 and STRIDE.  A repeat and a descent exactly there; rows that widen the narrow images 1 -> 2 -> 4 bytes -> none; a
    dictionary that grows (every code changes) and then meets its 257th value"""
    out = []
    for flaw in ("repeat", "descent", "untouched"):
        whole = order_columns(STRIDE + 300, flaw, (STRIDE - 1, STRIDE) if flaw != "untouched" else None)
        out.append((f"seam_{flaw}", [[(n, t, c[:STRIDE]) for n, t, c in whole], [(n, t, c[STRIDE:]) for n, t, c in whole]]))
    rng = np.random.default_rng(8)
    small = lambda k, dt: rng.integers(0, 200, k).astype(dt)
    parts = []
    for k, top in ((1000, None), (3, 60_000), (2, 1 << 31), (1, 1 << 40)):
        b, m, d, i = small(k, np.int64), small(k, np.int64) - 100, small(k, np.uint32) + 19940101, small(k, np.int32)
        if top is not None:
            b[-1] = m[-1] = top
            d[-1] = 19940101 + min(top, 70_000)
            i[-1] = min(top, 70_000)
        parts.append([("b", BIGINT, b), ("m", DECIMAL, m), ("d", DATE, d), ("i", INT, i)])
    out.append(("widen", parts))
    vals = dict_values(257, 10, seed=11)
    vals = vals[np.lexsort(vals.T[::-1])]                   # (in memcmp order, so that the values appended first go in FRONT of the old ones)
    out.append(("dictionary_grows", [[("s", ("CHAR", 10), dict_spread(900, vals[100:103], seed=1))],
                                     [("s", ("CHAR", 10), dict_spread(50, vals[:2], seed=2))],
                                     [("s", ("CHAR", 10), dict_spread(800, vals[2:256], seed=3))],
                                     [("s", ("CHAR", 10), vals[256:257].copy())],
                                     [("s", ("CHAR", 10), vals[256:257].copy())]]))
    return out


def appended(parts, k):
    """the columns of a table after the first k appends"""
    return [(name, t, np.concatenate([p[c][2] for p in parts[:k + 1]])) for c, (name, t, _) in enumerate(parts[0])]


# ---- tables -------------------------------------------------------------------------------------------------------------------------
def to_type(t):
    from resql_amd import plan as P
    T = P.TypeInit
    return {"INT": T.INT, "DATE": T.DATE, "BIGINT": T.BIGINT, "BOOL": T.BOOL}[t[0]]() if len(t) == 1 else getattr(T, t[0])(*t[1:])


def to_table(name, cols):
    """the columns as a plan.Table (what Context.table uploads)"""
    from resql_amd import plan as P
    n = len(cols[0][2])
    assert all(len(c[2]) == n for c in cols)
    return P.Table(name, [P.Column(cn, to_type(t), np.ascontiguousarray(data)) for cn, t, data in cols], n)



# ---- the comparison -----------------------------------------------------------------------------------------------------------------
def first_difference(got, want):
    got, want = np.frombuffer(bytes(got), dtype=np.uint8), np.frombuffer(bytes(want), dtype=np.uint8)
    if len(got) != len(want):
        return f"{len(got)} bytes for {len(want)}"
    at = np.flatnonzero(got != want)
    return "equal" if len(at) == 0 else f"{len(at)} bytes differ, the first at {int(at[0])}: {int(got[at[0]])} for {int(want[at[0]])}"


def assert_table_matches(dt, cols, device, dict_scans=False, owned=True):
    """everything an engine.DeviceTable `dt` made from `cols` keeps of them equals the references: the statistics blob, image_info, the
    dictionary entries - and, on a device, the narrow image and the codes.  Returns the blob's bytes."""
    raw = dt.stats_blob()
    blob = parse_blob(raw)
    n = len(cols[0][2]) if cols else 0
    assert (blob["magic"], blob["n_cols"], blob["row0"], blob["n_rows"]) == (STATS_MAGIC, len(cols), 0, n)
    for k, (name, t, data) in enumerate(cols):
        ref = column_reference(data, t, owned, dict_scans)
        assert blob["cols"][k] == ref["stats"], (name, t, "statistics (valid, ascending, strict, min, max, bytes)", blob["cols"][k], ref["stats"])
        width, base, image = ref["narrow"]
        entries, codes = ref["dict"] if ref["dict"] is not None else (np.zeros((0, 1), dtype=np.uint8), np.zeros(0, dtype=np.uint8))
        assert dt.image_info(name) == (width, base, len(entries), n), (name, t, "image_info", dt.image_info(name), (width, base, len(entries), n))
        got = dt.read_image(name, 1)
        assert got.tobytes() == entries.tobytes(), (name, "dictionary entries", first_difference(got, entries))
        if device:
            got = dt.read_image(name, 0)
            assert got.tobytes() == image, (name, t, f"narrow image of {width} bytes from {base}", first_difference(got, image))
            got = dt.read_image(name, 2)
            assert got.tobytes() == codes.tobytes(), (name, "dictionary codes", first_difference(got, codes))
    return raw
