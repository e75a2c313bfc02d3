"""Row stores for the bridge tests (rsq_table_from_rowstore_ex): ReSQL's tuple layout packed with numpy, the EDGE schema and its
values, and the two yardsticks - (a) the source columns with the NUL rule applied in numpy, (b) the host path's columns and statistics.
No tests here."""
import numpy as np

from resql_amd import engine, plan as P
from resql_amd.plan import TypeInit as T

TILE_BYTES = 49152          # the kernel's LDS tile: min(256, TILE_BYTES // tuple size) rows per workgroup


def is_string(t: P.SqlType) -> bool:
    return t.tag in (P.CHAR, P.VARCHAR)


def field_size(t: P.SqlType) -> int:
    """sizeInTuple(type, strings by value): BOOL 1, INT / DATE 4, BIGINT / DECIMAL 8, CHAR(1) 2, CHAR(n) / VARCHAR(n) n + 1"""
    return t.len + 1 if is_string(t) else t.width


def tuple_size(schema: P.Table) -> int:
    return sum(field_size(c.type) for c in schema.columns)


def bare(name: str, fields) -> P.Table:
    """a schema: (column name, type) pairs, no data"""
    return P.Table(name, [P.Column(n, t) for n, t in fields], 0)


def cell_bytes(t: P.SqlType, column: np.ndarray) -> np.ndarray:
    """a column's cells as [n, width] bytes"""
    raw = np.frombuffer(np.ascontiguousarray(column).tobytes(), dtype=np.uint8)
    return raw.reshape(-1, t.width) if t.width else raw.reshape(len(column), 0)


def expected_column(t: P.SqlType, column: np.ndarray) -> bytes:
    """yardstick (a): the column a bridge must produce from `column`'s values - a string ends at its first NUL, zeros behind it"""
    cells = cell_bytes(t, column)
    if is_string(t) and cells.size:
        cells = cells * np.minimum.accumulate(cells != 0, axis=1)
    return cells.astype(np.uint8).tobytes()


def pack(schema: P.Table, columns, block_bytes=None, first_offset: int = 0, junk: bool = True, seed: int = 11):
    """`columns` (one array per column of `schema`, in its order) as a list of blocks of packed tuples.  A block holds block_bytes
    bytes - as many whole tuples as fit and a remainder shorter than a tuple (block_bytes None: one block of all tuples and a
    remainder); the last block holds what is left, and a remainder too.  The blocks are views into one buffer, the first of them
    first_offset bytes behind a 64-byte boundary.  junk: the bytes behind every string's first NUL, the byte behind a string of
    full length and the second byte of CHAR(1) are seeded non-zero bytes."""
    n = len(columns[0]) if columns else 0
    ts = tuple_size(schema)
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, ts), dtype=np.uint8)
    off = 0
    for c, col in zip(schema.columns, columns):
        assert len(col) == n
        src = cell_bytes(c.type, col)
        if is_string(c.type):
            ln = c.type.len
            field = np.zeros((n, ln + 1), dtype=np.uint8)
            if junk:
                live = np.minimum.accumulate(src != 0, axis=1)
                field[:] = rng.integers(1, 256, size=(n, ln + 1), dtype=np.uint8)
                field[:, :ln] = np.where(live, src, field[:, :ln])
                first_nul = live.sum(axis=1)
                ends = np.nonzero(first_nul < ln)[0]
                field[ends, first_nul[ends]] = 0
            else:
                field[:, :ln] = src
            rows[:, off:off + ln + 1] = field
        else:
            rows[:, off:off + c.type.width] = src
        off += field_size(c.type)
    per = n if block_bytes is None else block_bytes // ts
    assert block_bytes is None or per >= 1, "a block holds at least one tuple"
    counts = []
    left = n
    while True:
        take = min(per, left)
        counts.append(take)
        left -= take
        if left == 0:
            break
    sizes = []
    for i, cnt in enumerate(counts):
        full = block_bytes is not None and cnt == per
        sizes.append(block_bytes if full else cnt * ts + min(ts - 1, 5))
    buf = np.zeros(first_offset + sum(sizes) + 128, dtype=np.uint8)
    base = (-buf.ctypes.data) % 64 + first_offset
    blocks, at, r = [], base, 0
    for cnt, size in zip(counts, sizes):
        block = buf[at:at + size]
        block[:cnt * ts] = rows[r:r + cnt].reshape(-1)
        block[cnt * ts:] = rng.integers(1, 256, size=size - cnt * ts, dtype=np.uint8)
        blocks.append(block)
        at += size
        r += cnt
    return blocks


def strings(values, ln: int) -> np.ndarray:
    """byte strings as a CHAR(ln) / VARCHAR(ln) column, every byte kept (interior NULs too)"""
    out = np.zeros((len(values), ln), dtype=np.uint8)
    for i, v in enumerate(values):
        assert len(v) <= ln
        out[i, :len(v)] = np.frombuffer(v, dtype=np.uint8)
    return out.view(f"S{ln}").reshape(len(values)) if ln > 1 else out.reshape(len(values))


# BOOL, CHAR(1), INT, CHAR(7), BIGINT, DATE, VARCHAR(25), DECIMAL(15,2): a tuple of 1 + 2 + 4 + 8 + 8 + 4 + 26 + 8 = 61 bytes - odd, the
# BIGINT at offset 15, the DECIMAL at 53
EDGE = bare("edge", [("e_flag", T.BOOL()), ("e_code", T.CHAR(1)), ("e_int", T.INT()), ("e_tag", T.CHAR(7)), ("e_big", T.BIGINT()),
                     ("e_date", T.DATE()), ("e_text", T.VARCHAR(25)), ("e_dec", T.DECIMAL(15, 2))])
assert tuple_size(EDGE) == 61

_INT_EDGES = [-2**31, 2**31 - 1, -1, 0, 1]
_BIG_EDGES = [-2**63, 2**63 - 1, -1, 0, 1 << 32]
_TAG_EDGES = [b"", b"ABCDEFG", b"ab\0cd", b"x", b"\0zzzzzz"]
_TEXT_EDGES = [b"", b"exactly twenty-five bytes", b"inner\0nul behind it", b"y", b"twenty-four bytes of it.", b"\0"]


def edge_columns(n: int, seed: int = 5):
    """n rows of EDGE: the first rows walk through the value edges (minima, maxima, -1, empty strings, strings of exactly len bytes,
    strings with an interior NUL), the rest is seeded"""
    rng = np.random.default_rng(seed)
    i = np.arange(n)

    def mix(edges, rest):
        out = np.array(rest)
        k = min(n, len(edges))
        out[:k] = edges[:k]
        return out

    flag = (i % 3 == 0).astype(np.uint8)
    code = np.frombuffer(b"ANRFO", dtype=np.uint8)[rng.integers(0, 5, size=n)]
    ints = mix(np.array(_INT_EDGES, dtype=np.int32), rng.integers(-2**31, 2**31, size=n, dtype=np.int64).astype(np.int32))
    bigs = mix(np.array(_BIG_EDGES, dtype=np.int64), rng.integers(-2**63, 2**63 - 1, size=n, dtype=np.int64))
    dates = (19920101 + rng.integers(0, 70000, size=n)).astype(np.uint32)
    decs = mix(np.array([-10**15 + 1, 10**15 - 1, -1, 0], dtype=np.int64), rng.integers(-10**14, 10**14, size=n, dtype=np.int64))
    alphabet = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz ,.", dtype=np.uint8)

    def texts(edges, ln):
        vals = []
        for r in range(n):
            if r < len(edges):
                vals.append(edges[r])
            else:
                vals.append(alphabet[rng.integers(0, len(alphabet), size=int(rng.integers(0, ln + 1)))].tobytes())
        return strings(vals, ln)

    return [flag, code, ints, texts(_TAG_EDGES, 7), bigs, dates, texts(_TEXT_EDGES, 25), decs]


def columns_of(dt: engine.DeviceTable, schema: P.Table) -> dict:
    if dt.n_rows == 0:          # (nothing to read: the host path's columns of no rows come without data)
        return {c.name: b"" for c in schema.columns}
    return {c.name: dt.read_column(c.name, c.type.np_dtype).tobytes() for c in schema.columns}


def expected_columns(schema: P.Table, columns) -> dict:
    return {c.name: expected_column(c.type, col) for c, col in zip(schema.columns, columns)}
