"""Tables and statements of tests/test_gpu_result_text.py: projections whose result cells hold the edge values of
tests/cpp/result_text_test.cpp (the tables are made from host columns), row counts on both sides of a workgroup's 256 rows, strings whose
rows of text lie on both sides of the 48 KiB LDS tile of resql_amd/csrc/result_text.hip, a table of 65 columns."""
import numpy as np

from resql_amd import plan as P

T = P.TypeInit
I64_MIN, I64_MAX = -2**63, 2**63 - 1
ROW_COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1000]

EDGE_SQL = "select ci, cb, d2, d0, d6, cd, cf, c1, c10, v25 from t"
STRINGS_SQL = "select k, a, b from t"
ALL_COLUMNS_SQL = "select * from t"          # (every column: a projection that lists them is limited to 32 expressions)


def _powers(top):
    return [s * (10**k + d) for k in range(top + 1) for d in (-1, 0, 1) for s in (1, -1)]


def _cycle(values, n, dtype, rng, lo, hi):
    """the edge values first, seeded values of every magnitude behind them"""
    out = np.empty(n, dtype=dtype)
    for i in range(n):
        if i < len(values):
            out[i] = values[i]
        else:
            span = int(rng.integers(1, 64))
            v = int(rng.integers(0, 2**62)) >> (63 - span)
            out[i] = max(lo, min(hi, v if rng.integers(0, 2) else -v))
    return out


def edge_table(n, seed=5, name="t"):
    """INT, BIGINT, DECIMAL(15,2), DECIMAL(18,0), DECIMAL(12,6), DATE, BOOL, CHAR(1), CHAR(10), VARCHAR(25)"""
    rng = np.random.default_rng(seed)
    i32 = [0, 1, -1, -2**31, 2**31 - 1] + [v for v in _powers(9) if -2**31 <= v < 2**31]
    i64 = [0, 1, -1, -2**31, 2**31 - 1, I64_MIN, I64_MAX, I64_MIN + 1] + _powers(18)
    dates = [0, 19920101, 99991231, 0xFFFFFFFF, (-19920101) & 0xFFFFFFFF, 19981201]
    chars10 = np.array([b"", b"full10char", b"ab   ", b"a", b" ", b"x\xff y"], dtype="S10")
    chars25 = np.array([b"", b"v" * 25, b"mid length", b"trailing  ", b"|"], dtype="S25")
    cols = [P.Column("ci", T.INT(), _cycle(i32, n, np.int32, rng, -2**31, 2**31 - 1)),
            P.Column("cb", T.BIGINT(), _cycle(i64, n, np.int64, rng, I64_MIN, I64_MAX)),
            P.Column("d2", T.DECIMAL(15, 2), _cycle(i64, n, np.int64, rng, I64_MIN, I64_MAX)),
            P.Column("d0", T.DECIMAL(18, 0), _cycle(i64[::-1], n, np.int64, rng, I64_MIN, I64_MAX)),
            P.Column("d6", T.DECIMAL(12, 6), _cycle(i64[3:], n, np.int64, rng, I64_MIN, I64_MAX)),
            P.Column("cd", T.DATE(), np.array([dates[i] if i < len(dates) else int(rng.integers(0, 2**32)) for i in range(n)], dtype=np.uint32)),
            P.Column("cf", T.BOOL(), np.array([(0, 1, 255, 1)[i % 4] for i in range(n)], dtype=np.uint8)),
            P.Column("c1", T.CHAR(1), np.array([(0, 65, 32, 255, 124)[i % 5] for i in range(n)], dtype=np.uint8)),
            P.Column("c10", T.CHAR(10), chars10[np.arange(n) % len(chars10)]),
            P.Column("v25", T.VARCHAR(25), chars25[(np.arange(n) * 3) % len(chars25)])]
    return P.Table(name, cols, n)


def strings_table(n, lengths, wide):
    """an id, a VARCHAR(100) and a VARCHAR(200) (or CHAR(200), which always prints 200 characters) whose row r holds lengths(r) and twice
    that many characters"""
    a = np.array([bytes([97 + (r + i) % 26 for i in range(min(100, lengths(r)))]) for r in range(n)], dtype="S100")
    b = np.array([bytes([65 + (r * 7 + i) % 26 for i in range(min(200, 2 * lengths(r)))]) for r in range(n)], dtype="S200")
    return P.Table("t", [P.Column("k", T.INT(), np.arange(n, dtype=np.int32)), P.Column("a", T.VARCHAR(100), a), P.Column("b", wide(200), b)], n)


def short_then_full_table():
    """512 rows: the first 256 hold up to 8 and 16 characters, the next 256 all 100 and 200"""
    return strings_table(512, lambda r: r % 9 if r < 256 else 100, T.VARCHAR)


def padded_table():
    """300 rows with a CHAR(200) column: 200 characters a row whatever the value holds"""
    return strings_table(300, lambda r: r % 101, T.CHAR)


def wide_table(n=10):
    return P.Table("t", [P.Column(f"c{i}", T.INT(), np.arange(n, dtype=np.int32) * (i + 1) - 5) for i in range(65)], n)


def warm_statements():
    """(SQL text, host tables) of every statement tests/test_gpu_result_text.py compiles with kernels of its own, for the build's
    code-object warm-up (a compile-only context)"""
    out = [(EDGE_SQL, [edge_table(n)]) for n in ROW_COUNTS + [300, 700]]
    out += [(STRINGS_SQL, [short_then_full_table()]), (STRINGS_SQL, [padded_table()]), (ALL_COLUMNS_SQL, [wide_table()])]
    return out
