"""Tables and statements of the result-pack tests (tests/test_result_pack_host.py, tests/test_gpu_result_pack.py): plans without an
aggregation, whose result tuples the device packs under Context.set_result_pack(1) (resql_amd/csrc/result_pack.hip).

The tables are numpy columns.  `big` has 70 001 rows - no multiple of any number of rows a workgroup takes - of every column type, strings
with trailing spaces among them, and a VARCHAR(400) that makes its rows wide: a materialisation whose output columns take up to 256 KB
lives in host-mapped memory and keeps the host path (SMALL), so the filter that passes one row in a hundred needs rows of more than
375 bytes to reach the device path over few rows.  Every key is scrambled with a multiplicative hash of the row number - never sorted:
the reference's quicksort takes its pivot from the segment's end and is quadratic on sorted input and on long runs of equal keys."""
import numpy as np

from resql_amd import engine, plan as P

T = P.TypeInit
NONE, SHAPE, SMALL, DOES_NOT_FIT, ORDER_LIMIT = (engine.RESULT_PACK_FALLBACK_NONE, engine.RESULT_PACK_FALLBACK_SHAPE, engine.RESULT_PACK_FALLBACK_SMALL,
                                                 engine.RESULT_PACK_FALLBACK_DOES_NOT_FIT, engine.RESULT_PACK_FALLBACK_ORDER_LIMIT)
MAPPED_BYTES = 256 << 10          # engine_pipelines.cpp allocMatCols: output columns of up to this many bytes are host-mapped
BIG_ROWS = 70_001


def scramble(n, mul=2654435761, shift=7):
    """a multiplicative hash of the row numbers 0..n-1, as uint64 values below 2^25"""
    return ((np.arange(n, dtype=np.uint64) * np.uint64(mul)) & np.uint64(0xffffffff)) >> np.uint64(shift)


def unique_ints(n):
    """n distinct int32 values in scrambled order: an odd multiplier is a bijection of the 2^17 residues"""
    assert n <= 1 << 17
    return ((np.arange(n, dtype=np.int64) * 40503 + 77) % (1 << 17)).astype(np.int32)


def big_table(n=BIG_ROWS, name="big"):
    """id: a unique INT; g: BIGINT of both signs; m: DECIMAL(15,2); dt: DATE; s: CHAR(10) and w: VARCHAR(12) of every length, with trailing
    spaces; o: BOOL; c: CHAR(1), NUL among its values; f: 100 values for the WHERE clauses and the join; z: eight rows per value (the
    leading rows of `order by z` tie); pad: VARCHAR(400), mostly short"""
    h = scramble(n)
    ids = unique_ints(n)
    pool10 = np.array([b"", b"full10char", b"ab   ", b"a", b" ", b"tail    ", b"x\xff y", b"mid len"], dtype="S10")
    pool12 = np.array([b"", b"v" * 12, b"trailing  ", b"|", b"two  words ", b"w"], dtype="S12")
    pool400 = np.array([bytes([65 + (i * 11 + j) % 26 for j in range((i * 29) % 401 if i % 8 == 0 else i % 23)]) + (b"  " if i % 5 == 0 else b"") for i in range(64)],
                       dtype="S400")
    pool400[1] = b"F" * 400          # (one value of the full width: no NUL in its cell)
    cols = [P.Column("id", T.INT(), ids),
            P.Column("g", T.BIGINT(), h.astype(np.int64) * 1_000_003_007 - 10_000_000_000_000_000),
            P.Column("m", T.DECIMAL(15, 2), (scramble(n, 40503, 3).astype(np.int64) - (1 << 27)) * 977),
            P.Column("dt", T.DATE(), (19920101 + scramble(n, 2246822519, 5) % np.uint64(2500)).astype(np.uint32)),
            P.Column("s", T.CHAR(10), pool10[(h % np.uint64(len(pool10))).astype(np.int64)]),
            P.Column("w", T.VARCHAR(12), pool12[(scramble(n, 668265263, 4) % np.uint64(len(pool12))).astype(np.int64)]),
            P.Column("o", T.BOOL(), (h % np.uint64(2)).astype(np.uint8)),
            P.Column("c", T.CHAR(1), np.array([0, 65, 32, 255, 124], dtype=np.uint8)[(scramble(n, 374761393, 9) % np.uint64(5)).astype(np.int64)]),
            P.Column("f", T.INT(), (scramble(n, 374761393, 11) % np.uint64(100)).astype(np.int32)),
            P.Column("z", T.INT(), (ids // 8).astype(np.int32)),
            P.Column("pad", T.VARCHAR(400), pool400[(scramble(n, 3266489917, 6) % np.uint64(len(pool400))).astype(np.int64)])]
    return P.Table(name, cols, n)


def small_table():
    return big_table(5, "small")


def dim_table():
    """the build side of the join: one row per value of big.f"""
    return P.Table("dim", [P.Column("dk", T.INT(), ((np.arange(100) * 37 + 11) % 100).astype(np.int32)),
                           P.Column("dname", T.CHAR(8), np.array([b"dim%d " % i for i in range(100)], dtype="S8")[(np.arange(100) * 37 + 11) % 100])], 100)


def gold_table(n=80):
    """the table of the reference's recorded answers (tests/golden/result_pack_reference.json): every column type, printable cells, and a
    VARCHAR(3900) of short values: few rows keep the recorded text small, and the wide column makes the output columns of a statement that
    selects it outgrow the host-mapped form"""
    h = scramble(n)
    pool10 = np.array([b"", b"full10char", b"ab   ", b"a", b" ", b"tail    ", b"mid len"], dtype="S10")
    pool12 = np.array([b"", b"v" * 12, b"trailing  ", b"two  words ", b"w"], dtype="S12")
    pool = np.array([b"", b"pad ", b"some padding", b"x", b"tail  ", b"ab", b"q" * 31], dtype="S3900")
    cols = [P.Column("id", T.INT(), unique_ints(n)),
            P.Column("g", T.BIGINT(), h.astype(np.int64) * 1_000_003_007 - 10_000_000_000_000_000),
            P.Column("m", T.DECIMAL(15, 2), (scramble(n, 40503, 3).astype(np.int64) - (1 << 27)) * 977),
            P.Column("dt", T.DATE(), (19920101 + scramble(n, 2246822519, 5) % np.uint64(28)).astype(np.uint32)),
            P.Column("s", T.CHAR(10), pool10[(h % np.uint64(len(pool10))).astype(np.int64)]),
            P.Column("w", T.VARCHAR(12), pool12[(scramble(n, 668265263, 4) % np.uint64(len(pool12))).astype(np.int64)]),
            P.Column("o", T.BOOL(), (h % np.uint64(2)).astype(np.uint8)),
            P.Column("c", T.CHAR(1), (65 + scramble(n, 374761393, 9) % np.uint64(5)).astype(np.uint8)),
            P.Column("f", T.INT(), (scramble(n, 374761393, 11) % np.uint64(100)).astype(np.int32)),
            P.Column("k", T.INT(), (scramble(n, 374761393, 11) % np.uint64(20)).astype(np.int32)),
            P.Column("pad", T.VARCHAR(3900), pool[(scramble(n, 3266489917, 6) % np.uint64(61) % np.uint64(len(pool))).astype(np.int64)])]
    return P.Table("gold", cols, n)


def gold_dim_table():
    """the build side of the recorded join: one row per value of gold.k - fewer rows than gold, unique keys"""
    return P.Table("gdim", [P.Column("dk", T.INT(), ((np.arange(20) * 7 + 3) % 20).astype(np.int32)),
                            P.Column("dname", T.CHAR(8), np.array([b"dim%d " % i for i in range(20)], dtype="S8")[(np.arange(20) * 7 + 3) % 20])], 20)


TABLES = {"big": big_table, "small": small_table, "dim": dim_table}
GOLD_TABLES = {"gold": gold_table, "gdim": gold_dim_table}
# the statements of tests/golden/result_pack_reference.json (make_result_pack_golden.py records what the reference answers): every column
# type; a filter; ORDER BY on a unique key without a LIMIT; ORDER BY with a LIMIT; the materialisation's own LIMIT; a hash join feeding
# the materialisation.  Each selects `pad`, so each one's output columns take more than MAPPED_BYTES and the device packs its tuples.
GOLD_STATEMENTS = [
    "select * from gold",
    "select id, g, s, o, pad from gold where f < 90",
    "select id, m, w, pad from gold order by id desc",
    "select id, g, dt, pad from gold order by dt, g desc, id limit 20",
    "select id, s, c, pad from gold limit 70",
    "select id, dname, m, pad from gold, gdim where k = dk",
]
ROW_BYTES = sum(c.type.width for c in big_table(1).columns)          # a row of `big` in the output columns of `select *`

# (name, statement, the tables it reads, set_order_limit, path, fallback reason, sorted_on_host) under set_result_pack(1): every case names
# what it expects.  The order-limit report's own expectation stands with the case that has one (test_gpu_result_pack.py).
CASES = [
    ("all", "select * from big", ["big"], 0, 1, NONE, 0),
    ("filter", "select * from big where f = 7", ["big"], 0, 1, NONE, 0),                      # one row in a hundred: the device path over few rows
    ("nothing", "select * from big where f > 1000", ["big"], 0, 0, SMALL, 0),                 # no row passes
    ("small", "select * from small", ["small"], 0, 0, SMALL, 0),                              # host-mapped output columns
    ("order", "select id, g, s, w, c from big order by id", ["big"], 0, 1, NONE, 1),          # unique keys, no LIMIT
    ("order_limit_host", "select id, g, s from big order by g desc, id limit 100", ["big"], 0, 1, NONE, 1),
    ("order_limit_device", "select id, g, s from big order by g desc, id limit 100", ["big"], 1, 0, ORDER_LIMIT, 0),
    ("ties", "select z, id, w from big order by z limit 5", ["big"], 1, 1, NONE, 1),          # order-limit says TIES; the quicksort over all rows decides
    ("own_limit", "select id, g, s, m from big limit 30000", ["big"], 0, 1, NONE, 0),         # the materialisation's own LIMIT
    ("join", "select id, dname, g, s from big, dim where f = dk", ["big", "dim"], 0, 1, NONE, 0),
    ("aggregation", "select f, count(*) as n from big group by f", ["big"], 0, 0, SHAPE, 0),
]
CASE_IDS = [c[0] for c in CASES]

# (statement over `big` and `dim`, planned) for the compile-time report
PLANNED = [
    ("select * from big", 1),
    ("select id, s from big where f = 7", 1),
    ("select id, g from big order by g desc, id", 1),
    ("select id, g from big order by g desc, id limit 10", 1),
    ("select id, g from big limit 10", 1),
    ("select id, dname from big, dim where f = dk", 1),
    ("select id * 3 - g as x, id from big", 1),
    ("select f, count(*) as n from big group by f", 0),                      # an aggregation
    ("select sum(g) as t from big", 0),
    ("select f, count(*) as n from big group by f order by n desc limit 3", 0),
]


def filter_rows(host):
    return int((host.col("f").data == 7).sum())


NESTED_LOOPS_SQL = "select id, g, s, dname from big, dim where dk < 2"          # on a context with RSQ_ENGINE_NESTED_LOOPS: every row of big beside two of dim


def nested_loops_rows(big, dim):
    """the rows NESTED_LOOPS_SQL answers with, as a sorted list of packed tuples (id INT, g BIGINT, s CHAR(10), dname CHAR(8): 32 bytes) -
    a model in numpy, the oracle has no nested-loops join"""
    keep = np.flatnonzero(dim.col("dk").data < 2)
    n = big.n_rows
    out = np.zeros((len(keep) * n, 32), dtype=np.uint8)
    for k, d in enumerate(keep):
        rows = out[k * n:(k + 1) * n]
        rows[:, 0:4] = big.col("id").data.view(np.uint8).reshape(n, 4)
        rows[:, 4:12] = big.col("g").data.view(np.uint8).reshape(n, 8)
        rows[:, 12:22] = np.frombuffer(big.col("s").data.tobytes(), dtype=np.uint8).reshape(n, 10)          # (numpy pads an S10 with NULs: the tuple's zeros)
        rows[:, 23:31] = np.frombuffer(dim.col("dname").data[d:d + 1].tobytes(), dtype=np.uint8)
    packed = out.tobytes()
    return sorted(packed[i:i + 32] for i in range(0, len(packed), 32))


def warm_statements():
    """(SQL text, host tables[, engine flags]) of every statement tests/test_gpu_result_pack.py compiles with kernels of its own, for the
    build's code-object warm-up (a compile-only context)"""
    host = {k: make() for k, make in TABLES.items()}
    out = [(sql, [host[t] for t in names]) for _, sql, names, *_ in CASES]
    out += [(sql, [host["big"]]) for sql in (TEXT_PLAIN, TEXT_OTHER, "select id, g from big")]
    gold = [make() for _, make in sorted(GOLD_TABLES.items())]
    out += [(sql, gold) for sql in GOLD_STATEMENTS]
    out += [(NESTED_LOOPS_SQL, [host["big"], host["dim"]], engine.ENGINE_NESTED_LOOPS)]          # (on a context with that engine flag)
    return out


# the text tests: a statement without an ORDER BY, of 449 bytes a tuple (chunks of 777 rows begin at odd byte offsets), and a different
# large statement that runs between A's execution and A's text (an ORDER BY's text: the `order` case)
TEXT_PLAIN = "select id, g, m, dt, s, w, pad from big"
TEXT_OTHER = "select g, pad, id from big where f < 50"
