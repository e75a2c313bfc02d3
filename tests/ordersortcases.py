"""Tables and statements of the ORDER BY tests (tests/test_order_sort_host.py, tests/test_gpu_order_sort.py,
tests/test_gpu_order_sort_prim.py): plans without an aggregation whose root is an ORDER BY directly above the materialisation, sorted on
the device under Context.set_order_sort(1).

As tests/orderlimitcases.py explains, every key is scrambled, never sorted, and every key list that must not tie ends in a unique key:
the reference's quicksort is quadratic on sorted input and on ties.  The tables that tie do so in groups of a few dozen rows.  Results of
up to 256 KB of cells come back through host-mapped memory (fallback SMALL); the tables of the other cases hold 70 000 rows and more."""
import numpy as np

from resql_amd import engine, plan as P

import orderlimitcases as O

T = P.TypeInit
NONE, SHAPE, SMALL, DOES_NOT_FIT, TIES, ORDER_LIMIT = (engine.ORDER_SORT_FALLBACK_NONE, engine.ORDER_SORT_FALLBACK_SHAPE, engine.ORDER_SORT_FALLBACK_SMALL,
                                                       engine.ORDER_SORT_FALLBACK_DOES_NOT_FIT, engine.ORDER_SORT_FALLBACK_TIES,
                                                       engine.ORDER_SORT_FALLBACK_ORDER_LIMIT)
I32_MIN, I32_MAX, I64_MIN, I64_MAX = O.I32_MIN, O.I32_MAX, O.I64_MIN, O.I64_MAX
ROWS = 70_001


def wide_table(n=ROWS):
    """w: a BIGINT over its whole range, both ends among the values, about 3 rows per value; u: a unique INT - 64 + 17 bits, two words"""
    step = np.uint64((2**64 - 16) // (n // 3))          # (unsigned arithmetic, then read as signed: 2^63 + 5 is I64_MIN + 5)
    w = ((O.scramble(n, 2246822519, 0) % np.uint64(n // 3)) * step + np.uint64(2**63 + 5)).view(np.int64)
    w[17] = I64_MIN
    w[n - 3] = I64_MAX
    return P.Table("wide", [P.Column("w", T.BIGINT(), w), P.Column("u", T.INT(), O.unique_ints(n)),
                            P.Column("s", T.VARCHAR(9), np.array([b"p%d" % (i % 613) for i in range(n)], dtype="S9"))], n)


def flag_table(n=ROWS):
    """flag: 1000 values of about 70 rows each - adjacent rows of any order by flag alone tie"""
    return P.Table("flags", [P.Column("flag", T.INT(), (O.scramble(n) % np.uint64(1000)).astype(np.int32)), P.Column("u", T.INT(), O.unique_ints(n))], n)


def tail_ties_table(n=ROWS):
    """g: the values 0 .. 999 once each, the others in groups of about 14 - an order by g ties from its row 1000 on and nowhere before"""
    r = (np.arange(n, dtype=np.int64) * 40503 + 77) % n          # a bijection of 0 .. n - 1: 40503 and n have no common factor
    assert n == ROWS and len(np.unique(r)) == n
    g = np.where(r < 1000, r, 1000 + r % 5000).astype(np.int32)
    return P.Table("tailties", [P.Column("g", T.INT(), g), P.Column("u", T.INT(), O.unique_ints(n))], n)


TABLES = {"t": O.main_table, "wide": wide_table, "flags": flag_table, "tailties": tail_ties_table, "same": O.one_value_table, "shapes": O.shape_table}

# (statement, the table it reads, order_limit's setting, path, fallback reason) under set_order_sort(1) - every case names what it expects
DEVICE = [
    ("select k, u, c25, v from t order by k, u", "t", 0, 1, NONE),                                   # ascending; CHAR and VARCHAR payload
    ("select k, u, c25, v from t order by k desc, u desc", "t", 0, 1, NONE),                         # descending
    ("select d, k, u from t order by d desc, k, u", "t", 0, 1, NONE),                                # mixed, three keys, a DATE at and above 2^31
    ("select a * 2 - b as x, u from t order by x desc, u", "t", 0, 1, NONE),                         # a projected key
    ("select k, u, v from t where f < 80 order by k desc, u", "t", 0, 1, NONE),                      # behind a WHERE
    ("select k, u, c25 from t order by k, u limit 50000", "t", 0, 1, NONE),
    ("select k, u, c25 from t order by k, u limit 2000000", "t", 0, 1, NONE),                        # above order_limit's 2^20: out_rows = rows
    ("select k, u, c25 from t order by k, u limit 2000000", "t", 1, 1, NONE),                        # ... which order_limit does not plan
    ("select k, u from t order by k, u limit 10", "t", 1, 0, ORDER_LIMIT),                           # order_limit decides first
    ("select k, u from same order by k, u limit 10", "same", 1, 1, NONE),                            # its OVERFLOW: this path decides
    ("select w, u, s from wide order by w, u", "wide", 0, 1, NONE),                                  # two words
    ("select w, u, s from wide order by w desc, u limit 7", "wide", 0, 1, NONE),
    ("select g, u from tailties order by g limit 1000", "tailties", 0, 1, NONE),                     # ties only behind row k + 1: the pair at (k, k + 1)
    ("select g, u from tailties order by g limit 0", "tailties", 0, 1, NONE),                        # a relation of no rows
]
HOST = [
    ("select flag, u from flags order by flag", "flags", 0, 0, TIES),
    ("select g, u from tailties order by g limit 1001", "tailties", 0, 0, TIES),                     # the pair at (k - 1, k) ties
    ("select c25, u from t order by c25, u", "t", 0, 0, SHAPE),                                      # a string key
    ("select k, c25, u from t order by k, c25, u limit 20", "t", 0, 0, SHAPE),                       # ... in a later position
    ("select i, g from shapes order by g desc, i", "shapes", 0, 0, SMALL),                           # 400 rows
    ("select k, u, c25, v from t where f > 1000 order by k desc, u", "t", 0, 0, SMALL),              # no row passes
]

# (statement over `shapes`, planned, keys) for the compile-time report
PLANNED = [
    ("select i, g from shapes order by g desc, i", 1, 2),                         # no LIMIT
    ("select i, m from shapes order by m, i limit 0", 1, 2),
    ("select i, dt from shapes order by dt, i limit 10", 1, 2),
    ("select i, dt from shapes order by dt, i limit 1048577", 1, 2),              # beyond order_limit's 2^20
    ("select i, g, m, dt from shapes order by g, m, dt, i, g desc, m desc, dt desc, i desc", 1, 8),
    ("select i, g, m, dt from shapes order by g, m, dt, i, g desc, m desc, dt desc, i desc, g", 0, 0),      # 9 keys
    ("select g, count(*) as n from shapes group by g order by g", 0, 0),         # an aggregation
    ("select s, i from shapes order by s, i", 0, 0),                              # CHAR(n) first
    ("select i, s from shapes order by i, s", 0, 0),                              # ... and later
    ("select w, i from shapes order by w, i", 0, 0),                              # VARCHAR(n)
    ("select i, w from shapes order by i, w", 0, 0),
    ("select o, i from shapes order by o, i", 0, 0),                              # BOOL
    ("select i, o from shapes order by i, o", 0, 0),
    ("select c, i from shapes order by c, i", 0, 0),                              # CHAR(1)
    ("select i, c from shapes order by i, c", 0, 0),
    ("select i * 3 - g as x, i from shapes order by x, i", 1, 2),                 # a projected expression
    ("select i, g from shapes", 0, 0),                                            # no ORDER BY
    ("select i, g from shapes limit 5", 0, 0),                                    # ... the materialisation's own LIMIT
]

# (a key list of which no key varies - TIES without a sort - is the primitive's test: the host's quicksort is quadratic over equal rows, and a
# result that is not SMALL holds tens of thousands of them)

# what the unmodified reference answers (tests/golden/order_sort_reference.json, made by tests/golden/make_order_sort_golden.py): over the
# eight-table database at SF 0.01.  Every key list ends in the table's unique key; lineitem and orders are generated in that key's order, so
# it never stands first.
GOLD_SF = 0.01
# (statement, path, reason under set_order_sort(1))
GOLD = [
    ("select l_orderkey, l_linenumber, l_extendedprice from lineitem order by l_extendedprice desc, l_orderkey, l_linenumber", 1, NONE),
    ("select l_orderkey, l_linenumber, l_extendedprice, l_shipdate, l_shipmode from lineitem where l_shipdate < date '1994-01-01' "
     "order by l_extendedprice desc, l_orderkey, l_linenumber", 1, NONE),
    ("select l_orderkey, l_linenumber, l_shipdate, l_comment from lineitem order by l_shipdate desc, l_orderkey desc, l_linenumber limit 40000", 1, NONE),
    ("select o_orderkey, o_totalprice, o_orderdate, o_comment from orders order by o_totalprice, o_orderkey", 1, NONE),
    ("select l_orderkey, l_linenumber, l_extendedprice * (1 - l_discount) as revenue from lineitem order by revenue desc, l_orderkey, l_linenumber limit 2000000", 1, NONE),
    ("select o_orderkey, o_custkey from orders where o_orderdate < date '1995-01-01' order by o_custkey desc, o_orderkey limit 5", 0, SMALL),      # 56 KB of cells
]
GOLD_STATEMENTS = [g[0] for g in GOLD]


GOLD_FULL_TEXT_BYTES = 100_000          # a recorded answer longer than this is kept as its SHA-1, its first and its last lines


def gold_matches(case, text):
    """is `text` the answer recorded in `case` of tests/golden/order_sort_reference.json?"""
    import hashlib
    if case["result"] is not None:
        return text == case["result"]
    return hashlib.sha1(text.encode()).hexdigest() == case["sha1"] and text.startswith(case["head"]) and text.endswith(case["tail"])


def warm_statements():
    """(SQL text, host tables) of every statement tests/test_gpu_order_sort.py compiles with kernels of its own, for the build's
    code-object warm-up (a compile-only context)"""
    host = {k: make() for k, make in TABLES.items()}
    out = [(sql, [host[name]]) for sql, name, *_ in DEVICE + HOST]
    from resql_amd import tpch_full
    db = tpch_full.database(GOLD_SF)
    return out + [(sql, [db[k] for k in sorted(db)]) for sql in GOLD_STATEMENTS]


def image(key, desc):
    """order_sort.h in numpy: the key's image as uint64 in which earlier is smaller - sign-extended, key ^ 2^63, complemented for
    descending order"""
    u = key.astype(np.int64).view(np.uint64) ^ np.uint64(1 << 63)
    return ~u if desc else u


def expected_order(keys, descending, lead):
    """(the stable order by the keys' images - numpy.lexsort takes the last key first -, the positions i, i + 1 < lead, whose rows are
    equal on every key, the bits per key, the 64-bit words)"""
    images = [image(k, d) for k, d in zip(keys, descending)]
    n = len(images[0])
    perm = np.lexsort(images[::-1]).astype(np.uint32) if n else np.zeros(0, dtype=np.uint32)
    tied = 0
    if lead > 1:
        same = np.ones(lead - 1, dtype=bool)
        for im in images:
            same &= im[perm[:lead - 1]] == im[perm[1:lead]]
        tied = int(same.sum())
    bits = [int(int(im.max()) - int(im.min())).bit_length() if n else 0 for im in images]
    return perm, tied, bits + [0] * (8 - len(bits)), (sum(bits) + 63) // 64
