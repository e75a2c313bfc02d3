"""Tables and statements of tests/test_dict_group_codegen.py and tests/test_gpu_dict_group.py: GROUP BY over dictionary-coded string
columns, whose code is the dense rank of the group (RSQ_DICT_SCANS=1).  Small inputs: the row counts around one tile, dictionaries
of 1 to 257 entries, the edge values of tests/dictcases.py at the widths 2, 9 and 25."""
import numpy as np

from resql_amd import plan as P

import dictcases as D

T = P.TypeInit

ROWS = 128 * 40 + 33                                                      # forty tiles and a tail
SHIPMODES = np.array([b"MAIL", b"SHIP", b"AIR", b"RAIL", b"TRUCK", b"FOB", b"REG AIR"], dtype="S10")
NOTE = "by dictionary code"


def values(count, width=9, salt=b""):
    """`count` distinct values of at most `width` bytes"""
    return np.array([salt + b"%x" % i for i in range(count)], dtype=f"S{width}")


def table(n, s_type, vals, seed=1, name="t"):
    """s: the coded column under test (every value occurs where the rows allow); u: a second coded column (CHAR(6), 5 values); f: a
    CHAR(1) column of 3 values; a: 0..999; k: the row number"""
    rng = np.random.default_rng(seed)
    vals = np.asarray(vals)
    s = vals[rng.integers(0, len(vals), n)] if n else vals[:0]
    if n >= len(vals):
        s[:len(vals)] = vals
    modes = np.array([b"MAIL", b"SHIP", b"AIR", b"RAIL", b"liamm"], dtype="S6")
    flags = np.array([b"A", b"N", b"R"], dtype="S1")
    return P.Table(name, [P.Column("s", s_type, s),
                          P.Column("u", T.CHAR(6), modes[rng.integers(0, 5, n)]),
                          P.Column("f", T.CHAR(1), flags[rng.integers(0, 3, n)]),
                          P.Column("a", T.BIGINT(), rng.integers(0, 1000, n).astype(np.int64)),
                          P.Column("k", T.BIGINT(), np.arange(n, dtype=np.int64))], n)


COUNT = "select s, count(*) from t group by s"
SUMS = "select s, sum(a), count(*) from t group by s"                     # no ORDER BY: the reference's emission order
MIXED = "select s, u, f, a, count(*) from t group by s, u, f, a"
TWO_CODED = "select s, u, count(*), sum(a), min(k), max(k) from t group by s, u"
HBM = "select s, a, count(*), sum(k) from t group by s, a"
HBM_TOP = "select s, a, count(*) as c, sum(k) as total from t group by s, a order by total desc, s, a limit 10"
LATE = "select s, sum(a), count(*) from t where k < 1500 group by s"

# over table(ROWS, CHAR(9) / VARCHAR(9), dictcases.edge_values(9, 12)): 'ab' against 'ab ', the empty value, full-width values, anagrams
STATEMENTS = {
    "no_order": SUMS,
    "order_asc_limit": "select s, sum(a) as total, count(*) from t group by s order by s limit 5",
    "order_desc_limit": "select s, sum(a) as total, count(*) from t group by s order by s desc limit 4",
    "entries_filtered_out": "select s, sum(a), count(*) from t where s like 'x%' or s = 'ab' group by s",
    "no_row_passes": "select s, sum(a), count(*) from t where a < 0 group by s",
    "key_in_case": "select s, case when s = 'ab' or s like 'xa%' then sum(a) else count(*) end from t group by s",
    "two_coded_and_numeric": "select s, u, a, count(*) from t where a < 3 group by s, u, a",
}

# r: a small build side keyed by a number; t probes it behind a selection (a wave compaction) and groups by ITS OWN coded column, or by
# r's coded payload ru (a join's build side: not dense, the hash form)
JOIN_OWN = "select s, sum(a), count(*) from t, r where a = ra and k < 4000 group by s"
JOIN_OWN_HBM = "select s, a, sum(k), count(*) from t, r where a = ra and k < 4000 group by s, a"       # 12 x 1000 groups: the HBM table
JOIN_PAYLOAD = "select ru, sum(a), count(*) from t, r where a = ra and k < 4000 group by ru"


def join_tables(kind="CHAR"):
    t = table(ROWS, getattr(T, kind)(9), D.edge_values(9, 12), seed=3)
    n = 600                                                               # r holds 600 of t's 1000 values of a
    modes = np.array([b"liamm", b"mmail", b"MAIL", b"AIR"], dtype="S6")
    r = P.Table("r", [P.Column("ra", T.BIGINT(), np.arange(n, dtype=np.int64) * 5 % 1000 + np.arange(n, dtype=np.int64) // 200),
                      P.Column("ru", T.CHAR(6), np.resize(modes, n))], n)
    return t, r


def warm_statements():
    """(sql, host tables, environment) of every statement tests/test_gpu_dict_group.py compiles with its own kernels, for the build's
    code-object warm-up (a compile-only context; each is compiled dense under its environment, and without it with RSQ_DICT_SCANS=0 and
    with RSQ_AGG_MODE=5, as the test's _check runs it)"""
    out = []
    for n, count in [(1, 1), (77, 2), (ROWS, 7), (ROWS, 64), (ROWS, 256), (ROWS, 257)]:
        out.append((SUMS, [table(n, T.VARCHAR(9), values(count))], {}))
    for kind, w in [("CHAR", 2), ("VARCHAR", 9), ("CHAR", 25), ("VARCHAR", 25)]:
        out.append((SUMS, [table(ROWS, getattr(T, kind)(w), D.edge_values(w))], {}))
    edge = {kind: table(ROWS, getattr(T, kind)(9), D.edge_values(9, 12), seed=2 + i) for i, kind in enumerate(("CHAR", "VARCHAR"))}
    for name, sql in STATEMENTS.items():
        out.append((sql, [edge["CHAR"]], {}))
    out.append((SUMS, [edge["VARCHAR"]], {}))
    for mode in "123":
        out.append((COUNT, [edge["CHAR"]], {"RSQ_AGG_MODE": mode}))
    hbm = table(ROWS, T.VARCHAR(9), values(256), seed=9)
    for env in ({}, {"RSQ_PARTITION": "0"}, {"RSQ_PARTITION": "2"}, {"RSQ_PARTITION": "2", "RSQ_STAGED": "0"}):
        out.append((HBM, [hbm], env))
    out.append((HBM_TOP, [hbm], {}))
    out.append((HBM_TOP, [hbm], {"RSQ_DEVICE_TOPK": "0"}))
    out.append((MIXED, [table(ROWS, T.CHAR(9), values(7), seed=5)], {}))
    out.append((LATE, [table(20_000, T.CHAR(9), D.edge_values(9, 12), seed=6)], {}))
    for kind in ("CHAR", "VARCHAR"):
        t, r = join_tables(kind)
        out.append((JOIN_OWN, [t, r], {}))
        out.append((JOIN_PAYLOAD, [t, r], {}))
        if kind == "CHAR":
            out.append((JOIN_OWN, [t, r], {"RSQ_AGG_MODE": "1"}))
            out.append((JOIN_OWN_HBM, [t, r], {}))
    out.append((TWO_CODED, [edge["CHAR"]], {"RSQ_CHECK_STATS": "1"}))
    out.append((SUMS, [table(3_000, T.VARCHAR(9), D.many_values(20), seed=4)], {}))
    out.append((SUMS, [table(ROWS, T.CHAR(9), D.edge_values(9, 12), seed=7)], {}))
    out.append((SUMS, [table(2_000, T.VARCHAR(9), D.edge_values(9, 12), seed=14)], {}))
    return out
