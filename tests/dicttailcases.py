"""Tables and statements of tests/test_gpu_dict_tail.py: dense aggregations keyed by dictionary-coded string columns (RSQ_DICT_SCANS=1)
whose tail runs on the device (resql_amd/csrc/devtail.hip).  Small inputs: about 5 000 rows for the statements with a handful of groups,
20 000 where more than 4 096 groups have to come back, dictionaries of 1 to 256 entries, the edge values of tests/dictcases.py.

A handful of groups and cells would be a register-mode table, which no device tail reads (its cells are padded): those statements are
compiled with RSQ_AGG_MODE=3, the workgroup's LDS table, and RSQ_DEVICE_TAIL_MIN=1 lets the device tail take them."""
import numpy as np

from resql_amd import plan as P

import dictcases as D
import dictgroupcases as G

T = P.TypeInit

ROWS = G.ROWS                                                             # forty tiles and a tail
MANY = 20_000
FEW = {"RSQ_AGG_MODE": "3"}                                               # (compile-time part of a few-groups statement's environment)

SUMS = G.SUMS
ALL_AGGS = "select s, sum(a), min(k), max(k), avg(a), count(*) from t group by s"
ALL_AGGS_BY_A = "select s, a, sum(k), min(k), max(k), avg(k), count(*) from t group by s, a"
HBM = G.HBM                                                               # group by s, a
KEY_ORDER = "select a, u, count(*), f, sum(k), s from t group by s, f, u, a"
NO_ROW = "select s, sum(a), count(*) from t where a < 0 group by s"
ORDERED = "select s, a, count(*) from t group by s, a order by s, a"
COMPUTED = "select s, case when s = 'ab' then sum(a) else count(*) end from t group by s"
TOP = G.HBM_TOP

# (kind, width, values) of the few-groups statement: the 12 edge values, dictionaries of 1, 2 and 256 entries, widths 2 and 25
FEW_GROUPS = {
    "char9_edge": ("CHAR", 9, D.edge_values(9, 12)),
    "varchar9_edge": ("VARCHAR", 9, D.edge_values(9, 12)),
    "one_entry": ("VARCHAR", 9, G.values(1)),
    "two_entries": ("CHAR", 9, G.values(2)),
    "256_entries": ("VARCHAR", 9, G.values(256)),
    "char2": ("CHAR", 2, D.edge_values(2)),
    "char25": ("CHAR", 25, D.edge_values(25)),
    "varchar25": ("VARCHAR", 25, D.edge_values(25)),
}


def merges(kind, vals):
    """two of the values are one value to CHAR (equal up to trailing spaces): the device merges their groups"""
    stripped = [bytes(v).rstrip(b" ") for v in vals]
    return kind == "CHAR" and len(set(stripped)) < len(stripped)


def few_groups_table(name):
    kind, w, vals = FEW_GROUPS[name]
    return G.table(ROWS, getattr(T, kind)(w), vals, seed=21)


def spelling_table(first, n=ROWS):
    """CHAR(9) 'ab' and 'ab ' (one group) and 'x': row 0 holds `first`, the other spelling comes later"""
    vals = np.array([b"ab", b"ab ", b"x"], dtype="S9")
    t = G.table(n, T.CHAR(9), vals, seed=22)
    s = t.columns[0].data
    other = b"ab" if first == b"ab " else b"ab "
    s[:3] = [first, b"x", other]
    return t


def class_of_three_table(n=MANY):
    """'x', 'x ' and 'x  ' are one value, every spelling in thousands of rows: with a as second key, up to three groups of every
    a fold into one at the same time"""
    return G.table(n, T.CHAR(9), np.array([b"x  ", b"x", b"y", b"x "], dtype="S9"), seed=23)


def replay_table(kind="CHAR"):
    return G.table(MANY, getattr(T, kind)(9), D.edge_values(9, 12), seed=24)


def key_order_table(n=MANY):
    """s and u coded CHAR columns that both hold values equal up to trailing spaces, f a CHAR(1) byte set, a numeric"""
    t = G.table(n, T.CHAR(9), D.edge_values(9, 12), seed=25)
    rng = np.random.default_rng(26)
    modes = np.array([b"MAIL", b"MAIL ", b"AIR", b"AIR  ", b"liamm"], dtype="S6")
    t.columns[1] = P.Column("u", T.CHAR(6), modes[rng.integers(0, 5, n)])
    return t


def by_itself_table():
    return G.table(ROWS, T.CHAR(9), G.values(256), seed=27)              # 256 entries x a's 1000 values: 256 000 cells per accumulator


def top_table():
    """256 entries, 'ab' and 'ab ' among them: the candidate pre-selection is refused, the host merges"""
    vals = np.concatenate([D.edge_values(9, 12), G.values(244, 9, b"v")])
    assert len(set(vals.tolist())) == 256
    return G.table(ROWS, T.CHAR(9), vals, seed=28)


def having_plan(t):
    """a HAVING-style statement (tests/derivedcases.py having_*): the aggregation by (s, a) is a sub-query, the selection reads its groups"""
    p = P.Plan([t])
    c = p.count(p.star())
    a = p.aggregation([c, p.sum(p.attr("k"))], [p.attr("s"), p.attr("a")], p.scan("t"))
    return p.set_root(p.materialize(p.selection(p.gt(c, p.constant(1, P.BIGINT)), a)), request_all=True)


def warm_statements():
    """(statement - SQL text or a plan -, host tables, environment) of every statement tests/test_gpu_dict_tail.py compiles, for the build's
    code-object warm-up (a compile-only context under RSQ_DICT_SCANS=1)"""
    out = []
    for name in FEW_GROUPS:
        out.append((SUMS, [few_groups_table(name)], FEW))
    for first in (b"ab ", b"ab"):
        out.append((ALL_AGGS, [spelling_table(first)], FEW))
    out.append((ALL_AGGS_BY_A, [class_of_three_table()], {}))
    for limit in ("", " limit 1", " limit 1234"):
        out.append((HBM + limit, [replay_table()], {}))
    out.append((KEY_ORDER, [key_order_table()], {}))
    out.append((NO_ROW, [few_groups_table("char9_edge")], FEW))
    out.append((SUMS, [G.table(1, T.CHAR(9), np.array([b"ab "], dtype="S9"), seed=29)], FEW))
    out.append((HBM, [by_itself_table()], {}))
    out.append((ORDERED, [replay_table()], {}))
    out.append((COMPUTED, [few_groups_table("char9_edge")], FEW))
    out.append((TOP, [top_table()], {}))
    out.append((having_plan(replay_table()), None, {}))
    return out
