"""Tables and statements of tests/test_gpu_dict_scan.py (dictionary-coded string columns): small inputs with the edge cases of the
values - 'ab' against 'ab ' in CHAR, empty VARCHAR values, values of the full declared length, anagram pairs - at the widths where
the words, 16-byte chunks and staged tiles of the wide string scans end."""
import numpy as np

from resql_amd import plan as P

T = P.TypeInit

ROW_COUNTS = [0, 1, 77, 128 * 40 + 33, 100_000]
WIDTHS = [2, 8, 9, 16, 25, 33, 44]
DICT_SIZES = [1, 2, 64, 65, 256, 257]


def edge_values(width, count=12):
    """`count` distinct values of at most `width` bytes: 'ab' and 'ab ' (where they fit), the empty value, one of the full width,
    anagram pairs"""
    full = (b"abcdefghijklmnopqrstuvwxyz" * 2)[:width]
    vals = [b"ab", b"", full, full[::-1]] + ([b"ab "] if width >= 3 else [])
    vals += [b"x" + bytes([97 + i % 26]) * min(width - 1, 1 + i % 3) for i in range(26)] if width >= 3 else [b"a", b"b", b"ba", b"xa", b"ax"]
    out = []
    for v in vals:
        if v[:width] not in out:
            out.append(v[:width])
    return np.array(out[:count], dtype=f"S{width}")


def table(n, s_type, values, seed=1, name="t", prefix=""):
    """s: the string column under test; u: a second coded column (CHAR(6), 5 values); a: 0..999; k: a row number"""
    rng = np.random.default_rng(seed)
    values = np.asarray(values)
    s = values[rng.integers(0, len(values), n)] if n else values[:0]
    if n >= len(values):
        s[:len(values)] = values                                          # every value occurs
    modes = np.array([b"MAIL", b"SHIP", b"AIR", b"RAIL", b"liamm"], dtype="S6")
    return P.Table(name, [P.Column(prefix + "s", s_type, s),
                          P.Column(prefix + "u", T.CHAR(6), modes[rng.integers(0, 5, n)]),
                          P.Column(prefix + "a", T.BIGINT(), rng.integers(0, 1000, n).astype(np.int64)),
                          P.Column(prefix + "k", T.BIGINT(), np.arange(n, dtype=np.int64))], n)


def many_values(count, width=9):
    return np.array([b"v%dx" % i if i % 3 else b"x%d" % i for i in range(count)], dtype=f"S{width}")


# statements over table(): name -> sql
GROUP_SUM = "select s, sum(a), count(*) from t where s <> 'xa' group by s"
WIDTH_SQL = "select s, count(*), sum(a) from t where s = '{full}' or s like 'x%' or s in ('ab', 'ba', '') group by s"
SIZE_SQL = "select s, sum(a) from t where s like '%x' or s like '%1%' or s = 'v1x' group by s"

PREDICATES = {
    "eq": "select sum(a), count(*) from t where s = 'ab'",
    "neq": "select sum(a), count(*) from t where s <> 'ab'",
    "in": "select sum(a), count(*) from t where s in ('ab', 'xaa', 'nothing', '')",
    "like_head": "select sum(a), count(*) from t where s like 'x%'",
    "like_tail": "select sum(a), count(*) from t where s like '%b'",
    "like_inside": "select sum(a), count(*) from t where s like '%cc%'",
    "or_of_two_columns": "select sum(a), count(*) from t where s = 'ab' or u = 'MAIL'",
    "and_of_two_columns": "select sum(a), count(*) from t where s like 'x%' and u in ('MAIL', 'SHIP')",
    "case": "select u, sum(case when s = 'ab' or s like 'xc%' then a else 0 end), sum(case when s <> 'ab' then 1 else 0 end) from t group by u",
    "late_loads": "select sum(a), sum(k), count(*) from t where k < 1500 and s like 'x%'",
}

SINKS = {
    "group_by": "select s, u, sum(a), count(*) from t group by s, u",
    "order_by_limit": "select s, sum(a) as total from t group by s order by total desc, s limit 5",
    "materialize": "select k, s, u from t where s like 'xb%' and a < 100",
}

# r: a second table whose string column rs holds every other value of t's s ('ab' and 'ab ', anagram pairs among them), joined on the
# coded columns; r's coded column ru is the payload that is materialised / grouped by behind the join
JOIN_SQL = "select k, ru, rs from t, r where s = rs and a < 300"
JOIN_GROUP_SQL = "select ru, sum(a), count(*) from t, r where s = rs group by ru"


def join_tables(kind="VARCHAR", n=20_000):
    vals = edge_values(9, 30)
    assert b"ab" in vals[::2] and b"ab " in vals[::2]
    t = table(n, getattr(T, kind)(9), vals)
    pick = vals[::2]
    modes = np.array([b"liamm", b"mmail", b"MAIL", b"AIR"], dtype="S6")
    r = P.Table("r", [P.Column("rs", getattr(T, kind)(9), pick), P.Column("ru", T.CHAR(6), np.resize(modes, len(pick)))], len(pick))
    return t, r
