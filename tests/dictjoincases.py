"""Tables and statements of tests/test_dict_join_codegen.py and tests/test_gpu_dict_join.py: GROUP BY over a dictionary-coded string
that reaches the aggregation as a join's build-side payload (RSQ_DICT_SCANS=2).  The payload word holds an address inside the origin
column's dictionary image, so the group's dense rank is (address - dictionary) / width.  The probe side is dictgroupcases.table at
dictgroupcases.ROWS rows; build sides hold a few hundred rows."""
import numpy as np

from resql_amd import plan as P, tpch_full

import dictcases as D
import dictgroupcases as G

T = P.TypeInit
ROWS = G.ROWS
NOTE = G.NOTE
MODES = np.array([b"liamm", b"mmail", b"MAIL", b"AIR"], dtype="S6")       # (the anagrams collide in Values::hash: the emission order shows)

JOIN_PAYLOAD = G.JOIN_PAYLOAD
NO_ROW = "select ru, sum(a), count(*) from t, r where a = ra and a < 0 group by ru"
MIXED = "select ru, s, f, sum(a), count(*) from t, r where a = ra and k < 4000 group by ru, s, f"
HBM = "select ru, a, sum(k), count(*) from t, r where a = ra and k < 4000 group by ru, a"
TOP = "select ru, sum(a) as total, count(*) from t, r where a = ra and k < 4000 group by ru order by total desc, ru limit 3"
HBM_TOP = "select ru, a, count(*) as c, sum(k) as total from t, r where a = ra and k < 4000 group by ru, a order by total desc, ru, a limit 10"


def scattered_keys(n):
    """n distinct values of t's a (0..999), not in ascending order: the table is built (a rank dictionary, or the hash form)"""
    return np.arange(n, dtype=np.int64) * 5 % 1000 + np.arange(n, dtype=np.int64) // 200


def build_side(ru_type, vals, keys, name="r"):
    """r: ra the join key, ru the coded payload (every value occurs, in turn), rw a number"""
    keys = np.asarray(keys, dtype=np.int64)
    n = len(keys)
    return P.Table(name, [P.Column("ra", T.BIGINT(), keys), P.Column("ru", ru_type, np.resize(np.asarray(vals), n)),
                          P.Column("rw", T.BIGINT(), np.arange(n, dtype=np.int64) * 3 % 17)], n)


def probe_side(seed=3):
    return G.table(ROWS, T.CHAR(9), D.edge_values(9, 12), seed=seed)


def tables(ru_type=None, vals=MODES, keys=None):
    return probe_side(), build_side(ru_type or T.CHAR(6), vals, scattered_keys(600) if keys is None else keys)


def lonely_tables():
    """one build row's key is outside t's values, and its ru occurs nowhere else: an entry of the dictionary that no probe row reaches"""
    t, r = tables(keys=np.concatenate([scattered_keys(599), [5000]]))
    r.col("ru").data[599] = b"LONELY"
    return t, r


def two_hop_tables():
    """n: 25 names of CHAR(25); m: 300 rows, each with one of the 25; t probes m"""
    names = np.array([b"NAME %02d OF TWENTY-FIVE" % i if i % 2 else b"N%d" % i for i in range(25)], dtype="S25")
    n = P.Table("n", [P.Column("nk", T.BIGINT(), np.arange(25, dtype=np.int64)), P.Column("nname", T.CHAR(25), names)], 25)
    mk = scattered_keys(300)
    m = P.Table("m", [P.Column("mk", T.BIGINT(), mk), P.Column("mn", T.BIGINT(), (mk * 7 + 3) % 25)], 300)
    return probe_side(), m, n


def two_hop_plan(single=True):
    """m probes n's table and builds its own with the name as a payload; t probes that one: the address crosses two tables (SQL text would
    let t probe both tables itself)"""
    t, m, n = two_hop_tables()
    p = P.Plan([t, m, n])
    inner = p.hashjoin([p.eq(p.attr("nk"), p.attr("mn"))], p.scan("n"), p.scan("m"), single_match=single)
    j = p.hashjoin([p.eq(p.attr("mk"), p.attr("a"))], inner, p.selection(p.lt(p.attr("k"), p.constant(4000, P.BIGINT)), p.scan("t")), single_match=single)
    s, c = p.sum(p.attr("a")), p.count(p.star())
    node = p.aggregation([s, c], [p.attr("nname")], j)
    return p.set_root(p.materialize(p.projection([p.attr("nname"), p.as_("total", s), p.as_("c", c)], node)))


def warm_statements():
    """(sql or plan, host tables, environment) of every statement tests/test_gpu_dict_join.py compiles with its own kernels, for the build's
    code-object warm-up: each is compiled under RSQ_DICT_SCANS=2 with its environment, and under 1 and 0 without, as the test's _check
    runs it"""
    out = []
    for kind in ("CHAR", "VARCHAR"):
        out.append((JOIN_PAYLOAD, list(tables(getattr(T, kind)(6))), {}))
        out.append((JOIN_PAYLOAD, list(tables(getattr(T, kind)(9), D.edge_values(9, 12))), {}))
    direct = list(tables(keys=np.arange(600)))
    out.append((JOIN_PAYLOAD, direct, {}))
    out.append((JOIN_PAYLOAD, direct, {"RSQ_JOIN_RANK": "0"}))
    hops = two_hop_plan()
    out.append((hops, list(hops.tables), {}))
    db = tpch_full.database(0.01)
    for name in ("q5", "q10"):
        out.append((tpch_full.QUERIES[name], [db[k] for k in sorted(db)], {}))
    for count in (1, 2, 256, 257):
        out.append((JOIN_PAYLOAD, list(tables(T.VARCHAR(9), G.values(count))), {}))
    std = list(tables())
    for sql in (MIXED, HBM, NO_ROW, TOP, HBM_TOP):
        out.append((sql, std, {}))
    out.append((HBM, std, {"RSQ_DEVICE_TAIL_MIN": "1"}))
    out.append((HBM, list(tables(T.CHAR(9), D.edge_values(9, 12))), {"RSQ_DEVICE_TAIL_MIN": "1"}))
    for mode in "123":
        out.append((JOIN_PAYLOAD, std, {"RSQ_AGG_MODE": mode}))
    out.append((JOIN_PAYLOAD, list(lonely_tables()), {}))
    a, b = appended_tables()
    out.append((JOIN_PAYLOAD, [probe_side(), a], {}))
    out.append((JOIN_PAYLOAD, [probe_side(), concat(a, b)], {}))
    return out


def _grouped(p, child):
    s, c = p.sum(p.attr("a")), p.count(p.star())
    return s, c


def computed_key_plan():
    """the group key is a CASE over the build-side payload: a computed string, by value"""
    t, r = tables(T.VARCHAR(6))
    p = P.Plan([t, r])
    j = p.hashjoin([p.eq(p.attr("ra"), p.attr("a"))], p.scan("r"), p.selection(p.lt(p.attr("k"), p.constant(4000, P.BIGINT)), p.scan("t")))
    g = p.case(p.when_then(p.eq(p.attr("ru"), p.constant("MAIL", P.VARCHAR)), p.attr("ru")), p.constant("other", P.VARCHAR))
    s, c = _grouped(p, j)
    node = p.aggregation([s, c], [g], j)
    return p.set_root(p.materialize(node), request_all=True)


def derived_key_plan():
    """the build side is an aggregation over r (a derived table, strings by value): its ru has no dictionary"""
    t, r = tables()
    p = P.Plan([t, r])
    d = p.aggregation([p.count(p.star())], [p.attr("ru"), p.attr("ra")], p.scan("r"))
    j = p.hashjoin([p.eq(p.attr("ra"), p.attr("a"))], d, p.selection(p.lt(p.attr("k"), p.constant(4000, P.BIGINT)), p.scan("t")))
    s, c = _grouped(p, j)
    node = p.aggregation([s, c], [p.attr("ru")], j)
    return p.set_root(p.materialize(node), request_all=True)


def concat(a, b):
    return P.Table(a.name, [P.Column(x.name, x.type, np.concatenate([x.data, y.data])) for x, y in zip(a.columns, b.columns)], a.n_rows + b.n_rows)


def appended_tables():
    """r, and rows to append whose one new value of ru sorts in front of the old ones (every old rank moves); their keys are new ones"""
    a = build_side(T.CHAR(6), MODES, scattered_keys(400))
    b = build_side(T.CHAR(6), np.array([b"AAA"], dtype="S6"), scattered_keys(600)[400:])
    return a, b
