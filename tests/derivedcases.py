"""Plans with derived aggregations: an AGGREGATION below a selection, a join or another aggregation (the reference's
AggregationOp::consumeAggregateFlounder hands its groups to whatever parent it has).  Builders over tpch_full.database(sf);
each returns a resql_amd.plan.Plan."""
from resql_amd import plan as P

TABLES = ("customer", "lineitem", "nation", "orders", "part", "region", "supplier")


def _plan(db):
    return P.Plan([db[k] for k in TABLES])


def having_hash_key(db, threshold=250):
    p = _plan(db)
    q = p.sum(p.attr("l_quantity"))
    a = p.aggregation([q], [p.attr("l_orderkey")], p.scan("lineitem"))
    return p.set_root(p.materialize(p.selection(p.gt(q, p.constant(threshold, P.DECIMAL)), a)), request_all=True)


def having_dense_key(db):
    p = _plan(db)
    c = p.count(p.star())
    a = p.aggregation([c], [p.attr("o_custkey")], p.scan("orders"))
    return p.set_root(p.materialize(p.selection(p.gt(c, p.constant(18, P.BIGINT)), a)), request_all=True)


def having_char_key(db):
    p = _plan(db)
    s = p.sum(p.attr("l_extendedprice"))
    a = p.aggregation([s, p.count(p.star())], [p.attr("l_returnflag"), p.attr("l_linestatus")], p.scan("lineitem"))
    return p.set_root(p.materialize(p.selection(p.gt(s, p.constant("20000000.00", P.DECIMAL)), a)), request_all=True)


def having_ungrouped(db):
    p = _plan(db)
    s = p.sum(p.attr("l_quantity"))
    a = p.aggregation([s, p.count(p.star())], [], p.scan("lineitem"))
    return p.set_root(p.materialize(p.selection(p.gt(s, p.constant(1000, P.DECIMAL)), a)), request_all=True)


def having_avg(db):
    p = _plan(db)
    v = p.avg(p.attr("l_quantity"))
    a = p.aggregation([v, p.count(p.star())], [p.attr("l_suppkey")], p.scan("lineitem"))
    return p.set_root(p.materialize(p.selection(p.gt(v, p.constant("26.50", P.DECIMAL)), a)), request_all=True)


def build_side(db):
    p = _plan(db)
    c = p.count(p.star())
    a = p.aggregation([c], [p.attr("o_custkey")], p.scan("orders"))
    j = p.hashjoin([p.eq(p.attr("o_custkey"), p.attr("c_custkey"))], a, p.scan("customer"))
    return p.set_root(p.materialize(p.projection([p.attr("c_name"), c], j)), request_all=True)


def build_side_multi(db):
    p = _plan(db)
    c = p.count(p.star())
    a = p.aggregation([c], [p.attr("o_custkey")], p.scan("orders"))
    j = p.hashjoin([p.eq(p.attr("o_custkey"), p.attr("c_custkey"))], a, p.scan("customer"))
    out = p.aggregation([p.sum(c), p.count(p.star())], [p.attr("c_nationkey")], j)
    return p.set_root(p.materialize(out), request_all=True)


def probe_side(db):
    p = _plan(db)
    s = p.sum(p.attr("l_quantity"))
    a = p.aggregation([s], [p.attr("l_orderkey")], p.scan("lineitem"))
    j = p.hashjoin([p.eq(p.attr("o_orderkey"), p.attr("l_orderkey"))], p.scan("orders"), a)
    return p.set_root(p.materialize(p.projection([p.attr("o_orderkey"), p.attr("o_orderdate"), s], j)), request_all=True)


def join_on_aggregate(db):
    p = _plan(db)
    c = p.count(p.star())
    a = p.aggregation([c], [p.attr("s_nationkey")], p.scan("supplier"))
    j = p.hashjoin([p.eq(p.attr("r_regionkey"), c)], p.scan("region"), a)
    return p.set_root(p.materialize(p.projection([p.attr("r_name"), p.attr("s_nationkey")], j)), request_all=True)


def projection_as(db):
    p = _plan(db)
    c = p.count(p.star())
    a = p.aggregation([c], [p.attr("s_nationkey")], p.scan("supplier"))
    pr = p.projection([p.as_("nk", p.attr("s_nationkey")), p.as_("nsupp", c)], a)
    j = p.hashjoin([p.eq(p.attr("nk"), p.attr("n_nationkey"))], pr, p.scan("nation"))
    return p.set_root(p.materialize(p.projection([p.attr("n_name"), p.attr("nsupp")], j)), request_all=True)


def agg_over_agg(db):
    p = _plan(db)
    c = p.count(p.star())
    a1 = p.aggregation([c], [p.attr("l_orderkey")], p.scan("lineitem"))
    return p.set_root(p.materialize(p.aggregation([p.count(p.star())], [c], a1)), request_all=True)


def agg_three_deep(db):
    p = _plan(db)
    c = p.count(p.star())
    a1 = p.aggregation([c], [p.attr("o_custkey")], p.scan("orders"))
    c2 = p.count(p.star())
    a2 = p.aggregation([c2], [c], a1)
    return p.set_root(p.materialize(p.aggregation([p.sum(c2), p.count(p.star())], [], a2)), request_all=True)


def agg_over_string_key(db):
    p = _plan(db)
    c = p.count(p.star())
    a1 = p.aggregation([c, p.sum(p.attr("c_acctbal"))], [p.attr("c_mktsegment"), p.attr("c_nationkey")], p.scan("customer"))
    return p.set_root(p.materialize(p.aggregation([p.max(c), p.count(p.star())], [p.attr("c_mktsegment")], a1)), request_all=True)


def two_derived_sides(db):
    p = _plan(db)
    c1 = p.count(p.star())
    a1 = p.aggregation([c1], [p.attr("s_nationkey")], p.scan("supplier"))
    c2 = p.count(p.star())
    a2 = p.aggregation([c2], [p.attr("c_nationkey")], p.scan("customer"))
    j = p.hashjoin([p.eq(p.attr("s_nationkey"), p.attr("c_nationkey"))], a1, a2)
    return p.set_root(p.materialize(p.projection([p.attr("c_nationkey"), c1, c2], j)), request_all=True)


def orderby_limit(db):
    p = _plan(db)
    s = p.sum(p.attr("l_extendedprice"))
    a = p.aggregation([s], [p.attr("l_partkey")], p.scan("lineitem"))
    j = p.hashjoin([p.eq(p.attr("l_partkey"), p.attr("p_partkey"))], a, p.scan("part"), single_match=True)
    pr = p.projection([p.attr("p_name"), p.as_("revenue", s)], j)
    return p.set_root(p.orderby([p.desc(p.attr("revenue")), p.attr("p_name")], pr), limit=10, request_all=True)


def materialize_limit(db):
    p = _plan(db)
    c = p.count(p.star())
    a = p.aggregation([c], [p.attr("l_orderkey")], p.scan("lineitem"))
    return p.set_root(p.materialize(p.selection(p.gt(c, p.constant(5, P.BIGINT)), a)), limit=7, request_all=True)


def empty_grouped(db):
    p = _plan(db)
    c = p.count(p.star())
    a = p.aggregation([c], [p.attr("l_suppkey")], p.selection(p.gt(p.attr("l_quantity"), p.constant(100, P.DECIMAL)), p.scan("lineitem")))
    j = p.hashjoin([p.eq(p.attr("l_suppkey"), p.attr("s_suppkey"))], a, p.scan("supplier"))
    return p.set_root(p.materialize(p.projection([p.attr("s_name"), c], j)), request_all=True)


def empty_ungrouped(db):
    p = _plan(db)
    c = p.count(p.star())
    a = p.aggregation([c, p.sum(p.attr("l_quantity"))], [], p.selection(p.gt(p.attr("l_quantity"), p.constant(100, P.DECIMAL)), p.scan("lineitem")))
    return p.set_root(p.materialize(p.aggregation([p.count(p.star())], [c], a)), request_all=True)


def string_key_join(db):
    p = _plan(db)
    c = p.count(p.star())
    a = p.aggregation([c], [p.attr("n_name")], p.scan("nation"))
    pr = p.projection([p.as_("nm", p.attr("n_name")), c], a)
    n2 = p.projection([p.attr("n_name"), p.attr("n_nationkey")], p.scan("nation"))
    j = p.hashjoin([p.eq(p.attr("nm"), p.attr("n_name"))], pr, n2)
    return p.set_root(p.materialize(p.projection([p.attr("nm"), p.attr("n_nationkey"), c], j)), request_all=True)


def q18(db, threshold=250):
    p = _plan(db)
    q = p.sum(p.attr("l_quantity"))
    big = p.projection([p.as_("big_orderkey", p.attr("l_orderkey"))],
                       p.selection(p.gt(q, p.constant(threshold, P.DECIMAL)), p.aggregation([q], [p.attr("l_orderkey")], p.scan("lineitem"))))
    j1 = p.hashjoin([p.eq(p.attr("big_orderkey"), p.attr("o_orderkey"))], big, p.scan("orders"))
    j2 = p.hashjoin([p.eq(p.attr("c_custkey"), p.attr("o_custkey"))], p.scan("customer"), j1)
    j3 = p.hashjoin([p.eq(p.attr("o_orderkey"), p.attr("l_orderkey"))], j2, p.scan("lineitem"))
    tot = p.sum(p.attr("l_quantity"))
    keys = ("c_name", "c_custkey", "o_orderkey", "o_orderdate")
    out = p.aggregation([tot], [p.attr(c) for c in keys], j3)
    proj = p.projection([p.attr(c) for c in keys] + [p.as_("sum_qty", tot)], out)
    return p.set_root(p.orderby([p.desc(p.attr("sum_qty")), p.attr("o_orderdate"), p.attr("o_orderkey")], proj), limit=100, request_all=True)


# ---- two small literal tables: CHAR(1) and VARCHAR group keys with trailing spaces, repeated values, an empty selection ----
def _literal_tables():
    T = P.TypeInit
    emp = P.table_from_strings("emp", [("e_id", T.BIGINT()), ("e_dept", T.CHAR(1)), ("e_city", T.VARCHAR(10)), ("e_pay", T.DECIMAL(10, 2))], [
        ["1", "a", "Bonn", "10.50"], ["2", "b", "Kiel", "20.00"], ["3", "a", "Bonn ", "30.25"], ["4", "c", "Ulm", "5.00"],
        ["5", "b", "Kiel", "7.75"], ["6", "a", "Ulm", "12.00"], ["7", "d", "Essen", "99.99"], ["8", "c", "Bonn", "1.00"],
        ["9", "b", "Ulm", "40.00"], ["10", "a", "Kiel", "3.50"], ["11", "e", "Essen", "0.01"], ["12", "b", "Bonn", "16.00"]])
    dept = P.table_from_strings("dept", [("d_dept", T.CHAR(1)), ("d_name", T.CHAR(8))], [
        ["a", "alpha"], ["b", "beta"], ["c", "gamma"], ["d", "delta"], ["f", "phi"]])
    return P.Plan([emp, dept])


def lit_having_char1_avg(db):
    p = _literal_tables()
    v = p.avg(p.attr("e_pay"))
    a = p.aggregation([v, p.count(p.star())], [p.attr("e_dept")], p.scan("emp"))
    return p.set_root(p.materialize(p.selection(p.gt(v, p.constant("12.00", P.DECIMAL)), a)), request_all=True)


def lit_join_char1_key(db):
    p = _literal_tables()
    s = p.sum(p.attr("e_pay"))
    a = p.aggregation([s], [p.attr("e_dept")], p.scan("emp"))
    j = p.hashjoin([p.eq(p.attr("e_dept"), p.attr("d_dept"))], a, p.scan("dept"))
    return p.set_root(p.materialize(p.projection([p.attr("d_name"), s], j)), request_all=True)


def lit_varchar_agg_over_agg(db):
    p = _literal_tables()
    c = p.count(p.star())
    a = p.aggregation([c, p.min(p.attr("e_pay"))], [p.attr("e_city")], p.scan("emp"))
    return p.set_root(p.materialize(p.aggregation([p.count(p.star())], [c], a)), request_all=True)


def lit_empty_join(db):
    p = _literal_tables()
    c = p.count(p.star())
    a = p.aggregation([c], [p.attr("e_dept")], p.selection(p.gt(p.attr("e_pay"), p.constant("1000.00", P.DECIMAL)), p.scan("emp")))
    j = p.hashjoin([p.eq(p.attr("e_dept"), p.attr("d_dept"))], a, p.scan("dept"))
    return p.set_root(p.materialize(p.projection([p.attr("d_name"), c], j)), request_all=True)


def lit_ungrouped_over_grouped(db):
    p = _literal_tables()
    s = p.sum(p.attr("e_pay"))
    c = p.count(p.star())
    a = p.aggregation([s, c], [p.attr("e_dept"), p.attr("e_city")], p.scan("emp"))
    return p.set_root(p.materialize(p.aggregation([p.sum(s), p.max(c), p.count(p.star())], [], a)), request_all=True)


LITERAL = {"lit_having_char1_avg", "lit_join_char1_key", "lit_varchar_agg_over_agg", "lit_empty_join", "lit_ungrouped_over_grouped"}


# plans the reference refuses: (builder, engine status); the words are the reference's (tests/golden/derived_agg_reference.json)
def refused_avg_int(db):
    p = _plan(db)
    a1 = p.aggregation([p.avg(p.attr("o_totalprice"))], [p.attr("o_custkey")], p.scan("orders"))
    return p.set_root(p.materialize(p.aggregation([p.max(p.attr("o_custkey")), p.count(p.star())], [], a1)), request_all=True)


def refused_min_int(db):
    p = _plan(db)
    a1 = p.aggregation([p.count(p.star())], [p.attr("c_nationkey")], p.scan("customer"))
    return p.set_root(p.materialize(p.aggregation([p.min(p.attr("c_nationkey"))], [], a1)), request_all=True)


CASES = [having_hash_key, having_dense_key, having_char_key, having_ungrouped, having_avg, build_side, build_side_multi, probe_side,
         join_on_aggregate, projection_as, agg_over_agg, agg_three_deep, agg_over_string_key, two_derived_sides, orderby_limit,
         materialize_limit, empty_grouped, empty_ungrouped, string_key_join, q18,
         lit_having_char1_avg, lit_join_char1_key, lit_varchar_agg_over_agg, lit_empty_join, lit_ungrouped_over_grouped]

REFUSED = [(refused_avg_int, 2), (refused_min_int, 2)]
