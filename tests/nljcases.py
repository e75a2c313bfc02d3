"""Statements whose FROM lists are not all linked by equalities: the reference's planner joins the leftover pieces with
nested-loops joins (planner.h:458-469).  tests/golden/make_nlj_golden.py records what the reference does with each."""

STATEMENTS = [
    # cross products, with and without WHERE
    "select r_name, n_name from region, nation",
    "select count(*) from region, nation",
    "select * from region, nation where r_regionkey = 1 and n_nationkey < 3",
    "select r_name, n_name from region, nation where r_regionkey < 2",
    "select n_name, r_name from nation, region where n_nationkey < 4 and r_regionkey > 2",
    # inequalities across the sides: BIGINT, DECIMAL, DATE; INT vs INT (the reference has no `<` between two INT columns)
    "select r_name, count(*) from supplier, region where s_nationkey < r_regionkey * 5 group by r_name",
    "select count(*) from nation, region where n_regionkey < r_regionkey",
    "select s_name, n_name from supplier, nation where s_acctbal < n_nationkey * 100 and s_suppkey < 20 and n_nationkey < 5",
    "select count(*), sum(s_acctbal) from supplier, region where s_acctbal > r_regionkey * 2000.00",
    "select c_name, o_orderkey from customer, orders where c_custkey < 3 and o_orderkey < 40 and o_totalprice < c_acctbal * 10",
    "select count(*) from nation, region, supplier where n_regionkey < r_regionkey and s_suppkey < 3 and n_nationkey < 2",
    # aggregates with and without GROUP BY
    "select min(s_acctbal), max(s_acctbal), sum(s_acctbal), count(*) from supplier, region where r_regionkey < 3",
    "select n_name, count(*), sum(r_regionkey * 1) from nation, region where n_nationkey < 6 group by n_name",
    "select r_name, min(s_acctbal), max(s_acctbal) from region, supplier where s_suppkey < 50 group by r_name",
    "select r_regionkey, n_regionkey, count(*) from region, nation group by r_regionkey, n_regionkey",
    # ORDER BY ... LIMIT, and LIMIT without ORDER BY
    "select n_name, r_name from nation, region where n_nationkey < 8 order by n_name, r_name limit 7",
    "select s_name, r_name from supplier, region where s_suppkey < 30 limit 11",
    "select r_name, n_name, n_nationkey from region, nation order by n_nationkey desc, r_name limit 5",
    # CHAR and VARCHAR columns from both sides
    "select n_name, r_comment from nation, region where n_nationkey < 3 and r_regionkey < 2",
    "select s_address, r_name, s_phone from supplier, region where s_suppkey < 4",
    "select count(*) from nation, region where n_name = 'GERMANY' and r_name = 'EUROPE'",
    "select * from nation, region where n_nationkey = 7",
    # a hash-join piece as one side
    "select n_name, r_name, s_name from supplier, nation, region where s_nationkey = n_nationkey and s_suppkey < 10 and r_regionkey < 2",
    "select r_name, count(*) from region, nation, supplier where n_nationkey = s_nationkey group by r_name",
    # three pieces
    "select count(*) from region, nation, supplier where r_regionkey < 2 and n_nationkey < 3 and s_suppkey < 5",
    "select r_name, n_name, s_name from region, nation, supplier where r_regionkey = 0 and n_nationkey < 2 and s_suppkey < 3",
    # an empty inner side and an empty outer side
    "select r_name, n_name from region, nation where r_regionkey > 10",
    "select r_name, n_name from region, nation where n_nationkey > 100",
    "select count(*) from region, nation where n_nationkey > 100",
    # a condition that spans both sides and a constant
    "select count(*) from part, region where p_size < r_regionkey * 3 and p_partkey < 200",
]
