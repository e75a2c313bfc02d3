#!/usr/bin/env python3
"""Generate tests/golden/order_limit_reference.json: what the UNMODIFIED reference answers (its own JIT execution, one thread) for
ORDER BY ... LIMIT statements without an aggregation over the eight-table database (SF 0.01) - the shape Context.set_order_limit(1)
decides from device-selected candidates.  Every key list ends in the table's unique key, so no two rows tie and the answer does not
depend on the quicksort's path; the script checks that on the reference's own answer for LIMIT + 1 rows before it records anything.

Run where the reference is built (oracle/_ref/ref_harness):  python tests/golden/make_order_limit_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from resql_amd import engine, tpch_full  # noqa: E402
from oracle import orc  # noqa: E402

SF = 0.01
# (statement with its LIMIT left open, the limit, the leading select-list columns that are the table's unique key)
STATEMENTS = [
    ("select l_orderkey, l_linenumber, l_extendedprice from lineitem order by l_extendedprice desc, l_orderkey, l_linenumber limit %d", 10, 2),
    ("select l_orderkey, l_linenumber, l_extendedprice, l_shipdate from lineitem where l_shipdate < date '1994-01-01' "
     "order by l_extendedprice desc, l_orderkey, l_linenumber limit %d", 10, 2),
    ("select l_orderkey, l_linenumber, l_shipdate, l_shipmode from lineitem order by l_shipdate, l_orderkey, l_linenumber limit %d", 20, 2),
    ("select l_orderkey, l_linenumber, l_quantity, l_comment from lineitem order by l_quantity desc, l_orderkey desc, l_linenumber limit %d", 7, 2),
    ("select o_orderkey, o_totalprice, o_orderdate from orders order by o_totalprice, o_orderkey limit %d", 100, 1),
    ("select o_orderkey, o_custkey, o_comment from orders where o_orderdate < date '1995-01-01' order by o_custkey desc, o_orderkey limit %d", 5, 1),
    ("select l_orderkey, l_linenumber, l_extendedprice * (1 - l_discount) as revenue from lineitem order by revenue desc, l_orderkey, l_linenumber limit %d", 10, 2),
    ("select l_orderkey, l_linenumber, l_partkey from lineitem order by l_partkey, l_orderkey, l_linenumber limit %d", 1, 2),
]


def rows_of(text):
    return [line.split("|") for line in text.splitlines() if line and not line.startswith("#")]


def main():
    ctx = engine.Context(device=-1)
    db = tpch_full.database(SF)
    host = [db[k] for k in sorted(db)]
    out = {"sf": SF, "tables": sorted(db), "cases": []}
    for sql, limit, key_cols in STATEMENTS:
        # the leading limit + 1 rows of the reference's own answer: distinct unique keys, so none of them ties with another on the whole key list
        more = rows_of(orc.run_reference_sql(host, ctx.sql_describe(sql % (limit + 1), 0), threads=1))
        keys = [tuple(r[:key_cols]) for r in more]
        assert len(more) == limit + 1 and len(set(keys)) == len(keys), (sql, len(more))
        result = orc.run_reference_sql(host, ctx.sql_describe(sql % limit, 0), threads=1)
        assert rows_of(result) == more[:limit], sql
        out["cases"].append({"sql": sql % limit, "limit": limit, "result": result})
        print(sql % limit, "-> %d bytes" % len(result), file=sys.stderr)
    ctx.close()
    with open(os.path.join(HERE, "order_limit_reference.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
