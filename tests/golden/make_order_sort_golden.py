#!/usr/bin/env python3
"""Generate tests/golden/order_sort_reference.json: what the UNMODIFIED reference answers (its own JIT execution, one thread) for ORDER BY
statements without an aggregation over the eight-table database (SF 0.01) - the shape Context.set_order_sort(1) sorts on the device: no
LIMIT, a LIMIT, a LIMIT above the rows, a filter, a projected key (the statements are tests/ordersortcases.py GOLD_STATEMENTS).  Every
key list ends in the table's unique key, so no two rows tie and the answer does not depend on the quicksort's path; the script checks
that on the reference's own answer before it records anything.  No key list begins with the key the table is generated in the order
of.  Data only: the statements and the reference's text - in full where it is short; a sorted relation of 60 000 rows is a megabyte of
text, so the long ones are recorded as their row count, their SHA-1 and their first and last 20 lines (tests/ordersortcases.py
gold_matches compares an answer with either form).

Run where the reference is built (oracle/_ref/ref_harness):  python tests/golden/make_order_sort_golden.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from resql_amd import engine, tpch_full  # noqa: E402
from oracle import orc  # noqa: E402
import ordersortcases as S  # noqa: E402


def rows_of(text):
    return [line.split("|") for line in text.splitlines() if line and not line.startswith("#")]


def main():
    ctx = engine.Context(device=-1)
    db = tpch_full.database(S.GOLD_SF)
    host = [db[k] for k in sorted(db)]
    out = {"sf": S.GOLD_SF, "tables": sorted(db), "cases": []}
    for sql in S.GOLD_STATEMENTS:
        result = orc.run_reference_sql(host, ctx.sql_describe(sql, 0), threads=1)
        rows = rows_of(result)
        key_cols = 2 if " from lineitem" in sql else 1          # (the select list begins with the table's unique key)
        keys = [tuple(r[:key_cols]) for r in rows]
        assert rows and len(set(keys)) == len(keys), (sql, len(rows))
        lines = result.splitlines(keepends=True)
        out["cases"].append({"sql": sql, "rows": len(rows), "sha1": hashlib.sha1(result.encode()).hexdigest(), "head": "".join(lines[:20]),
                             "tail": "".join(lines[-20:]), "result": result if len(result) <= S.GOLD_FULL_TEXT_BYTES else None})
        print(sql, "-> %d rows, %d bytes" % (len(rows), len(result)), file=sys.stderr)
    ctx.close()
    with open(os.path.join(HERE, "order_sort_reference.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
