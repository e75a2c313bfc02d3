#!/usr/bin/env python3
"""Generate tests/golden/result_pack_reference.json: what the UNMODIFIED reference answers (its own JIT execution, one thread) for plain
SELECTs without an aggregation - the shape whose result tuples Context.set_result_pack(1) packs on the device - over the seeded tables
of tests/resultpackcases.py (gold_table, dim_table; the statements are its GOLD_STATEMENTS): every column type, a filter, ORDER BY on a unique key without a LIMIT, ORDER BY
with a LIMIT, the materialisation's own LIMIT, a hash join feeding the materialisation.  Every ORDER BY ends in the unique key, so no
two rows tie and the answer does not depend on the quicksort's path.  Data only: the statements and the reference's text.

Run where the reference is built (oracle/_ref/ref_harness):  python tests/golden/make_result_pack_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from resql_amd import engine  # noqa: E402
from oracle import orc  # noqa: E402
import resultpackcases as R  # noqa: E402

COVERS = ["every column type", "a filter", "order by a unique key, no limit", "order by with a limit", "the materialisation's own limit",
          "a hash join feeds the materialisation"]


def main():
    ctx = engine.Context(device=-1)
    names = sorted(R.GOLD_TABLES)
    host = [R.GOLD_TABLES[k]() for k in names]
    out = {"tables": names, "cases": []}
    f = host[names.index("gold")].col("f").data
    expect = [len(f), int((f < 90).sum()), len(f), 20, 70, len(f)]
    for what, sql, rows in zip(COVERS, R.GOLD_STATEMENTS, expect):
        result = orc.run_reference_sql(host, ctx.sql_describe(sql, 0), threads=1)
        got = sum(1 for line in result.splitlines() if line and not line.startswith("#"))
        assert got == rows, (sql, got, rows)
        out["cases"].append({"covers": what, "sql": sql, "rows": rows, "result": result})
        print(sql, "-> %d rows, %d bytes" % (rows, len(result)), file=sys.stderr)
    ctx.close()
    with open(os.path.join(HERE, "result_pack_reference.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
