#!/usr/bin/env python3
"""Generate tests/golden/nlj_reference.json: what the UNMODIFIED reference does with the statements of tests/nljcases.py
over the eight-table database (SF 0.01, one thread): its planner's operator tree (with the MaterializeOp wrappers a
NestedLoopsJoinOp puts around its children) and the result of its own JIT execution, or its refusal.

Run where the reference is built (oracle/_ref/ref_harness):  python tests/golden/make_nlj_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from resql_amd import engine, tpch_full  # noqa: E402
from oracle import orc  # noqa: E402
import nljcases  # noqa: E402

SF = 0.01


def main():
    ctx = engine.Context(device=-1)
    db = tpch_full.database(SF)
    host = [db[k] for k in sorted(db)]
    out = {"sf": SF, "tables": sorted(db), "cases": []}
    for sql in nljcases.STATEMENTS:
        toks = ctx.sql_describe(sql, 0)
        case = {"sql": sql}
        try:
            case["plan"] = orc.run_reference_sql(host, toks, dump_plan=True)
        except orc.OracleError as e:
            case["plan"] = "REFUSED " + str(e).strip().splitlines()[-1][:200] + "\n"
        try:
            case["result"] = orc.run_reference_sql(host, toks, threads=1)
        except orc.OracleError as e:
            case["refused"] = str(e).strip().splitlines()[-1][:300]
        out["cases"].append(case)
        print(sql, "->", "refused: " + case["refused"] if "refused" in case else "%d bytes" % len(case["result"]), file=sys.stderr)
    ctx.close()
    with open(os.path.join(HERE, "nlj_reference.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
