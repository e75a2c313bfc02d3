#!/usr/bin/env python3
"""Pairs per second of the nested-loops join's pair loop at SF1 (RSQ_ENGINE_NESTED_LOOPS), against its VALU bound.

  lineitem_x_nation   count with a predicate across the sides: 6 M outer rows (lineitem) x 25 inner rows (nation)
  supplier_x_orders   grouped by a dense key: 10 000 outer rows (supplier) x 1.5 M inner rows (orders), about 1.5e10 pairs

The FROM order decides the sides: the reference folds pieces in creation order, so the LAST table is the outer, streaming side.
Each case runs in a child process of its own under `timeout -k 10`; a case that fails or times out ends the script there.
VALU bound = pairs x VALU instructions per pair (read off the kernel's ISA, tools/isa.sh) / (256 CUs x 64 lanes x 2.4 GHz).

--slices N is the context's nested_loops_inner_slices (0: the engine chooses per execution, 1: the inner range is never split); every
output line holds it, and the slice count the last execution launched with.

usage: python tools/nested_loops_timing.py [--reps N] [--slices N] [--out FILE.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (statement, outer table, inner table, VALU instructions per pair in the pair loop)
CASES = {
    "lineitem_x_nation": ("select count(*) from nation, lineitem where l_quantity < n_nationkey * 2", "lineitem", "nation", 2),
    "supplier_x_orders": ("select s_nationkey, count(*) from orders, supplier where o_totalprice < s_acctbal * 10 group by s_nationkey",
                          "supplier", "orders", 2),
}
CLOCK_HZ = 2.4e9
LANES_PER_CLOCK = 256 * 64


def child(name, reps, slices):
    sys.path.insert(0, ROOT)
    from resql_amd import engine, tpch_full
    sql, outer, inner, valu = CASES[name]
    db = tpch_full.database(1.0)                     # (every column filled: o_totalprice is not one the TPC-H statements read)
    ctx = engine.Context(device=0, engine_flags=engine.ENGINE_NESTED_LOOPS, nested_loops_max_pairs=1 << 40,
                         nested_loops_inner_slices=slices)
    tabs = [ctx.table(db[k]) for k in sorted(db)]
    q = ctx.sql_compile(sql, tabs)
    q.execute()                                      # (first execution: kernels loaded, inner side sized)
    kernel_s = []
    for _ in range(reps):
        q.execute()
        kernel_s.append(q.report().kernel_time_ms / 1e3)
    best = min(kernel_s)
    pairs = db[outer].n_rows * db[inner].n_rows
    bound = pairs * valu / (LANES_PER_CLOCK * CLOCK_HZ)
    print(json.dumps({"case": name, "sql": sql, "pairs": pairs, "slices": slices, "slices_launched": q.nested_loops_slices(), "kernel_s": kernel_s,
                      "kernel_s_best": best, "pairs_per_s": pairs / best,
                      "valu_per_pair": valu, "valu_bound_s": bound, "fraction_of_valu_bound": bound / best, "result_rows": q.result().n_rows}))
    q.close()
    for t in tabs:
        t.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slices", type=int, default=0)
    ap.add_argument("--only", choices=sorted(CASES), help="run this case alone")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps, a.slices)
        return
    lines = []
    for name in CASES:
        if a.only and name != a.only:
            continue
        pr = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps),
                             "--slices", str(a.slices)],
                            capture_output=True, text=True)
        if pr.returncode != 0:
            sys.stderr.write(f"{name}: exit status {pr.returncode}\n{pr.stdout[-2000:]}\n{pr.stderr[-4000:]}\n")
            sys.exit(1)
        line = pr.stdout.strip().splitlines()[-1]
        print(line)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
