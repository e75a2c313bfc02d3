#!/usr/bin/env python3
"""TPC-H Q18's shape (tests/derivedcases.py q18: a HAVING-style selection over the l_orderkey aggregation as the build side of three
joins, an aggregation on top) at SF1 and SF10: steady-state ms per execution, launches per execution, and where the time goes - the
derived sub-query alone (the same aggregation as a statement of its own), the derived-table writer (k_derived_columns, from a separate
`rocprofv3 --kernel-trace --stats` run) and the rest (the three joins and the outer aggregation).  The writer's bytes are
rows x (tuple bytes + column bytes); its fraction of the byte bound is those bytes / 8 TB/s over its measured time.
Each case runs in a child process of its own under `timeout -k 10`; a case that fails ends the script there.

usage: python tools/derived_agg_timing.py [--reps N] [--sf 1 10] [--rocprof] [--out FILE.jsonl]
       python tools/derived_agg_timing.py --reference      (the unmodified reference's CPU time at SF1, one thread; oracle/_ref)
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8e12
THRESHOLD = {1: 300, 10: 300}


def _setup(sf):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from resql_amd import tpch_full
    import derivedcases as D
    return D, tpch_full.database(float(sf), fill_unused=False)


def _sub_plan(D, db):
    p = D._plan(db)
    q = p.sum(p.attr("l_quantity"))
    return p.set_root(p.materialize(p.aggregation([q], [p.attr("l_orderkey")], p.scan("lineitem"))), request_all=True)


def child(sf, reps):
    D, db = _setup(sf)
    from resql_amd import engine
    ctx = engine.Context(device=0)
    tabs = [ctx.table(db[k]) for k in D.TABLES]
    out = {"case": "q18_sf%g" % sf, "sf": sf, "threshold": THRESHOLD[sf]}
    for key, plan in (("statement", D.q18(db, threshold=THRESHOLD[sf])), ("derived_subquery", _sub_plan(D, db))):
        q = ctx.compile(plan, tabs)
        q.execute()
        wall, kern = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            q.execute()
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(q.report().kernel_time_ms)
        r = q.result(text=False)
        out[key] = {"ms_per_execution_best": min(wall), "ms_per_execution_median": sorted(wall)[len(wall) // 2],
                    "kernel_ms_best": min(kern), "launches_per_execution": q.report().num_kernels, "rows": r.n_rows}
        q.close()
    out["derived_rows"] = out["derived_subquery"]["rows"]
    out["writer_bytes"] = out["derived_rows"] * (12 + 12)      # l_orderkey INT + SUM DECIMAL: 12 tuple bytes, 12 column bytes per row
    for t in tabs:
        t.close()
    ctx.close()
    print(json.dumps(out))


def writer_stats(sf, reps):
    d = tempfile.mkdtemp(prefix="derived_prof_")
    cmd = ["timeout", "-k", "10", "1200", "rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--",
           sys.executable, os.path.abspath(__file__), "--child", str(sf), "--reps", str(reps)]
    pr = subprocess.run(cmd, capture_output=True, text=True)
    if pr.returncode != 0:
        return {"writer": "not measured", "rocprof_status": pr.returncode, "rocprof_tail": pr.stderr[-500:]}
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                if "k_derived_columns" in row.get("Name", ""):
                    return {"writer_calls": int(row["Calls"]), "writer_ms_avg": float(row["AverageNs"]) / 1e6}
    return {"writer": "not measured", "rocprof_status": 0}


def reference():
    D, db = _setup(1)
    from oracle import orc
    _, tm = orc.run_reference(D.q18(db, threshold=THRESHOLD[1]), threads=1, repeat=3)
    print(json.dumps({"case": "q18_sf1_reference_cpu", "threads": 1, "exec_ms": tm["exec_ms"], "compile_ms": tm["compile_ms"]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", type=float)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sf", type=float, nargs="+", default=[1, 10])
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        child(int(a.child), a.reps)
        return
    if a.reference:
        reference()
        return
    lines = []
    for sf in a.sf:
        pr = subprocess.run(["timeout", "-k", "10", "1200", sys.executable, os.path.abspath(__file__), "--child", str(sf), "--reps", str(a.reps)],
                            capture_output=True, text=True)
        if pr.returncode != 0:
            sys.stderr.write(f"sf {sf}: exit status {pr.returncode}\n{pr.stdout[-2000:]}\n{pr.stderr[-4000:]}\n")
            sys.exit(1)
        rec = json.loads(pr.stdout.strip().splitlines()[-1])
        if a.rocprof:
            rec.update(writer_stats(sf, 3))
            if "writer_ms_avg" in rec:
                rec["writer_byte_bound_ms"] = rec["writer_bytes"] / HBM_BYTES_PER_S * 1e3
                rec["writer_fraction_of_byte_bound"] = rec["writer_byte_bound_ms"] / rec["writer_ms_avg"]
                rec["joins_and_outer_aggregation_ms"] = (rec["statement"]["ms_per_execution_best"] - rec["derived_subquery"]["ms_per_execution_best"]
                                                         - rec["writer_ms_avg"])
        else:
            rec["writer"] = "not measured"
        line = json.dumps(rec)
        print(line)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
