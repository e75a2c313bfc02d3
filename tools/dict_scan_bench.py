"""Dictionary images against the wide string scans (RSQ_DICT_SCANS=0) on one resident TPC-H database, in one session.
usage: python tools/dict_scan_bench.py [SF] [--runs N] [--repeat N] [--only q19] [--out FILE] [--skip-warm]
The database is generated once and loaded twice, into a context whose tables were created with the switch off and one with RSQ_DICT_SCANS=1
(the images are opt-in); the creation of lineitem, part and customer (whose name, address, phone and comment columns have far more than 256 values:
what the sample pass costs) is timed both ways.  Then N runs alternate between the two: every run compiles each of the eight
statements afresh and takes the median whole-execution and kernel time of `repeat` executions.  One JSON line per figure."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from resql_amd import engine, tpch_full  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


sf = float(sys.argv[1]) if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else 1.0
runs, repeat, only, out_path = arg("--runs", 3), arg("--repeat", 30), arg("--only", ""), arg("--out", "")
out = open(out_path, "w") if out_path else None


def emit(d):
    line = json.dumps(d)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


t0 = time.time()
db = tpch_full.database(sf, fill_unused=sf < 1.0)
names = sorted(db)
emit({"generated_sf": sf, "seconds": round(time.time() - t0, 1), "rows": {k: db[k].n_rows for k in names}})

ctxs, tabs = {}, {}
# The switch is read from the environment when a table is created and when a statement is compiled.  The switch-off context's tables
# have no images, so its statements scan wide whatever the variable says later; it is still set per run so that both sides of a run are
# compiled under the setting they were loaded with.
# (the first pair of loads also warms the driver: the second pair's creation times are the ones to read; --skip-warm loads once)
for sw in (("0", "1") if "--skip-warm" in sys.argv else ("0", "1", "0", "1")):
    os.environ["RSQ_DICT_SCANS"] = sw
    if sw in ctxs:
        for t in tabs[sw]:
            t.close()
        ctxs[sw].close()
    ctxs[sw] = engine.Context(device=0)
    made = []
    for k in names:
        t1 = time.perf_counter()
        made.append(ctxs[sw].table(db[k]))
        ms = (time.perf_counter() - t1) * 1e3
        if k in ("lineitem", "part", "customer"):
            emit({"create_table": k, "RSQ_DICT_SCANS": sw, "pass": 2 if sw in tabs else 1, "ms": round(ms, 1),
                  "column_image_bytes": ctxs[sw].memory_stats()["column_image_bytes"]})
    tabs[sw] = made

answers = {}
for run in range(1, runs + 1):
    for sw in ("0", "1"):
        os.environ["RSQ_DICT_SCANS"] = sw
        for name, sql in sorted(tpch_full.QUERIES.items()):
            if only and name not in only.split(","):
                continue
            q = ctxs[sw].sql_compile(sql, tabs[sw])
            q.await_kernels()
            q.execute()
            ex, ke = [], []
            for _ in range(repeat):
                q.execute()
                r = q.report()
                ex.append(r.execution_time_ms)
                if r.kernel_time_ms > 0:
                    ke.append(r.kernel_time_ms)
            text = q.result().text
            same = answers.setdefault(name, text) == text
            stored = [l.split(" -> ")[0].split("scan ")[1] for l in q.explain.splitlines() if l.startswith("pipeline")]
            emit({"query": name, "RSQ_DICT_SCANS": sw, "run": run, "exec_ms_median": round(statistics.median(ex), 4), "exec_ms_min": round(min(ex), 4),
                  "kernel_ms_median": round(statistics.median(ke), 4) if ke else None, "same_answer": same, "scans": stored})
            q.close()
for sw in ctxs:
    for t in tabs[sw]:
        t.close()
    ctxs[sw].close()
