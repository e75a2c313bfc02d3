"""GROUP BY over a dictionary-coded column: dense group ids from the codes against the hash aggregation of the build before them, both
with RSQ_DICT_SCANS=1, on one MI355X in one session.
usage: python tools/dict_group_bench.py [SF] --parent-tree DIR [--runs N] [--repeat N] [--out FILE] [--sha SHA] [--also NAME=VALUE]
DIR is a built checkout of the parent commit (its resql_amd/libresql_hip.so in place); this file's own tree is the other build.  One
worker process per build generates lineitem and orders of scale factor SF, loads them and compiles the two statements - TPC-H Q12
and `select l_shipmode, sum(l_quantity), count(*) from lineitem group by l_shipmode` -; both stay resident and the runs ALTERNATE
between them, so that clocks and neighbours change under both alike.  A run is `repeat` executions of each statement; per build and
statement the file gets every run's median and the median, minimum and maximum over the runs' medians (whole execution and kernels),
the aggregation's explain step, and whether both builds gave one answer.  One JSON line per figure, stamped with --sha.  --also adds a
third worker: this tree again with one more environment switch (RSQ_AGG_MODE=1: the register form also behind Q12's compaction)."""
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATEMENTS = {
    "q12": None,                                                          # (tpch_full.QUERIES["q12"], resolved in the worker)
    "group_by_shipmode": "select l_shipmode, sum(l_quantity), count(*) from lineitem group by l_shipmode",
}


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def worker(tree, sf, repeat, also=""):
    """one build: load, compile, then a run per line read from the orchestrator ('run' / anything else ends it)"""
    sys.path.insert(0, tree)
    os.environ["RSQ_DICT_SCANS"] = "1"
    if also:
        os.environ[also.split("=", 1)[0]] = also.split("=", 1)[1]
    from resql_amd import engine, tpch_full
    host = [tpch_full.orders(sf), tpch_full.lineitem(sf)]
    print(f"[{tree} {also}] tables generated", file=sys.stderr, flush=True)
    ctx = engine.Context(device=0)
    tabs = [ctx.table(t) for t in host]
    print(f"[{tree} {also}] tables loaded", file=sys.stderr, flush=True)
    qs = {}
    for name, sql in STATEMENTS.items():
        q = ctx.sql_compile(sql or tpch_full.QUERIES[name], tabs if name == "q12" else tabs[1:])
        q.await_kernels()
        for _ in range(3):
            q.execute()
        qs[name] = q
    agg = {n: [s for l in q.explain.splitlines() if l.startswith("pipeline") for s in l.split(" -> ") if "aggregation" in s] for n, q in qs.items()}
    print(json.dumps({"ready": True, "aggregation": agg, "answers": {n: q.result().text for n, q in qs.items()}}), flush=True)
    for line in sys.stdin:
        if line.strip() != "run":
            break
        out = {}
        for name, q in qs.items():
            ex, ke = [], []
            for _ in range(repeat):
                q.execute()
                r = q.report()
                ex.append(r.execution_time_ms)
                if r.kernel_time_ms > 0:
                    ke.append(r.kernel_time_ms)
            out[name] = {"exec_ms_median": statistics.median(ex), "exec_ms_min": min(ex), "kernel_ms_median": statistics.median(ke) if ke else None}
        print(json.dumps(out), flush=True)
    for q in qs.values():
        q.close()
    for t in tabs:
        t.close()
    ctx.close()


def main():
    sf = float(sys.argv[1]) if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else 10.0
    runs, repeat, out_path, sha = arg("--runs", 7), arg("--repeat", 30), arg("--out", ""), arg("--sha", "")
    trees = {"parent": os.path.abspath(arg("--parent-tree", "")), "this": HERE}
    also = {b: "" for b in trees}
    if arg("--also", ""):
        trees["this " + arg("--also", "")] = HERE
        also["this " + arg("--also", "")] = arg("--also", "")
    out = open(out_path, "w") if out_path else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    procs = {b: subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", t, str(sf), str(repeat), also[b]], stdin=subprocess.PIPE,
                                 stdout=subprocess.PIPE, text=True) for b, t in trees.items()}
    try:
        ready = {b: json.loads(p.stdout.readline()) for b, p in procs.items()}
        for name in STATEMENTS:
            emit({"statement": name, "sf": sf, "RSQ_DICT_SCANS": "1", "same_answer": all(ready[b]["answers"][name] == ready["parent"]["answers"][name] for b in trees),
                  "aggregation": {b: ready[b]["aggregation"][name] for b in trees}})
        series = {b: {n: [] for n in STATEMENTS} for b in trees}
        for run in range(1, runs + 1):
            for b in (list(trees) if run % 2 else list(trees)[::-1]):             # (alternating, and alternating who goes first)
                procs[b].stdin.write("run\n")
                procs[b].stdin.flush()
                got = json.loads(procs[b].stdout.readline())
                for n, v in got.items():
                    series[b][n].append(v)
                    emit(dict(v, statement=n, build=b, run=run))
        for n in STATEMENTS:
            for b in trees:
                ex = [v["exec_ms_median"] for v in series[b][n]]
                ke = [v["kernel_ms_median"] for v in series[b][n] if v["kernel_ms_median"] is not None]
                emit({"summary": n, "build": b, "runs": runs, "executions_per_run": repeat,
                      "exec_ms": {"median": round(statistics.median(ex), 4), "min": round(min(ex), 4), "max": round(max(ex), 4)},
                      "kernel_ms": {"median": round(statistics.median(ke), 4), "min": round(min(ke), 4), "max": round(max(ke), 4)} if ke else None})
    finally:
        for p in procs.values():
            try:
                p.stdin.write("quit\n")
                p.stdin.close()
            except OSError:
                pass
        for p in procs.values():
            p.wait()
    if sha:
        emit({"head_sha": sha})


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--worker":
        worker(sys.argv[2], float(sys.argv[3]), int(sys.argv[4]), sys.argv[5] if len(sys.argv) > 5 else "")
    else:
        main()
