"""GROUP BY over a dictionary-coded column: dense group ids from the codes against the hash aggregation of the build before them, both
with RSQ_DICT_SCANS=1, on one MI355X in one session.
usage: python tools/dict_group_bench.py [SF] --parent-tree DIR [--runs N] [--repeat N] [--out FILE] [--sha SHA] [--also NAME=VALUE]
DIR is a built checkout of the parent commit (its resql_amd/libresql_hip.so in place); this file's own tree is the other build.  One
worker process per build generates lineitem and orders of scale factor SF, loads them and compiles the two statements - TPC-H Q12
and `select l_shipmode, sum(l_quantity), count(*) from lineitem group by l_shipmode` -; both stay resident and the runs ALTERNATE
between them, so that clocks and neighbours change under both alike.  A run is `repeat` executions of each statement; per build and
statement the file gets every run's median and the median, minimum and maximum over the runs' medians (whole execution and kernels),
the aggregation's explain step, and whether both builds gave one answer.  One JSON line per figure, stamped with --sha.  --also adds a
third worker: this tree again with one more environment switch (RSQ_AGG_MODE=1: the register form also behind Q12's compaction).

usage: python tools/dict_group_bench.py [SF] --tail [--runs N] [--repeat N] [--out FILE] [--sha SHA]
The device tail of a dense aggregation with a coded key against its host tail (RSQ_DEVICE_TAIL=0, which is the parent commit's tail
for such a statement): `group by l_shipmode, l_suppkey`, one process, one compiled statement, the switch read at every execution and
the runs alternating.  Per run and over the runs: whole execution, kernels and tail (rsq_report.finalize_time_ms), as
tools/hash_tail_bench.py prints them.

usage: python tools/dict_group_bench.py [SF] --join-keys --parent-tree DIR [--runs N] [--repeat N] [--out FILE] [--sha SHA]
Dense group ids for a string from a join's build side (RSQ_DICT_SCANS=2): TPC-H Q5, whose n_name reaches lineitem's aggregation through
the supplier's table, and Q12 as the control (its key is lineitem's own column: 1 and 2 give it one kernel).  One worker per build
loads the six tables Q5 reads with the images on and compiles both statements under RSQ_DICT_SCANS = 0, 1 and 2 (the parent: 0 and 1);
all stay resident and the runs alternate between builds and switches.  Every answer is compared with tests/golden/ref_full_<q>_sf<SF>.tbl.

usage: python tools/dict_group_bench.py [SF] --shards N[,N...] [--runs N] [--repeat N] [--out FILE] [--sha SHA]
One dictionary across shards (ENGINE_DICT_MULTI): TPC-H Q12 and Q5 over N shard contexts on ONE GPU (MultiContext([0] * N)), lineitem
sharded by rows and every other table replicated, RSQ_DICT_SCANS=2.  Two handles of this build stay resident, one with the flag and one
without (the parent commit's behaviour), and the runs alternate between them.  Per handle and statement: the merge the statement takes,
whether the answer is tests/golden/ref_full_<q>_sf<SF>.tbl, and median [min, max] of execution, kernel and collective time.  N contexts
on one device take turns on it: the figures compare the kernel form and the merge form, they say nothing about scaling.

usage: python tools/dict_group_bench.py [SF] --recode [--runs N] [--out FILE] [--sha SHA]
The recode pass that installs a union dictionary (k_dict_recode) against what it replaces, encoding the wide column anew
(k_dict_encode), over lineitem's l_shipmode at scale factor SF: device time by events, one process, the two alternating.  --recode and
--shards may be given together: the tables are generated once."""
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


def join_worker(tree, sf, repeat, switches):
    """one build: the tables with the images on, Q5 and Q12 compiled under every switch, then a run per line read from the orchestrator"""
    sys.path.insert(0, tree)
    os.environ["RSQ_DICT_SCANS"] = max(switches)                          # (the images are built when a table is created)
    from resql_amd import engine, tpch_full
    db = tpch_full.database(sf, fill_unused=False)
    names = sorted(db)
    print(f"[{tree}] tables generated", file=sys.stderr, flush=True)
    ctx = engine.Context(device=0)
    tabs = [ctx.table(db[k]) for k in names]
    print(f"[{tree}] tables loaded", file=sys.stderr, flush=True)
    qs, ready = {}, {"ready": True, "aggregation": {}, "equals_reference_answer": {}, "answers": {}}
    for name in ("q5", "q12"):
        gold = os.path.join(HERE, "tests", "golden", f"ref_full_{name}_sf{sf:g}.tbl")
        want = open(gold, encoding="latin1").read() if os.path.exists(gold) else None
        for sw in switches:
            os.environ["RSQ_DICT_SCANS"] = sw                             # (read when a statement is compiled)
            q = ctx.sql_compile(tpch_full.QUERIES[name], tabs)
            q.await_kernels()
            for _ in range(3):
                q.execute()
            key = f"{name}@{sw}"
            qs[key] = q
            ready["aggregation"][key] = [s for l in q.explain.splitlines() if l.startswith("pipeline") for s in l.split(" -> ") if "aggregation" in s]
            ready["answers"][key] = q.result().text
            ready["equals_reference_answer"][key] = None if want is None else q.result().text == want
    print(json.dumps(ready), flush=True)
    flip = False
    for line in sys.stdin:
        if line.strip() != "run":
            break
        out = {}
        for key in (sorted(qs, reverse=flip)):
            q, ex, ke = qs[key], [], []
            for _ in range(repeat):
                q.execute()
                r = q.report()
                ex.append(r.execution_time_ms)
                if r.kernel_time_ms > 0:
                    ke.append(r.kernel_time_ms)
            out[key] = {"exec_ms_median": statistics.median(ex), "exec_ms_min": min(ex), "kernel_ms_median": statistics.median(ke) if ke else None}
        flip = not flip
        print(json.dumps(out), flush=True)
    for q in qs.values():
        q.close()
    for t in tabs:
        t.close()
    ctx.close()


def join_keys(sf, runs, repeat, emit, parent_tree):
    trees = {"this": (HERE, "0,1,2")}
    if parent_tree:
        trees = {"parent": (os.path.abspath(parent_tree), "0,1"), "this": (HERE, "0,1,2")}
    procs = {b: subprocess.Popen([sys.executable, os.path.abspath(__file__), "--join-worker", t, str(sf), str(repeat), sw], stdin=subprocess.PIPE,
                                 stdout=subprocess.PIPE, text=True) for b, (t, sw) in trees.items()}
    try:
        ready = {b: json.loads(p.stdout.readline()) for b, p in procs.items()}
        first = ready["this"]["answers"]
        for b in trees:
            for key, agg in ready[b]["aggregation"].items():
                emit({"statement": key.split("@")[0], "sf": sf, "RSQ_DICT_SCANS": key.split("@")[1], "build": b, "aggregation": agg,
                      "equals_reference_answer": ready[b]["equals_reference_answer"][key],
                      "same_answer_as_this_at_0": ready[b]["answers"][key] == first[key.split("@")[0] + "@0"]})
        series = {b: {} for b in trees}
        for run in range(1, runs + 1):
            for b in (list(trees) if run % 2 else list(trees)[::-1]):             # (alternating, and alternating who goes first)
                procs[b].stdin.write("run\n")
                procs[b].stdin.flush()
                for key, v in json.loads(procs[b].stdout.readline()).items():
                    series[b].setdefault(key, []).append(v)
                    emit(dict(v, statement=key.split("@")[0], RSQ_DICT_SCANS=key.split("@")[1], build=b, run=run))
        for b in trees:
            for key, vs in sorted(series[b].items()):
                ex = [v["exec_ms_median"] for v in vs]
                ke = [v["kernel_ms_median"] for v in vs if v["kernel_ms_median"] is not None]
                emit({"summary": key.split("@")[0], "RSQ_DICT_SCANS": key.split("@")[1], "build": b, "runs": runs, "executions_per_run": repeat,
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


def shards_mode(sf, n, runs, repeat, emit, db):
    os.environ["RSQ_DICT_SCANS"] = "2"
    from resql_amd import engine, plan as P, tpch_full
    names = sorted(db)
    li = db["lineitem"]
    emit({"note": f"{n} shard contexts on one device take turns on it: these figures compare the kernel form and the merge form of the two "
                  "settings, not scaling", "sf": sf, "shards": n})
    handles, qs = {}, {}
    try:
        for flag in ("off", "on"):
            m = engine.MultiContext([0] * n, engine_flags=engine.ENGINE_DICT_MULTI if flag == "on" else 0)
            per = []
            for i, sh in enumerate(m.shards):
                r0, nr = m.shard_rows(li.n_rows, i)
                part = P.Table("lineitem", [P.Column(c.name, c.type, None if c.data is None else c.data[r0:r0 + nr]) for c in li.columns], nr)
                tabs = [sh.table(part if k == "lineitem" else db[k]) for k in names]
                tabs[names.index("lineitem")].set_row0(r0)
                per.append(tabs)
            # the plan is made over shard 0's tables: lineitem's shards size like the whole table from the start (the compile would unify
            # them anyway), or a quarter of lineitem is no larger than orders and the planner turns Q12's join round
            shards = [tabs[names.index("lineitem")] for tabs in per]
            blobs = [t.stats_blob() for t in shards]
            for t in shards:
                t.unify_shard_stats(blobs)
            handles[flag] = (m, per)
            print(f"[{flag}] tables loaded", file=sys.stderr, flush=True)
        for name in ("q12", "q5"):
            gold = os.path.join(HERE, "tests", "golden", f"ref_full_{name}_sf{sf:g}.tbl")
            want = open(gold, encoding="latin1").read() if os.path.exists(gold) else None
            m0, per0 = handles["off"]
            plan = m0.shards[0].sql_plan(tpch_full.QUERIES[name], per0[0], [db[k] for k in names])
            for flag, (m, per) in handles.items():
                q = m.compile(plan, per)
                for _ in range(3):
                    q.execute()
                qs[(name, flag)] = q
                text = q.result().text
                emit({"statement": name, "sf": sf, "shards": n, "ENGINE_DICT_MULTI": flag, "merge": q.merge_name,
                      "aggregation": [s for l in q.explain(0).splitlines() if l.startswith("pipeline") for s in l.split(" -> ") if "aggregation" in s],
                      "equals_reference_answer": None if want is None else text == want})
        series = {k: [] for k in qs}
        for run in range(1, runs + 1):
            for key in (sorted(qs) if run % 2 else sorted(qs, reverse=True)):     # (alternating, and alternating who goes first)
                q, ex, ke, co = qs[key], [], [], []
                for _ in range(repeat):
                    q.execute()
                    r = q.report()[0]
                    ex.append(r.execution_time_ms)
                    ke.append(r.kernel_time_ms)
                    co.append(q.collective_ms)
                v = {"exec_ms_median": statistics.median(ex), "kernel_ms_median": statistics.median(ke), "collective_ms_median": statistics.median(co)}
                series[key].append(v)
                emit(dict(v, statement=key[0], ENGINE_DICT_MULTI=key[1], shards=n, run=run))
        for key, vs in sorted(series.items()):
            cols = {k: [v[k + "_ms_median"] for v in vs] for k in ("exec", "kernel", "collective")}
            emit(dict({"summary": key[0], "ENGINE_DICT_MULTI": key[1], "shards": n, "runs": runs, "executions_per_run": repeat},
                      **{k + "_ms": {"median": round(statistics.median(c), 4), "min": round(min(c), 4), "max": round(max(c), 4)} for k, c in cols.items()}))
    finally:
        for q in qs.values():
            q.close()
        for m, per in handles.values():
            m.close()


def recode_mode(sf, runs, emit, db):
    os.environ["RSQ_DICT_SCANS"] = "1"
    from resql_amd import engine, plan as P
    c = db["lineitem"].col("l_shipmode")
    ctx = engine.Context(device=0)
    tab = ctx.table(P.Table("lineitem", [P.Column(c.name, c.type, c.data)], len(c.data)))
    try:
        series = {"recode": [], "encode": []}
        for run in range(runs + 1):                                           # (run 0 warms both)
            for which in (("recode", "encode") if run % 2 else ("encode", "recode")):
                ms = tab.time_dictionary_pass("l_shipmode", 0 if which == "recode" else 1)
                if run:
                    series[which].append(ms)
                    emit({"pass": which, "column": "l_shipmode", "sf": sf, "rows": tab.n_rows, "run": run, "device_ms": round(ms, 4)})
        for which, v in series.items():
            emit({"summary": which, "column": "l_shipmode", "sf": sf, "rows": tab.n_rows, "entries": tab.image_info("l_shipmode")[2], "runs": runs,
                  "device_ms": {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}})
    finally:
        tab.close()
        ctx.close()


TAIL_SQL = "select l_shipmode, l_suppkey, count(*), sum(l_quantity) from lineitem group by l_shipmode, l_suppkey"


def tail_rows(sf, runs, repeat, emit):
    """device tail against RSQ_DEVICE_TAIL=0 over one compiled statement"""
    sys.path.insert(0, HERE)
    os.environ["RSQ_DICT_SCANS"] = "1"
    from resql_amd import engine, tpch_full
    ctx = engine.Context(device=0)
    tab = ctx.table(tpch_full.lineitem(sf))
    q = ctx.sql_compile(TAIL_SQL, [tab])
    q.await_kernels()
    answers, series = {}, {"device": [], "host": []}
    try:
        for run in range(runs + 1):                                           # (run 0 warms both tails and keeps their answers)
            for tail in (("device", "host") if run % 2 else ("host", "device")):
                os.environ["RSQ_DEVICE_TAIL"] = "1" if tail == "device" else "0"
                ex, ke, fi = [], [], []
                for _ in range(repeat if run else 3):
                    q.execute()
                    r = q.report()
                    ex.append(r.execution_time_ms)
                    fi.append(r.finalize_time_ms)
                    if r.kernel_time_ms > 0:
                        ke.append(r.kernel_time_ms)
                if not run:
                    answers[tail] = q.result().text
                    continue
                v = {"exec_ms_median": statistics.median(ex), "kernel_ms_median": statistics.median(ke) if ke else None, "tail_ms_median": statistics.median(fi)}
                series[tail].append(v)
                emit(dict(v, statement=TAIL_SQL, tail=tail, run=run))
        agg = [s for l in q.explain.splitlines() if l.startswith("pipeline") for s in l.split(" -> ") if "aggregation" in s]
        emit({"statement": TAIL_SQL, "sf": sf, "RSQ_DICT_SCANS": "1", "same_answer": answers["device"] == answers["host"], "aggregation": agg})
        for tail, vs in series.items():
            cols = {k: [v[k + "_ms_median"] for v in vs if v[k + "_ms_median"] is not None] for k in ("exec", "kernel", "tail")}
            emit(dict({"summary": "group_by_shipmode_suppkey", "tail": tail, "runs": runs, "executions_per_run": repeat},
                      **{k + "_ms": {"median": round(statistics.median(c), 4), "min": round(min(c), 4), "max": round(max(c), 4)} if c else None for k, c in cols.items()}))
    finally:
        os.environ.pop("RSQ_DEVICE_TAIL", None)
        q.close()
        tab.close()
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

    if "--shards" in sys.argv or "--recode" in sys.argv:
        sys.path.insert(0, HERE)
        from resql_amd import tpch_full
        db = tpch_full.database(sf, fill_unused=False)                        # (generated once for everything asked for)
        print("tables generated", file=sys.stderr, flush=True)
        if "--recode" in sys.argv:
            recode_mode(sf, runs, emit, db)
        for n in ([int(x) for x in arg("--shards", "").split(",")] if "--shards" in sys.argv else []):
            shards_mode(sf, n, runs, repeat, emit, db)
        if sha:
            emit({"head_sha": sha})
        return

    if "--join-keys" in sys.argv:
        join_keys(sf, runs, repeat, emit, arg("--parent-tree", ""))
        if sha:
            emit({"head_sha": sha})
        return

    if "--tail" in sys.argv:
        tail_rows(sf, runs, repeat, emit)
        if sha:
            emit({"head_sha": sha})
        return

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
    if len(sys.argv) > 1 and sys.argv[1] == "--join-worker":
        join_worker(sys.argv[2], float(sys.argv[3]), int(sys.argv[4]), sys.argv[5].split(","))
    elif len(sys.argv) > 1 and sys.argv[1] == "--worker":
        worker(sys.argv[2], float(sys.argv[3]), int(sys.argv[4]), sys.argv[5] if len(sys.argv) > 5 else "")
    else:
        main()
