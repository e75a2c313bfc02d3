"""What ORDER BY ... LIMIT over a materialisation costs at SF1 (6 M lineitem rows), host path against device path against the parent
commit.  A development aid, not part of bench.py.
usage: python tools/order_limit_timing.py [SF] --parent-tree DIR [--parent-commit SHA] [--repeat N] [--out FILE] [--parent-out FILE] [--limit-seconds N]
DIR is a built checkout of the commit before Context.set_order_limit existed.  Four processes run one after the other on one device,
alternating: the parent, this tree with the setter at 1, this tree with the setter at 0, the parent again (its two runs show the
run-to-run spread).  Each generates lineitem, compiles three statements and executes each once unrecorded and N times (default 3)
recorded:
  all         order by l_extendedprice desc, l_orderkey, l_linenumber limit 10 over all rows
  filtered    the same behind l_shipdate < date '1994-01-01'
  overflow    order by l_linenumber, l_extendedprice desc, l_orderkey limit 10: a quarter of the rows share the first key's leading value,
              so the selection runs, counts more candidates than its capacity, and the host path follows - the device path's worst case.
              (The one-key form `order by l_linenumber limit 10` is not run: the reference's quicksort - Lomuto, the pivot from the segment's
              end - is quadratic over the 860 K rows that tie on each value, on either path and on the parent.)
One JSON line per process and statement - wall, execution, kernel and finalize ms of every recorded execution, select_ms / copy_ms /
tail_ms and the report of the last one, a digest of the result text - goes to FILE (this tree) or the parent's FILE; a summary line per
statement compares the medians and the digests.  Every process is ended after N seconds (default 400)."""
import hashlib
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLUMNS = ["l_orderkey", "l_linenumber", "l_extendedprice", "l_shipdate"]
STATEMENTS = [
    ("all", "select l_orderkey, l_linenumber, l_extendedprice, l_shipdate from lineitem order by l_extendedprice desc, l_orderkey, l_linenumber limit 10"),
    ("filtered", "select l_orderkey, l_linenumber, l_extendedprice, l_shipdate from lineitem where l_shipdate < date '1994-01-01' "
                 "order by l_extendedprice desc, l_orderkey, l_linenumber limit 10"),
    ("overflow", "select l_orderkey, l_linenumber, l_extendedprice, l_shipdate from lineitem order by l_linenumber, l_extendedprice desc, l_orderkey limit 10"),
]


def _arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def measure(tree, setter, label, sf, repeat):
    sys.path.insert(0, tree)
    from resql_amd import engine, plan as P, tpch_full
    li = tpch_full.lineitem(sf)
    table = P.Table("lineitem", [c for c in li.columns if c.name in COLUMNS], li.n_rows)
    ctx = engine.Context(device=0)
    if setter is not None:
        ctx.set_order_limit(setter)
    tab = ctx.table(table)
    for name, sql in STATEMENTS:
        q = ctx.sql_compile(sql, [tab])
        q.await_kernels()          # (the specialised kernels, not the interpreter tier a cold code-object cache starts on)
        line = {"label": label, "setter": setter, "statement": name, "sql": sql, "sf": sf, "table_rows": table.n_rows,
                "launches": [], "wall_ms": [], "execution_ms": [], "kernel_ms": [], "finalize_ms": [], "select_ms": [], "copy_ms": [], "tail_ms": []}
        for i in range(repeat + 1):
            t0 = time.perf_counter()
            q.execute()
            wall = (time.perf_counter() - t0) * 1e3
            if i == 0:
                continue          # (the first execution sizes the materialisation and allocates)
            r = q.report()
            line["launches"].append(int(r.num_kernels))
            line["wall_ms"].append(round(wall, 3)); line["execution_ms"].append(round(r.execution_time_ms, 3))
            line["kernel_ms"].append(round(r.kernel_time_ms, 3)); line["finalize_ms"].append(round(r.finalize_time_ms, 3))
            if hasattr(q, "order_limit_report"):
                rep = q.order_limit_report()
                for k in ("select_ms", "copy_ms", "tail_ms"):
                    line[k].append(round(rep[k], 3))
                line["report"] = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in rep.items()}
        res = q.result()
        line["result_rows"] = res.n_rows
        line["result_sha1"] = hashlib.sha1(res.text.encode("latin1")).hexdigest()
        print(json.dumps(line), flush=True)
        q.close()
    tab.close()
    ctx.close()


def main():
    sf = float(sys.argv[1]) if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else 1.0
    repeat = int(_arg("--repeat", "3"))
    if "--child" in sys.argv:
        setter = _arg("--setter", "none")
        measure(_arg("--tree", HERE), None if setter == "none" else int(setter), _arg("--label", "this"), sf, repeat)
        return 0
    parent = _arg("--parent-tree", None)
    if not parent or not os.path.isdir(os.path.join(parent, "resql_amd")):
        print("order_limit_timing: --parent-tree DIR (a built checkout of the parent commit) is required", file=sys.stderr)
        return 2
    limit = float(_arg("--limit-seconds", "400"))
    sha = _arg("--parent-commit", None)
    outs = {"this": _arg("--out", None), "parent": _arg("--parent-out", None)}
    lines = []
    for label, tree, setter in (("parent run 1", parent, None), ("this, setter 1", HERE, 1), ("this, setter 0", HERE, 0), ("parent run 2", parent, None)):
        cmd = [sys.executable, os.path.abspath(__file__), str(sf), "--child", "--tree", os.path.abspath(tree), "--label", label, "--repeat", str(repeat),
               "--setter", "none" if setter is None else str(setter)]
        try:          # (a fresh child process per configuration: this one never opens the GPU)
            pr = subprocess.run(cmd, timeout=limit, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            print(f"order_limit_timing: '{label}' ended after {limit:g} s", file=sys.stderr)
            return 124
        if pr.returncode != 0:          # nothing more is started on the device after a process that failed
            print(pr.stdout + pr.stderr, file=sys.stderr)
            return pr.returncode
        for text in pr.stdout.splitlines():
            if not text.startswith("{"):
                continue
            line = json.loads(text)
            if sha:
                line["parent_commit"] = sha
            lines.append(line)
            print(json.dumps(line), flush=True)
            path = outs["parent" if setter is None else "this"]
            if path:
                with open(path, "a") as f:
                    f.write(json.dumps(line) + "\n")

    def median(v):
        return sorted(v)[len(v) // 2]
    for name, _ in STATEMENTS:
        by = {l["label"]: l for l in lines if l["statement"] == name}
        p1, p2, dev, host = by["parent run 1"], by["parent run 2"], by["this, setter 1"], by["this, setter 0"]
        pm = [median(p1["execution_ms"]), median(p2["execution_ms"])]
        summary = {"statement": name, "summary": True, "parent_execution_ms": pm, "parent_spread_ms": round(abs(pm[0] - pm[1]), 3),
                   "setter_0_execution_ms": median(host["execution_ms"]), "setter_1_execution_ms": median(dev["execution_ms"]),
                   "setter_1_over_parent_ms": round(median(dev["execution_ms"]) - min(pm), 3),
                   "setter_1_path": dev["report"]["path"], "setter_1_fallback_reason": dev["report"]["fallback_reason"],
                   "setter_1_select_ms": median(dev["select_ms"]), "setter_1_copy_ms": median(dev["copy_ms"]),
                   "setter_0_launches": host["launches"][-1], "parent_launches": p1["launches"][-1], "setter_1_launches": dev["launches"][-1],
                   "same_answer": len({l["result_sha1"] for l in by.values()}) == 1}
        if sha:
            summary["parent_commit"] = sha
        print(json.dumps(summary), flush=True)
        if outs["this"]:
            with open(outs["this"], "a") as f:
                f.write(json.dumps(summary) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
