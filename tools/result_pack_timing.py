"""What a SELECT without an aggregation costs from scan to result tuples (and on to '.tbl' text) at SF1: the host packing its tuples
(Context.set_result_pack(0)) against the device packing them (1) against the parent commit.  A development aid, not part of bench.py.
usage: python tools/result_pack_timing.py [SF] --parent-tree DIR [--parent-commit SHA] [--rounds K] [--once a,b] [--repeat N] [--only a,b]
                                          [--out FILE] [--parent-out FILE] [--limit-seconds N]
DIR is a built checkout of the parent commit (one that has Context.set_result_pack runs under its setting 0).  Processes run one after the other on one device, the
two builds alternating, K rounds (default 1) of: the parent, this tree with the two settings alternating on one compiled query, the
parent, this tree under setting 0 alone (what a host that never calls the setter runs) - and the parent once more at the end.  The
host path's time depends on the process (where its pageable buffers lie), so the parent's spread is taken over all its processes.
Statements named by --once are measured in the first round only.  Each process generates lineitem and orders and, per statement,
executes twice per setting unrecorded and N times (default 10) recorded:
  lineitem    a projection of lineitem's first 12 columns, no LIMIT (6 M rows at SF1; the statement of profiles/result_text_sf1.jsonl)
  filtered    the same behind l_shipdate < date '1994-01-01' (1.7 M rows)
  orders      a projection of every column of orders
  sorted      `lineitem` with ORDER BY l_extendedprice desc, l_orderkey, l_linenumber and no LIMIT: the reference's quicksort over all
              6 M tuples on the host, either way.  (ORDER BY l_orderkey, l_linenumber is not run: the table is generated in that order, and the reference's quicksort - the pivot from
              the segment's end - is quadratic on sorted input, on either path and on the parent.)
then the same over execute + rsq_query_result_write(mode 2) into /dev/null as a whole.  One JSON line per process and statement goes to
FILE (this tree) or the parent's FILE: per setting [median, min, max] ms of execution, finalize, the pack report's kernel / copy / sort,
execute-plus-text and the text's upload, then launches, tuples_from_device and a digest of the result tuples.  This tree's file ends
with a summary line per statement: the medians of every process, the parent's spread (max - min over the samples of all its
processes), setting 1's slowest process against the parent's fastest minus that spread, setting 0's processes against the range of the
parent's process medians and against their median plus that spread.  Every process is ended after N seconds (default 900)."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMES = ("execution_ms", "finalize_ms", "kernel_ms", "copy_ms", "sort_ms", "execute_and_text_ms", "text_upload_ms")


def _arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def statements(db):
    li = [c.name for c in db["lineitem"].columns if c.data is not None][:12]
    od = [c.name for c in db["orders"].columns if c.data is not None]
    proj = "select " + ", ".join(li) + " from lineitem"
    return {"lineitem": (proj, "lineitem"),
            "filtered": (proj + " where l_shipdate < date '1994-01-01'", "lineitem"),
            "orders": ("select " + ", ".join(od) + " from orders", "orders"),
            "sorted": (proj + " order by l_extendedprice desc, l_orderkey, l_linenumber", "lineitem")}


def tuples_digest(ctx, q, P):
    """(rows, tuple size, sha1 of the result view's tuples, read where they lie)"""
    v = P.rsq_result_view()
    ctx._check(ctx._L.rsq_query_result(q.h, C.byref(v)))
    n = v.n_rows * v.tuple_size
    buf = (C.c_uint8 * n).from_address(C.addressof(v.tuples.contents)) if n else b""
    return v.n_rows, v.tuple_size, hashlib.sha1(memoryview(buf)).hexdigest()[:16]


def measure(tree, label, sf, repeat, only, want):
    sys.path.insert(0, tree)
    from resql_amd import engine, plan as P, tpch_full
    db = {"lineitem": tpch_full.lineitem(sf), "orders": tpch_full.orders(sf)}
    ctx = engine.Context(device=0)
    has_setter = hasattr(ctx, "set_result_pack")
    settings = [int(s) for s in want] if has_setter else [None]
    tabs = {k: ctx.table(t) for k, t in db.items()}

    def execute(q, s):
        if has_setter:
            ctx.set_result_pack(s)
        q.execute()

    for name, (sql, table) in statements(db).items():
        if only and name not in only:
            continue
        n = repeat
        q = ctx.sql_compile(sql, [tabs[table]])
        q.await_kernels()          # (the specialised kernels, not the interpreter tier a cold code-object cache starts on)
        per = {s: {k: [] for k in TIMES} for s in settings}
        for s in settings * 2:          # unrecorded: the first execution sizes the materialisation and allocates
            execute(q, s)
        for s in settings * n:
            execute(q, s)
            r, p = q.report(), per[s]
            p["execution_ms"].append(r.execution_time_ms); p["finalize_ms"].append(r.finalize_time_ms)
            p["launches"] = int(r.num_kernels)
            if has_setter:
                rep = q.result_pack_report()
                for k in ("kernel_ms", "copy_ms", "sort_ms"):
                    p[k].append(rep[k])
                p["path"], p["fallback_reason"], p["sorted_on_host"] = rep["path"], rep["fallback_reason"], rep["sorted_on_host"]
        for s in settings:          # the answer under each setting, once, outside the timed executions
            execute(q, s)
            per[s]["rows"], per[s]["tuple_size"], per[s]["tuples_sha1"] = tuples_digest(ctx, q, P)
        for s in settings * n:
            t0 = time.perf_counter()
            execute(q, s)
            rep = q.write_result_text("/dev/null", mode=engine.TEXT_DEVICE)
            per[s]["execute_and_text_ms"].append((time.perf_counter() - t0) * 1e3)
            per[s]["text_upload_ms"].append(rep["upload_ms"])
            per[s]["tuples_from_device"] = rep["tuples_from_device"]
        for p in per.values():
            for k in TIMES:
                p[k] = [round(x, 3) for x in (sorted(p[k])[len(p[k]) // 2], min(p[k]), max(p[k]))] if p[k] else None
        print(json.dumps({"label": label, "statement": name, "sf": sf, "executions_per_setting": n,
                          "settings": {("parent" if s is None else str(s)): per[s] for s in settings}}), flush=True)
        q.close()
    for t in tabs.values():
        t.close()
    ctx.close()


def summarise(name, lines):
    mine = [l for l in lines if l["statement"] == name]
    parent = [l["settings"].get("parent") or l["settings"]["0"] for l in mine if l["label"].startswith("parent")]
    zero = [l["settings"]["0"] for l in mine if not l["label"].startswith("parent")]
    one = [l["settings"]["1"] for l in mine if "1" in l["settings"]]
    out = {"statement": name, "summary": True, "rows": one[0]["rows"], "tuple_size": one[0]["tuple_size"]}
    for key in ("execution_ms", "finalize_ms", "execute_and_text_ms"):
        medians = sorted(p[key][0] for p in parent)
        spread = round(max(p[key][2] for p in parent) - min(p[key][1] for p in parent), 3)
        out[key] = {"parent_process_medians": [p[key][0] for p in parent], "parent_spread": spread,
                    "setting_0_process_medians": [p[key][0] for p in zero], "setting_1_process_medians": [p[key][0] for p in one],
                    "setting_1_faster_than_parent_beyond_its_spread": max(p[key][0] for p in one) < medians[0] - spread,
                    "setting_0_within_range_of_parent_medians": max(p[key][0] for p in zero) <= medians[-1],
                    "setting_0_within_parent_spread": max(p[key][0] for p in zero) <= medians[len(medians) // 2] + spread}
    out["launches"] = {"parent": parent[0]["launches"], "setting_0": zero[0]["launches"], "setting_1": one[0]["launches"]}
    out["same_answer"] = len({p["tuples_sha1"] for p in parent + zero + one}) == 1
    return out


def main():
    sf = float(sys.argv[1]) if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else 1.0
    only = [s for s in _arg("--only", "").split(",") if s]
    if "--child" in sys.argv:
        measure(_arg("--tree", HERE), _arg("--label", "this"), sf, int(_arg("--repeat", "10")), only, _arg("--settings", "0,1").split(","))
        return 0
    parent = _arg("--parent-tree", None)
    if not parent or not os.path.isdir(os.path.join(parent, "resql_amd")):
        print("result_pack_timing: --parent-tree DIR (a built checkout of the parent commit) is required", file=sys.stderr)
        return 2
    limit, sha = float(_arg("--limit-seconds", "900")), _arg("--parent-commit", None)
    rounds, once = int(_arg("--rounds", "1")), [s for s in _arg("--once", "").split(",") if s]
    lines, runs = [], []
    for r in range(1, rounds + 1):
        runs += [(f"parent {2 * r - 1}", None, "0", r), (f"this {r}, settings alternating", HERE, "0,1", r), (f"parent {2 * r}", None, "0", r),
                 (f"this {r}, setting 0 alone", HERE, "0", r)]
    runs.append((f"parent {2 * rounds + 1}", None, "0", rounds))

    def record(line, path):
        if sha:
            line["parent_commit"] = sha
        print(json.dumps(line), flush=True)
        if path:
            with open(path, "a") as f:
                f.write(json.dumps(line) + "\n")

    for label, tree, settings, r in runs:
        names = [n for n in (only or ["lineitem", "filtered", "orders", "sorted"]) if r == 1 or n not in once]
        cmd = [sys.executable, os.path.abspath(__file__), str(sf), "--child", "--tree", os.path.abspath(tree or parent), "--label", label,
               "--settings", settings, "--repeat", _arg("--repeat", "10"), "--only", ",".join(names)]
        try:          # (a fresh child process per run: this one never opens the GPU)
            pr = subprocess.run(cmd, timeout=limit, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            print(f"result_pack_timing: '{label}' ended after {limit:g} s", file=sys.stderr)
            return 124
        if pr.returncode != 0:          # nothing more is started on the device after a process that failed
            print(pr.stdout, file=sys.stderr)
            return pr.returncode
        for text in pr.stdout.splitlines():
            if text.startswith("{"):
                lines.append(json.loads(text))
                record(lines[-1], _arg("--out", None) if tree else _arg("--parent-out", None))
    for name in dict.fromkeys(l["statement"] for l in lines):
        record(summarise(name, lines), _arg("--out", None))
    return 0


if __name__ == "__main__":
    sys.exit(main())
