"""What an ORDER BY over a materialisation costs at SF1: the host's quicksort over all tuples (Context.set_order_sort(0)) against the
device ordering the rows (1) against the parent commit.  A development aid, not part of bench.py.
usage: python tools/order_sort_timing.py [SF] --parent-tree DIR [--parent-commit SHA] [--rounds K] [--repeat N] [--only a,b]
                                         [--out FILE] [--parent-out FILE] [--limit-seconds N]
DIR is a built checkout of the parent commit (one that has Context.set_order_sort runs under its setting 0).  Processes run one after the other on one device, the two
builds alternating, K rounds (default 1) of: the parent, this tree under setting 1, the parent, this tree under setting 0 (what a host
that never calls the setter runs) - and the parent once more at the end.  One setting per process: an execution on the host path takes
a second.  Each process generates lineitem and, per statement, executes twice unrecorded and N times (default 5) recorded:
  sorted      a projection of lineitem's first 12 columns with ORDER BY l_extendedprice desc, l_orderkey, l_linenumber and no LIMIT (6 M
              rows at SF1; the `sorted` statement of tools/result_pack_timing.py)
  filtered    the same behind l_shipdate < date '1994-01-01' (1.7 M rows)
  overflow    order by l_linenumber, l_extendedprice desc, l_orderkey limit 10 with Context.set_order_limit(1) too (the parent has that
              setter): a quarter of the rows share the first key's leading value, order_limit's selection overflows its capacity and
              the next path follows - the host's sort, or under setting 1 the device's
(ORDER BY l_orderkey, l_linenumber is not run: the table is generated in that order, and the reference's quicksort - the pivot from the
segment's end - is quadratic on sorted input.)  One JSON line per process and statement goes to FILE (this tree) or the parent's FILE:
[median, min, max] ms of execution and finalize and of the sort report's range / sort / pack / gather / copy, then the launches, the
report's key bits, words, passes and tied pairs, and a digest of the result tuples.  This tree's file ends with a summary line per
statement: the parent's spread (max - min over the samples of all its processes), setting 0's process medians against the median of
the parent's process medians plus that spread, setting 1's slowest sample against the parent's fastest, and the ratio of the medians.
Every process is ended after N seconds (default 900)."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMES = ("execution_ms", "finalize_ms", "range_ms", "sort_ms", "pack_ms", "gather_ms", "copy_ms")
NAMES = ["sorted", "filtered", "overflow"]


def _arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def statements(db):
    li = [c.name for c in db["lineitem"].columns if c.data is not None][:12]
    proj = "select " + ", ".join(li) + " from lineitem"
    keys = " order by l_extendedprice desc, l_orderkey, l_linenumber"
    return {"sorted": (proj + keys, 0),
            "filtered": (proj + " where l_shipdate < date '1994-01-01'" + keys, 0),
            "overflow": ("select l_orderkey, l_linenumber, l_extendedprice, l_shipdate from lineitem order by l_linenumber, l_extendedprice desc, l_orderkey limit 10", 1)}


def tuples_digest(ctx, q, P):
    """(rows, tuple size, sha1 of the result view's tuples, read where they lie)"""
    v = P.rsq_result_view()
    ctx._check(ctx._L.rsq_query_result(q.h, C.byref(v)))
    n = v.n_rows * v.tuple_size
    buf = (C.c_uint8 * n).from_address(C.addressof(v.tuples.contents)) if n else b""
    return v.n_rows, v.tuple_size, hashlib.sha1(memoryview(buf)).hexdigest()[:16]


def measure(tree, label, sf, repeat, only, setting):
    sys.path.insert(0, tree)
    from resql_amd import engine, plan as P, tpch_full
    db = {"lineitem": tpch_full.lineitem(sf)}
    ctx = engine.Context(device=0)
    has_setter = hasattr(ctx, "set_order_sort")
    table = ctx.table(db["lineitem"])
    for name, (sql, order_limit) in statements(db).items():
        if only and name not in only:
            continue
        ctx.set_order_limit(order_limit)
        if has_setter:
            ctx.set_order_sort(setting)
        q = ctx.sql_compile(sql, [table])
        q.await_kernels()          # (the specialised kernels, not the interpreter tier a cold code-object cache starts on)
        p = {k: [] for k in TIMES}
        for _ in range(2):          # unrecorded: the first execution sizes the materialisation and allocates
            q.execute()
        for _ in range(repeat):
            q.execute()
            r = q.report()
            p["execution_ms"].append(r.execution_time_ms); p["finalize_ms"].append(r.finalize_time_ms)
            p["launches"] = int(r.num_kernels)
            p["order_limit_fallback"] = q.order_limit_report()["fallback_reason"]
            if has_setter:
                rep = q.order_sort_report()
                for k in TIMES[2:]:
                    p[k].append(rep[k])
                for k in ("path", "fallback_reason", "key_bits", "total_bits", "words", "passes", "rows", "lead", "out_rows", "tied_pairs", "tuple_size"):
                    p[k] = rep[k]
        p["result_rows"], p["result_tuple_size"], p["tuples_sha1"] = tuples_digest(ctx, q, P)
        for k in TIMES:
            p[k] = [round(x, 3) for x in (sorted(p[k])[len(p[k]) // 2], min(p[k]), max(p[k]))] if p[k] else None
        print(json.dumps({"label": label, "statement": name, "sf": sf, "executions": repeat, "setting": "parent" if label.startswith("parent") or not has_setter else setting, "times": p}), flush=True)
        q.close()
    table.close()
    ctx.close()


def summarise(name, lines):
    mine = [l["times"] for l in lines if l["statement"] == name]
    parent = [l["times"] for l in lines if l["statement"] == name and l["setting"] == "parent"]
    zero = [l["times"] for l in lines if l["statement"] == name and l["setting"] == 0]
    one = [l["times"] for l in lines if l["statement"] == name and l["setting"] == 1]
    out = {"statement": name, "summary": True, "rows": one[0]["rows"], "out_rows": one[0]["out_rows"], "tuple_size": one[0]["tuple_size"],
           "key_bits": one[0]["key_bits"], "words": one[0]["words"], "passes": one[0]["passes"], "setting_1_path": one[0]["path"]}
    for key in ("execution_ms", "finalize_ms"):
        medians = sorted(p[key][0] for p in parent)
        spread = round(max(p[key][2] for p in parent) - min(p[key][1] for p in parent), 3)
        fastest_parent, slowest_one = min(p[key][1] for p in parent), max(p[key][2] for p in one)
        out[key] = {"parent_process_medians": [p[key][0] for p in parent], "parent_spread": spread, "parent_fastest_sample": fastest_parent,
                    "setting_0_process_medians": [p[key][0] for p in zero], "setting_1_process_medians": [p[key][0] for p in one],
                    "setting_1_slowest_sample": slowest_one,
                    "setting_1_slowest_below_parent_fastest": slowest_one < fastest_parent,
                    "setting_0_within_parent_spread": max(p[key][0] for p in zero) <= medians[len(medians) // 2] + spread,
                    "ratio_of_medians": round(medians[len(medians) // 2] / max(sorted(p[key][0] for p in one)[len(one) // 2], 1e-9), 1)}
    for k in TIMES[2:]:
        out[k] = [p[k][0] for p in one]
    out["launches"] = {"parent": parent[0]["launches"], "setting_0": zero[0]["launches"], "setting_1": one[0]["launches"]}
    out["same_answer"] = len({p["tuples_sha1"] for p in mine}) == 1
    return out


def main():
    sf = float(sys.argv[1]) if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else 1.0
    only = [s for s in _arg("--only", "").split(",") if s]
    if "--child" in sys.argv:
        measure(_arg("--tree", HERE), _arg("--label", "this"), sf, int(_arg("--repeat", "5")), only, int(_arg("--setting", "0")))
        return 0
    parent = _arg("--parent-tree", None)
    if not parent or not os.path.isdir(os.path.join(parent, "resql_amd")):
        print("order_sort_timing: --parent-tree DIR (a built checkout of the parent commit) is required", file=sys.stderr)
        return 2
    limit, sha = float(_arg("--limit-seconds", "900")), _arg("--parent-commit", None)
    rounds = int(_arg("--rounds", "1"))
    lines, runs = [], []
    for r in range(1, rounds + 1):
        runs += [(f"parent {2 * r - 1}", None, 0), (f"this {r}, setting 1", HERE, 1), (f"parent {2 * r}", None, 0), (f"this {r}, setting 0", HERE, 0)]
    runs.append((f"parent {2 * rounds + 1}", None, 0))

    def record(line, path):
        if sha:
            line["parent_commit"] = sha
        print(json.dumps(line), flush=True)
        if path:
            with open(path, "a") as f:
                f.write(json.dumps(line) + "\n")

    for label, tree, setting in runs:
        cmd = [sys.executable, os.path.abspath(__file__), str(sf), "--child", "--tree", os.path.abspath(tree or parent), "--label", label,
               "--setting", str(setting), "--repeat", _arg("--repeat", "5"), "--only", ",".join(only or NAMES)]
        try:          # (a fresh child process per run: this one never opens the GPU)
            pr = subprocess.run(cmd, timeout=limit, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            print(f"order_sort_timing: '{label}' ended after {limit:g} s", file=sys.stderr)
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
