"""What a large result costs on its way to '.tbl' text: the host path (serializeResultView, one thread) against the device path
(resql_amd/csrc/result_text.hip) on the same executed statement.  A development aid beside tools/sql_bench.py, not part of bench.py.
usage: python tools/result_text_bench.py [SF] [--limit-seconds N] [--out FILE]
Two statements over tpch_full.database(SF): a projection of lineitem's columns without LIMIT (6 M rows at SF1) and Q18's derived
aggregation materialised (tests/derivedcases.py having_hash_key with a threshold every group passes: 1.5 M groups at SF1).  Each is
executed once; then the host text (mode 1) and the device text (mode 2) are timed once each and compared.  One JSON line per
statement, appended to FILE when given.  The measurement runs in a child process that is ended after N seconds (default 600)."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def measure(sf, out_path):
    from resql_amd import engine, plan as P, tpch_full
    import derivedcases
    t0 = time.time()
    db = tpch_full.database(sf, fill_unused=sf < 1.0)
    names = sorted(db)
    print(f"# generated SF{sf:g} in {time.time() - t0:.1f} s", flush=True)
    ctx = engine.Context(device=0)
    tabs = {k: ctx.table(db[k]) for k in names}
    cols = [c.name for c in db["lineitem"].columns if c.data is not None][:12]
    statements = [("lineitem_projection", "select " + ", ".join(cols) + " from lineitem", None),
                  ("q18_derived_groups", None, derivedcases.having_hash_key(db, threshold=0))]
    for name, sql, plan in statements:
        q = ctx.sql_compile(sql, [tabs[k] for k in names]) if sql else ctx.compile(plan, [tabs[t.name] for t in plan.tables])
        q.execute()
        v = P.rsq_result_view()
        ctx._check(ctx._L.rsq_query_result(q.h, C.byref(v)))
        rows, tuple_size = v.n_rows, v.tuple_size
        t0 = time.time()
        want, host_rep = q.result_text(mode=engine.TEXT_HOST)
        host_wall = (time.time() - t0) * 1e3
        t0 = time.time()
        got, rep = q.result_text(mode=engine.TEXT_DEVICE)
        dev_wall = (time.time() - t0) * 1e3
        groups = (rows + 255) // 256
        line = {"statement": name, "sf": sf, "rows": rows, "tuple_size": tuple_size, "text_bytes": len(want),
                "host_ms": round(host_rep["total_ms"], 3), "host_wall_ms": round(host_wall, 3),
                "device_path": rep["path"], "fallback_reason": rep["fallback_reason"], "tuples_from_device": rep["tuples_from_device"],
                "chunks": rep["chunks"], "upload_ms": round(rep["upload_ms"], 3), "kernel_ms": round(rep["kernel_ms"], 3),
                "download_ms": round(rep["download_ms"], 3), "device_ms": round(rep["total_ms"], 3), "device_wall_ms": round(dev_wall, 3),
                # what the two kernels move: both read the tuples; the first writes a length per row and a total per workgroup, the second
                # reads them back (with the workgroups' offsets) and writes the text
                "kernel_bytes_read": 2 * rows * tuple_size + rows * 4 + groups * 8, "kernel_bytes_written": len(want) + rows * 4 + groups * 4,
                "equal": got == want}
        print(json.dumps(line), flush=True)
        if out_path:
            with open(out_path, "a") as f:
                f.write(json.dumps(line) + "\n")
        q.close()
    for t in tabs.values():
        t.close()
    ctx.close()


if __name__ == "__main__":
    sf = float(sys.argv[1]) if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else 1.0
    if "--child" in sys.argv:
        measure(sf, _arg("--out", None))
        sys.exit(0)
    limit = float(_arg("--limit-seconds", "600"))
    try:          # (a fresh child process: this one never opens the GPU)
        sys.exit(subprocess.run([sys.executable, os.path.abspath(__file__)] + sys.argv[1:] + ["--child"], timeout=limit).returncode)
    except subprocess.TimeoutExpired:
        print(f"result_text_bench: ended after {limit:g} s", file=sys.stderr)
        sys.exit(124)
