"""BULK INSERT timed: the host parse (mode 1, 16 threads) against the device parse (mode 2) of the same '.tbl' files on the same box.
Writes lineitem and orders with tests/tpch_dbgen.py into a temporary directory (text-pool columns hold a filler of dbgen's mean
comment length), loads each file twice per mode and keeps the second load (page cache warm), and appends one line per (table, mode)
to profiles/tbl_device_ingest_sf1.jsonl: the report's phases, the three kernels' HIP-event times with their text GB/s, and the floor of
the device path, max(file read, text bytes / 63 GB/s).  Every load runs in a child process under its own time limit; the first one
that fails ends the run.  Never part of bench.py's `value`.

    python tools/tbl_ingest_bench.py [--sf 1.0] [--out profiles/tbl_device_ingest_sf1.jsonl] [--limit 300]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LINK_GBPS = 63.0          # host-to-device link of the MI355X box
FILLER = {"lineitem": "x" * 27, "orders": "x" * 49}          # mean length of dbgen's l_comment / o_comment


def child(table: str, path: str, mode: int) -> None:
    from resql_amd import engine, plan as P, tpch
    schema = P.Table(table, [P.Column(n, t) for n, t in {"lineitem": tpch.LINEITEM_SCHEMA, "orders": tpch.ORDERS_SCHEMA}[table]], 0)
    ctx = engine.Context(device=0)
    try:
        rep = None
        for _ in range(2):
            t = ctx.load_tbl(schema, path, threads=16, mode=mode)
            rep = t.load_report
            t.close()
    finally:
        ctx.close()
    gb = rep["text_bytes"] / 1e9
    out = {"table": table, "mode": mode, "threads": 16 if mode == 1 else 0, **rep}
    if rep["path"] == 1:
        for k in ("count", "starts", "parse"):
            out[f"{k}_kernel_gbps"] = gb / (rep[f"{k}_kernel_ms"] / 1e3) if rep[f"{k}_kernel_ms"] > 0 else 0.0
        out["link_floor_ms"] = gb / LINK_GBPS * 1e3
        out["floor_ms"] = max(rep["read_ms"], out["link_floor_ms"])
    print("RESULT " + json.dumps(out), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sf", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tbl_device_ingest_sf1.jsonl"))
    ap.add_argument("--limit", type=int, default=300, help="seconds per load step")
    ap.add_argument("--child", nargs=3, metavar=("TABLE", "PATH", "MODE"))
    a = ap.parse_args()
    if a.child:
        child(a.child[0], a.child[1], int(a.child[2]))
        return 0
    import tpch_dbgen
    with tempfile.TemporaryDirectory() as d:
        tabs = tpch_dbgen.Tables(a.sf)
        for table in ("lineitem", "orders"):
            with open(os.path.join(d, table + ".tbl"), "w") as f:
                for line in tabs.tbl_lines(table, FILLER[table]):
                    f.write(line + "\n")
        del tabs
        lines = []
        for table in ("lineitem", "orders"):
            for mode in (1, 2):
                pr = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", table,
                                     os.path.join(d, table + ".tbl"), str(mode)], capture_output=True, text=True)
                got = [l[7:] for l in pr.stdout.splitlines() if l.startswith("RESULT ")]
                if pr.returncode != 0 or not got:
                    print(f"{table} mode {mode}: the load ended with status {pr.returncode}; nothing more is started\n{pr.stdout}{pr.stderr}")
                    return 1
                rec = json.loads(got[0])
                rec["sf"] = a.sf
                lines.append(rec)
                print(json.dumps(rec), flush=True)
    with open(a.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
