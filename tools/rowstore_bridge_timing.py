"""What the row-store bridge costs a drop-in host: rsq_table_from_rowstore_ex over a ReSQL row store of lineitem and orders, transposed
by the host path (mode 1: one thread, pageable upload - the default) and by the device path (mode 2: resql_amd/csrc/rowstore_device.hip),
in one process.  A development aid, not part of bench.py.
usage: python tools/rowstore_bridge_timing.py [SF] [--runs N] [--limit-seconds N] [--out FILE]
The tables are tpch_full's lineitem and orders with every column of the schema (columns no generator fills - comments, clerks - take
phrases from a small seeded dictionary), packed into 2 MiB blocks (tests/rowstorecases.py pack).  Each mode runs N times (default 3),
host and device in turn; one JSON line per run with the phases of rsq_rowstore_report and the time the call spent in the driver's
allocation calls (columns, and pinned slabs the first time), appended to FILE when given, and one summary
line per table:
  total_ms of the device path against the host path's, from the same process (the yardstick: the host path is unchanged code)
  kernel_ms against (tuple bytes + column bytes) / the read bandwidth rsq_measure_read_bandwidth reports (recorded, not asserted)
The device columns are compared with the host's byte for byte.  The measurement runs in a child process that is ended after N seconds
(default 900)."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BLOCK_BYTES = 2 << 20


def _arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def _fill(table, seed):
    """every column of the schema with data: the ones without a generator get phrases of a 1024-entry dictionary"""
    import numpy as np
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz    ", dtype=np.uint8)
    for c in table.columns:
        if c.data is not None:
            continue
        ln = c.type.len
        if c.type.width != ln or ln < 2:          # (a number or a single byte)
            c.data = rng.integers(1, 100, size=table.n_rows).astype(c.type.np_dtype)
            continue
        phrases = np.zeros((1024, ln), dtype=np.uint8)
        for p in phrases:
            k = int(rng.integers(ln // 3, ln + 1))
            p[:k] = letters[rng.integers(0, len(letters), size=k)]
        c.data = phrases.view(f"S{ln}").reshape(1024)[rng.integers(0, 1024, size=table.n_rows)]
    return table


def measure(sf, runs, out_path):
    import numpy as np
    from resql_amd import engine, tpch_full
    import rowstorecases as R
    ctx = engine.Context(device=0)
    gbps = ctx.read_bandwidth()
    print(f"# read bandwidth {gbps:.0f} GB/s", flush=True)

    def driver():          # ms the context has spent in the driver's allocation calls so far, and its pinned slabs
        m = engine.rsq_memory_stats(C.sizeof(engine.rsq_memory_stats))
        ctx._check(ctx._L.rsq_ctx_memory_stats(ctx.h, C.byref(m)))
        return m.driver_ms, m.pinned_slab_bytes

    def emit(line):
        print(json.dumps(line), flush=True)
        if out_path:
            with open(out_path, "a") as f:
                f.write(json.dumps(line) + "\n")

    for make in (tpch_full.lineitem, tpch_full.orders):
        t0 = time.time()
        table = _fill(make(sf), 17)
        blocks = R.pack(table, [c.data for c in table.columns], block_bytes=BLOCK_BYTES, junk=False)
        ts = R.tuple_size(table)
        column_bytes = table.n_rows * sum(c.type.width for c in table.columns)
        print(f"# {table.name}: {table.n_rows} rows of {ts} bytes in {len(blocks)} blocks, packed in {time.time() - t0:.1f} s", flush=True)
        want = None
        totals = {"host": [], "device": []}
        kernels = []
        for run in range(runs):
            for name, mode in (("host", engine.ROWSTORE_HOST), ("device", engine.ROWSTORE_DEVICE)):
                d0, p0 = driver()
                t0 = time.time()
                dt = ctx.from_rowstore(table, blocks, mode=mode)
                wall = (time.time() - t0) * 1e3
                d1, p1 = driver()
                rep = dt.bridge_report
                line = {"table": table.name, "sf": sf, "mode": name, "run": run, "wall_ms": round(wall, 3), "driver_alloc_ms": round(d1 - d0, 3),
                        "pinned_slab_growth_bytes": p1 - p0}
                line.update({k: (round(v, 3) if isinstance(v, float) else v) for k, v in rep.items()})
                if run == 0:          # the columns, once: the host's are the yardstick
                    got = R.columns_of(dt, table)
                    if name == "host":
                        want = got
                    else:
                        line["equal"] = got == want
                    del got
                emit(line)
                totals[name].append(rep["total_ms"])
                if name == "device":
                    kernels.append(rep["kernel_ms"])
                dt.close()
        floor_ms = (table.n_rows * ts + column_bytes) / (gbps * 1e9) * 1e3
        emit({"table": table.name, "sf": sf, "summary": True, "rows": table.n_rows, "tuple_bytes": table.n_rows * ts, "column_bytes": column_bytes,
              "host_total_ms": round(float(np.median(totals["host"])), 3), "device_total_ms": round(float(np.median(totals["device"])), 3),
              "device_over_host": round(float(np.median(totals["device"]) / np.median(totals["host"])), 4),
              "kernel_ms": round(float(np.median(kernels)), 3), "read_bandwidth_gbps": round(gbps, 1), "kernel_floor_ms": round(floor_ms, 3),
              "kernel_over_floor": round(float(np.median(kernels)) / floor_ms, 2)})
        del blocks, table, want
    ctx.close()


if __name__ == "__main__":
    sf = float(sys.argv[1]) if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else 1.0
    if "--child" in sys.argv:
        measure(sf, int(_arg("--runs", "3")), _arg("--out", None))
        sys.exit(0)
    limit = float(_arg("--limit-seconds", "900"))
    try:          # (a fresh child process: this one never opens the GPU)
        sys.exit(subprocess.run([sys.executable, os.path.abspath(__file__)] + sys.argv[1:] + ["--child"], timeout=limit).returncode)
    except subprocess.TimeoutExpired:
        print(f"rowstore_bridge_timing: ended after {limit:g} s", file=sys.stderr)
        sys.exit(124)
