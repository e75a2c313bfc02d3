#!/bin/bash
# Collect the per-round profile artefacts on the GPU box (run through gpurun from the repo root):
#   bench line, rocprofv3 kernel statistics of the same command, separate --pmc passes (FETCH_SIZE; WRITE_SIZE), TPC-H Q3 per pipeline.
# rocprofv3 is run from /tmp with TMPDIR=/tmp (it hangs when started inside the repo snapshot); the profiled program stands
# directly behind `--`; every step runs under a hard timeout and a failed step is reported and skipped, not built upon.
# usage: bash tools/collect_profiles.sh rNN
set -u
R=${1:-r03}
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$ROOT/gpurun_out/profiles
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp

step() { echo "== $*"; }
# the commit the files were collected at goes INTO every file (HEAD_SHA from the caller: the GPU box has no .git)
stamp_all() { [ -n "${HEAD_SHA:-}" ] && python3 "$ROOT/tools/stamp_profiles.py" "$OUT" "$R" "$HEAD_SHA"; }
found() {   # found DIR PATTERN -> path of the first match, or empty (and a message)
    local f; f=$(find "$1" -name "$2" 2>/dev/null | head -n 1)
    if [ -z "$f" ]; then echo "   (no $2 under $1: step skipped)" >&2; fi
    echo "$f"
}

# PART=a (default): bench, Q1 / Q3 / large-group kernel statistics and PMC passes; PART=b: end-to-end tables (config 5, SQL at SF1 / SF10,
# cold compile latencies, shard tails, late-load traffic, the C-ABI path); PART=c: the join statements one by one (kernel statistics + a FETCH_SIZE
# pass each).  Each part fits one gpurun call.  HEAD_SHA=<commit> in the environment is written into every file collected.
PART=${PART:-a}
if [ "$PART" = "c" ]; then
step "the join statements at SF10, one by one: kernel statistics and one FETCH_SIZE pass each"
for qn in q5 q10 q12 q19; do
    rm -rf /tmp/prof_j_$qn /tmp/prof_jp_$qn
    timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_j_$qn -- python3 "$ROOT/tools/sql_bench.py" 10 --repeat 6 --only $qn > /tmp/j_$qn.log 2>&1
    f=$(found /tmp/prof_j_$qn '*kernel_stats.csv'); [ -n "$f" ] && cp "$f" "$OUT/${R}_${qn}_sf10_kernel_stats.csv"
    timeout -k 10 200 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d /tmp/prof_jp_$qn -- python3 "$ROOT/tools/sql_bench.py" 10 --repeat 3 --only $qn > /tmp/jp_$qn.log 2>&1
done
python3 - "$OUT/${R}_joins_sf10_pmc.json" <<'PY'
import csv, glob, json, sys
out = {"note": "FETCH_SIZE per dispatch (KB as rocprofv3 reports them; gfx950 counts 1/2 of the bytes of wide coalesced streaming reads, MI355X_MICROARCH.md): "
               "the LARGEST dispatch of each kernel name per statement (sizing passes share a name with the build they size); average duration from the "
               "separate --kernel-trace --stats run of the same command", "statements": {}}
for qn in ("q5", "q10", "q12", "q19"):
    fs = glob.glob(f"/tmp/prof_jp_{qn}/*/*counter_collection.csv"); ks = glob.glob(f"/tmp/prof_j_{qn}/*/*kernel_stats.csv")
    e = {}
    if fs:
        per = {}
        for r in csv.DictReader(open(fs[0])):
            k = r["Kernel_Name"].split("(")[0]
            if r["Counter_Name"] != "FETCH_SIZE" or not (k.startswith("rsq_p") or "k_rank" in k or "k_compact" in k or "k_topk" in k or "k_scan" in k): continue
            per.setdefault(k, {}); per[k][r["Dispatch_Id"]] = per[k].get(r["Dispatch_Id"], 0.0) + float(r["Counter_Value"])
        for k, d in per.items(): e.setdefault(k, {})["FETCH_SIZE_KB"] = round(max(d.values()), 1)
    if ks:
        for r in csv.DictReader(open(ks[0])):
            k = r["Name"].split("(")[0]
            if k in e: e[k]["avg_us"] = round(float(r["AverageNs"]) / 1e3, 1); e[k]["calls"] = int(r["Calls"])
    out["statements"][qn] = e
json.dump(out, open(sys.argv[1], "w"), indent=1)
print("   join statements:", {q: len(v) for q, v in out["statements"].items()})
PY
step "compile latency with the kernels compiled in process, and at SF10 with the interpreter's execution time beside the specialised one"
AMD_COMGR_CACHE=0 RSQ_GENERIC=1 RSQ_COMPILE_HELPERS=0 timeout -k 10 300 python3 "$ROOT/tools/compile_latency.py" 1 2>/dev/null | grep '^{' > "$OUT/${R}_compile_latency_in_process.jsonl"
AMD_COMGR_CACHE=0 RSQ_GENERIC=1 timeout -k 10 300 python3 "$ROOT/tools/compile_latency.py" 10 2>/dev/null | grep '^{' > "$OUT/${R}_compile_latency_sf10.jsonl"
step "an empty code-object cache: interpreter -> quick tier -> full kernels, per statement (SF1 and SF10)"
# (AMD_COMGR_CACHE=0: the compiler's own per-user cache of compiled programs would answer for hiprtc after the first collection step that compiled
# the same texts - these steps measure a statement NOBODY has compiled before)
AMD_COMGR_CACHE=0 RSQ_GENERIC=1 timeout -k 10 300 python3 "$ROOT/tools/tier_latency.py" 1 2>/dev/null | grep '^{' > "$OUT/${R}_kernel_tiers_sf1.jsonl"
AMD_COMGR_CACHE=0 RSQ_GENERIC=1 timeout -k 10 300 python3 "$ROOT/tools/tier_latency.py" 10 --only q3,q5,q10,q12,q19 2>/dev/null | grep '^{' > "$OUT/${R}_kernel_tiers_sf10.jsonl"
step "group rows of a hash aggregation: the tail on the device against the host's"
timeout -k 10 200 python3 "$ROOT/tools/hash_tail_bench.py" > "$OUT/${R}_hash_tail_device_vs_host.txt" 2>/dev/null
timeout -k 10 200 python3 "$ROOT/tools/hash_tail_bench.py" 100000000 262144 >> "$OUT/${R}_hash_tail_device_vs_host.txt" 2>/dev/null
ls -la "$OUT" | tail -n 12
stamp_all
exit 0
fi
if [ "$PART" = "b" ]; then
step "TPC-H Q3 at SF10 WITHOUT the profiler (what README / DESIGN quote)"
timeout -k 10 200 python3 "$ROOT/tools/profile_case.py" q3 10 16 2>/dev/null | grep '^q3 ' > "$OUT/${R}_q3_sf10_runs_noprofiler.txt"
step "one 1.25 B-row shard, 2^20 groups, end to end: cold and warm executions of ONE query (10 % and 50 %, reference emission order and 'any')"
for s in 0.1 0.5; do
    timeout -k 10 120 python3 "$ROOT/tools/shard_tail.py" 20 $s 2>/dev/null | grep '^execution' > "$OUT/${R}_shard_g20_sel${s}_end_to_end.txt"
done
timeout -k 10 120 python3 "$ROOT/tools/shard_tail.py" 20 0.1 1250000000 any 2>/dev/null | grep '^execution' > "$OUT/${R}_shard_g20_sel0.1_end_to_end_emit_any.txt"
step "BASELINE config 5: 10 B rows as 8 shards, kernel and end-to-end"
timeout -k 10 500 python3 "$ROOT/tools/synthetic_10b.py" --out "gpurun_out/profiles/${R}_synthetic_10b.json" > "$OUT/${R}_synthetic_10b.log" 2>&1
step "late loads: FETCH_SIZE of the scan kernel at 1 % selectivity (1.25 B rows, G = 8) and of TPC-H Q6 at SF10: the traffic-based fraction"
for w in "synthetic 1250000000 8 0.01 4" "q6 10 4"; do
    tag=$(echo $w | cut -d' ' -f1)
    rm -rf /tmp/prof_ll_$tag /tmp/prof_ll_ks_$tag
    timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_ll_ks_$tag -- python3 "$ROOT/tools/profile_case.py" $w > /tmp/ll_ks.log 2>&1
    timeout -k 10 200 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d /tmp/prof_ll_$tag -- python3 "$ROOT/tools/profile_case.py" $w > /tmp/ll_pmc.log 2>&1
done
python3 - "$OUT/${R}_late_loads_pmc.json" <<'PY'
import csv, glob, json, sys
out = {"note": "late loads skip most cache lines of the columns behind a selective leading selection: algorithmic bytes / time then exceeds the HBM peak and is "
               "NOT a roofline fraction.  traffic_frac = FETCH_SIZE (x2: gfx950 reports half of wide streaming reads, MI355X_MICROARCH.md) / kernel time / 8 TB/s; "
               "FETCH_SIZE and the kernel time come from separate rocprofv3 runs of the same command", "cases": {}}
for tag, rows, bpr in (("synthetic", 1250000000, 32), ("q6", 59999996, 28)):
    fs = glob.glob(f"/tmp/prof_ll_{tag}/*/*counter_collection.csv"); ks = glob.glob(f"/tmp/prof_ll_ks_{tag}/*/*kernel_stats.csv")
    if not fs or not ks: continue
    per = {}
    for r in csv.DictReader(open(fs[0])):
        if r["Counter_Name"] == "FETCH_SIZE" and r["Kernel_Name"].startswith("rsq_p0"): per[r["Dispatch_Id"]] = per.get(r["Dispatch_Id"], 0.0) + float(r["Counter_Value"])
    kb = max(per.values()) if per else 0
    avg_ns = [float(r["AverageNs"]) for r in csv.DictReader(open(ks[0])) if r["Name"].startswith("rsq_p0")]
    if not avg_ns or not kb: continue
    t = min(avg_ns) * 1e-9
    out["cases"][tag] = {"rows": rows, "algorithmic_bytes": rows * bpr, "kernel_us": round(t * 1e6, 1), "FETCH_SIZE_KB": round(kb, 1),
                         "hbm_read_bytes_corrected": round(kb * 1024 * 2), "algorithmic_frac_of_8TBps": round(rows * bpr / t / 8e12, 3),
                         "traffic_frac_of_8TBps": round(kb * 1024 * 2 / t / 8e12, 3)}
json.dump(out, open(sys.argv[1], "w"), indent=1)
print("   late loads:", {k: (v["algorithmic_frac_of_8TBps"], v["traffic_frac_of_8TBps"]) for k, v in out["cases"].items()})
PY
step "the reference's eight TPC-H statements from SQL text at SF1 (with the reference beside them) and at SF10 (answers checked against the reference's goldens)"
timeout -k 10 300 python3 "$ROOT/tools/sql_bench.py" 1 --reference 2>/dev/null | grep '^{' > "$OUT/${R}_sql_sf1.jsonl"
timeout -k 10 300 python3 "$ROOT/tools/sql_bench.py" 10 2>/dev/null | grep '^{' > "$OUT/${R}_sql_sf10.jsonl"
rm -rf /tmp/prof_sql
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_sql -- python3 "$ROOT/tools/sql_bench.py" 10 --repeat 5 --only q5,q10,q12,q14,q19 > /tmp/sqlp.log 2>&1
f=$(found /tmp/prof_sql '*kernel_stats.csv'); [ -n "$f" ] && cp "$f" "$OUT/${R}_sql_sf10_kernel_stats.csv"
step "compile latency, cold and warm (empty code-object cache)"
AMD_COMGR_CACHE=0 RSQ_GENERIC=1 timeout -k 10 300 python3 "$ROOT/tools/compile_latency.py" 1 2>/dev/null | grep '^{' > "$OUT/${R}_compile_latency.jsonl"
step "compile -> ONE execution -> delete, per statement: first-ever, fresh queries (plan memo + arenas), steady; and the same with both switched off"
timeout -k 10 300 python3 "$ROOT/tools/first_exec.py" 10 2>/dev/null | grep -E '^\{|^# \{' > "$OUT/${R}_first_exec_sf10.jsonl"
timeout -k 10 300 python3 "$ROOT/tools/first_exec.py" 10 --driver-alloc --no-memo 2>/dev/null | grep -E '^\{|^# \{' > "$OUT/${R}_first_exec_sf10_driver_alloc_no_memo.jsonl"
step "what 5 GB of line stores cost beside a 40 GB streaming read (the staged partitioning's write side, DESIGN §4)"
if hipcc -O3 --offload-arch=gfx950 -o /tmp/store_rate "$ROOT/tools/exp/store_rate.hip" 2>/dev/null; then timeout -k 10 200 /tmp/store_rate > "$OUT/${R}_store_rate.txt" 2>&1; fi
step "does a shard's tail overlap the next shard's scan?  two 1.25 B-row shards on two contexts of this GPU (DESIGN round-5 item 6)"
( timeout -k 10 200 python3 "$ROOT/tools/exp/pair_overlap.py" 0.1 2>&1 | grep '^sel'; timeout -k 10 200 python3 "$ROOT/tools/exp/pair_overlap.py" 0.5 2>&1 | grep '^sel' ) > "$OUT/${R}_pair_overlap.txt"
step "two rank PROCESSES on this one GPU (bench.py --gpus 2 --share-gpu): Q1 at SF10, and TPC-H Q3 with key-aligned shards"
timeout -k 10 300 python3 "$ROOT/bench.py" --full --gpus 2 --share-gpu --no-cpu-baseline --no-extras --steps 20 2>/dev/null | grep '^{' > "$OUT/${R}_bench_share_gpu_2ranks.json"
timeout -k 10 300 python3 "$ROOT/bench.py" --full --gpus 2 --share-gpu --workload q3 --sf 10 --steps 10 --warmup 2 2>/dev/null | grep '^{' > "$OUT/${R}_bench_share_gpu_q3_2ranks.json"
step "the same Q1 step through the C ABI's one-process path: 8 shards on this one GPU"
timeout -k 10 200 python3 "$ROOT/bench.py" --full --path capi --capi-devices 0,0,0,0,0,0,0,0 --steps 20 2>/dev/null | grep '^{' > "$OUT/${R}_bench_capi_8shards_1gpu.json"
ls -la "$OUT" | tail -n 20
stamp_all
exit 0
fi

# The kernel statistics of the headline command come FIRST, on the box as it is handed over, and the profiled process's own bench line is
# kept beside them: round 4 compared a --stats average taken after minutes of 40 GB scans and a 16-thread host baseline (366 us) with HIP
# events of the box's first minute (345 us) - tools/q1_profile_gap.py shows the two agree to 1-3 % when they come from the same minute
# (profiles/history/r05_q1_rocprof_vs_events_*.txt).  tests/test_profiles_stamped.py compares the average with THIS line's step.
step "kernel trace + stats of the bench command (the profiled process's own line is kept)"
rm -rf /tmp/prof_ks
if timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_ks -- python3 "$ROOT/bench.py" --no-cpu-baseline --no-extras > /tmp/ks.log 2>&1; then
    f=$(found /tmp/prof_ks '*kernel_stats.csv'); [ -n "$f" ] && cp "$f" "$OUT/${R}_q1_sf10_kernel_stats.csv"
    grep '^{' /tmp/ks.log | tail -n 1 > "$OUT/${R}_q1_sf10_kernel_stats_run.json"
else echo "   rocprofv3 --kernel-trace failed: $(tail -n 2 /tmp/ks.log)"; fi
step "rocprofv3 durations against the engine's HIP events, same command, back to back"
timeout -k 10 400 python3 "$ROOT/tools/q1_profile_gap.py" "$OUT/${R}_q1_rocprof_vs_events.txt" > /tmp/gap.log 2>&1 || echo "   q1_profile_gap failed: $(tail -n 2 /tmp/gap.log)"

step "bench line (N = 1)"
if timeout -k 10 400 python3 "$ROOT/bench.py" --full > "$OUT/${R}_bench_n1.log" 2>&1; then
    grep '^{' "$OUT/${R}_bench_n1.log" | tail -n 1 > "$OUT/${R}_bench_n1.json"
else echo "   bench.py failed"; fi
step "bench line, multi-rank step forced on one rank (RCCL world of one)"
if timeout -k 10 300 python3 "$ROOT/bench.py" --full --dist-path --no-cpu-baseline > "$OUT/${R}_bench_distpath.log" 2>&1; then
    grep '^{' "$OUT/${R}_bench_distpath.log" | tail -n 1 > "$OUT/${R}_bench_distpath.json"
fi

pmc_pass() {   # pmc_pass COUNTER OUTDIR -- program args
    local c=$1 d=$2; shift 3
    rm -rf "$d"
    timeout -k 10 300 rocprofv3 --pmc "$c" --kernel-trace --output-format csv -d "$d" -- "$@" > "/tmp/pmc_$c.log" 2>&1 || echo "   rocprofv3 --pmc $c failed: $(tail -n 2 /tmp/pmc_$c.log)"
}
step "PMC FETCH_SIZE of the Q1 kernel (its own pass; --no-extras: no other launch of a kernel of that name in the process)"
PMC_STEPS=5; PMC_WARMUP=1
pmc_pass FETCH_SIZE /tmp/prof_pmc -- python3 "$ROOT/bench.py" --no-cpu-baseline --no-extras --steps $PMC_STEPS --warmup $PMC_WARMUP
f=$(found /tmp/prof_pmc '*counter_collection.csv')
if [ -n "$f" ]; then python3 - "$f" "$OUT/${R}_q1_sf10_pmc.json" $((PMC_STEPS + PMC_WARMUP)) <<'PY'
import csv, json, sys
rows = [r for r in csv.DictReader(open(sys.argv[1])) if r["Kernel_Name"].startswith("rsq_p0_lineitem_aggregate") and r["Counter_Name"] == "FETCH_SIZE"]
expected = int(sys.argv[3])
per = {}
for r in rows:
    per[r["Dispatch_Id"]] = per.get(r["Dispatch_Id"], 0.0) + float(r["Counter_Value"])
n = len(per); kb = sum(per.values()) / max(n, 1)
alg = 38 * 59999996
out = {"kernel": "rsq_p0_lineitem_aggregate (TPC-H Q1 SF10: scan 7 columns + filter + 6-group aggregation + last-workgroup hand-over)",
       "command": "rocprofv3 --pmc FETCH_SIZE --kernel-trace -- python3 bench.py --no-cpu-baseline --no-extras --steps 5 --warmup 1",
       "launches": n, "expected_launches": expected,
       "FETCH_SIZE_KB_per_launch": kb, "FETCH_SIZE_KB_min": min(per.values()) if per else None, "FETCH_SIZE_KB_max": max(per.values()) if per else None,
       "grid_sizes": sorted({r.get("Grid_Size", "?") for r in rows}),
       "note": "gfx950: FETCH_SIZE reports 1/2 of the bytes of wide coalesced streaming reads (MI355X_MICROARCH.md, HBM section) -> x2; collected in its own --pmc pass",
       "hbm_read_bytes_per_launch_corrected": kb * 1024 * 2, "algorithmic_bytes_per_launch": alg,
       "over_algorithmic": kb * 1024 * 2 / alg}
# a pass that saw other dispatches than the timed plan's, or whose figure cannot be a full scan's, says so itself (bench.py and
# tests/test_profiles_stamped.py refuse it): round 4's file averaged 262 SF1 + SF10 dispatches and nobody looked
if n != expected: out["invalid"] = f"{n} dispatches of the kernel where the command launches {expected}"
elif not (0.98 <= out["over_algorithmic"] <= 1.5): out["invalid"] = f"{out['over_algorithmic']:.3f} x the algorithmic bytes cannot be a full scan"
elif per and max(per.values()) > 1.05 * min(per.values()): out["invalid"] = "the dispatches differ by more than 5 %: not one configuration"
json.dump(out, open(sys.argv[2], "w"), indent=1)
print("   pmc launches", n, "of", expected, "corrected bytes", kb * 1024 * 2, "=", round(out["over_algorithmic"], 4), "x algorithmic", "INVALID: " + out["invalid"] if "invalid" in out else "")
PY
fi

step "TPC-H Q3 at SF10: executions (the first one is the cold one), kernel statistics per pipeline"
rm -rf /tmp/prof_q3
if timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_q3 -- python3 "$ROOT/tools/profile_case.py" q3 10 12 > /tmp/q3_runs.log 2>&1; then
    grep '^q3 ' /tmp/q3_runs.log > "$OUT/${R}_q3_sf10_runs.txt"
    f=$(found /tmp/prof_q3 '*kernel_stats.csv'); [ -n "$f" ] && cp "$f" "$OUT/${R}_q3_sf10_kernel_stats.csv"
fi
step "TPC-H Q3 at SF10: FETCH_SIZE and WRITE_SIZE per pipeline (two passes)"
for c in FETCH_SIZE WRITE_SIZE; do
    pmc_pass $c /tmp/prof_q3_$c -- python3 "$ROOT/tools/profile_case.py" q3 10 5
done
python3 - "$OUT/${R}_q3_sf10_pmc.json" <<'PY'
import csv, glob, json, sys
out = {"note": "average per dispatch over the steady-state executions; KB as rocprofv3 reports them (gfx950: FETCH_SIZE counts 1/2 of wide streaming reads, "
               "MI355X_MICROARCH.md) - random 8..32-byte accesses are counted in full 32-byte requests", "kernels": {}}
for c in ("FETCH_SIZE", "WRITE_SIZE"):
    fs = glob.glob(f"/tmp/prof_q3_{c}/*/*counter_collection.csv")
    if not fs: continue
    acc, n = {}, {}
    for r in csv.DictReader(open(fs[0])):
        k = r["Kernel_Name"].split("(")[0]
        if r["Counter_Name"] != c or not (k.startswith("rsq_p") or "k_rank" in k or "k_compact" in k or "k_topk" in k or "k_prepare" in k or "k_fill" in k): continue
        acc[k] = acc.get(k, 0.0) + float(r["Counter_Value"]); n.setdefault(k, set()).add(r["Dispatch_Id"])
    for k in acc: out["kernels"].setdefault(k, {})[c + "_KB_per_dispatch"] = round(acc[k] / len(n[k]), 1)
json.dump(out, open(sys.argv[1], "w"), indent=1)
print("   q3 pmc kernels:", len(out["kernels"]))
PY

step "large-group aggregation (1.25 B rows, 2^20 groups, 10 % and 50 % pass): kernel statistics, FETCH_SIZE and WRITE_SIZE in separate passes"
for s in 0.1 0.5; do
    rm -rf /tmp/prof_lg_$s
    if timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_lg_$s -- python3 "$ROOT/tools/profile_case.py" synthetic 1250000000 1048576 $s 6 > /tmp/lg_runs.log 2>&1; then
        grep '^synthetic ' /tmp/lg_runs.log > "$OUT/${R}_synth_g20_sel${s}_runs.txt"
        f=$(found /tmp/prof_lg_$s '*kernel_stats.csv'); [ -n "$f" ] && cp "$f" "$OUT/${R}_synth_g20_sel${s}_kernel_stats.csv"
    fi
    for c in FETCH_SIZE WRITE_SIZE; do
        pmc_pass $c /tmp/prof_lg_${s}_$c -- python3 "$ROOT/tools/profile_case.py" synthetic 1250000000 1048576 $s 3
    done
done
python3 - "$OUT/${R}_synth_g20_pmc.json" <<'PY'
import csv, glob, json, sys
rows = 1250000000
out = {"workload": "synthetic 4 x int64, a < tau, group by b (2^20 groups), sum(c), sum(d), count(*): one 1.25 B-row shard (40 GB)",
       "note": "per dispatch, the LARGEST dispatch of each kernel name (the sampled counting pass shares the scan kernel's name and is small); KB as "
               "rocprofv3 reports them; gfx950: FETCH_SIZE counts 1/2 of the bytes of wide coalesced streaming reads (MI355X_MICROARCH.md, HBM section) "
               "-> x2 in *_corrected; WRITE_SIZE as is; FETCH_SIZE and WRITE_SIZE were collected in separate passes",
       "algorithmic_bytes": 32 * rows, "selectivity": {}}
for s in ("0.1", "0.5"):
    e = {}
    for c in ("FETCH_SIZE", "WRITE_SIZE"):
        fs = glob.glob(f"/tmp/prof_lg_{s}_{c}/*/*counter_collection.csv")
        if not fs: continue
        per = {}
        for r in csv.DictReader(open(fs[0])):
            k = r["Kernel_Name"].split("(")[0]
            if r["Counter_Name"] != c or not (k.startswith("rsq_p") or k.startswith("rsq_staged")): continue
            per.setdefault(k, {}); per[k][r["Dispatch_Id"]] = per[k].get(r["Dispatch_Id"], 0.0) + float(r["Counter_Value"])
        for k, d in per.items():
            kb = max(d.values())
            e.setdefault(k, {})[c + "_KB"] = round(kb, 1)
            e[k]["hbm_read_bytes_corrected" if c == "FETCH_SIZE" else "hbm_write_bytes"] = round(kb * 1024 * (2 if c == "FETCH_SIZE" else 1))
    moved = sum(v.get("hbm_read_bytes_corrected", 0) + v.get("hbm_write_bytes", 0) for v in e.values())
    out["selectivity"][s] = {"kernels": e, "bytes_moved": moved, "bytes_moved_per_row": round(moved / rows, 2), "over_algorithmic": round(moved / (32 * rows), 3)}
json.dump(out, open(sys.argv[1], "w"), indent=1)
print("   large-group pmc:", {s: v["bytes_moved_per_row"] for s, v in out["selectivity"].items()}, "bytes per row")
PY

[ -f "$OUT/${R}_q1_sf10_kernel_stats.csv" ] && head -n 3 "$OUT/${R}_q1_sf10_kernel_stats.csv" | cut -c1-150
[ -f "$OUT/${R}_q3_sf10_kernel_stats.csv" ] && head -n 5 "$OUT/${R}_q3_sf10_kernel_stats.csv" | cut -c1-150
[ -f "$OUT/${R}_bench_n1.json" ] && cut -c1-600 "$OUT/${R}_bench_n1.json"
stamp_all
exit 0
