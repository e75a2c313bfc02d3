// codegen_loop.cpp - the kernel around the row function: tile loads (plain, late, staged strings), the software-pipelined and the plain
// tile loop, the wave compaction queues and their drains, the tail rows, the variants compiled from one source.
#include "codegen_internal.h"

namespace rsq {
namespace cg {

// -------------------------------------------------------------------------------------------
// staged string tiles (see strStaged): chunk c = 64 * round + lane of the tile's 8 * W 16-byte chunks
std::string Walker::postTileFor(const std::string& tile) {
    std::string out = postTile;
    for (size_t at; (at = out.find("$TILE")) != std::string::npos;) out.replace(at, 5, tile);
    return out;
}

void Walker::stagedChunkLoads(std::ostringstream& s, const std::string& ind, const char* pre, int col, int u) {     // (`b` = the lane's first row of the tile)
    const int W = strPrefetchWidth[col];
    for (int r = 0; r < stagedRounds(col); r++)
        s << ind << pre << col << "_" << u << "_" << r << " = rsq::ld_str_chunk<" << W << ", " << r << ">(a.c" << col << " + (b - lane * 2) * " << W << ", lane);\n";
}

// ... through the wave's LDS region into the words the row function takes (same-wave LDS operations execute in order)
void Walker::stagedUnstage(std::ostringstream& s, const std::string& ind, int u) {
    for (auto& sp : strPrefetch) {
        auto it = strStaged.find(sp.first);
        if (it == strStaged.end()) continue;
        const int W = strPrefetchWidth[sp.first];
        for (int r = 0; r < stagedRounds(sp.first); r++)
            s << ind << "rsq::st_str_chunk<" << W << ", " << r << ">(strt + " << it->second << ", lane, q" << sp.first << "_" << u << "_" << r << ");\n";
    }
    if (!strStaged.empty()) s << ind << "rsq::wave_lds_order();\n";
    for (auto& sp : strPrefetch) {
        auto it = strStaged.find(sp.first);
        if (it == strStaged.end()) continue;
        const int W = strPrefetchWidth[sp.first];
        for (int j = 0; j < 2; j++)
            for (int w = 0; w * 8 < sp.second; w++)
                s << ind << "const u64 s" << sp.first << "_" << u << "_" << j << "_" << w << " = rsq::ld_bytes<" << std::min(8, sp.second - w * 8) << ">(strt + " << it->second
                  << " + (lane * 2 + " << j << ") * " << W << " + " << w * 8 << ");\n";
    }
    if (!strStaged.empty()) s << ind << "rsq::wave_lds_order();\n";
}

// -------------------------------------------------------------------------------------------
// second round of loads of tile `tile` (unrolled copy u): the late columns, by the lanes that hold a row the leading selection passes
void Walker::emitLateLoads(std::ostringstream& s, const std::string& tile, int u, const std::vector<char>& lateCol, const std::string& tileEnd) {
    s << "        if (" << tile << " < " << tileEnd << ") {\n";
    for (int j = 0; j < 2; j++) {
        s << "            const bool lp" << j << " = lead_pred(a";
        for (int k : leadCols) s << ", t" << k << "_" << u << "[" << j << "]";
        s << ");\n";
    }
    s << "            if (lp0 | lp1) {\n                const i64 b = ((" << tile << ") << 7) + lane * 2;\n";
    for (size_t k = 0; k < lateCol.size(); k++) if (lateCol[k]) s << "                " << tileLoad((int)k, "t" + std::to_string(k) + "_" + std::to_string(u)) << "\n";
    s << "            }\n        }\n";
}

// the marker lines of the register aggregation's second form (codegen_internal.h): preprocessor lines, or form 0's text alone
void Walker::resolveRowCells(std::string& text, bool keep) {
    std::string out;
    bool drop = false;
    for (size_t at = 0; at < text.size();) {
        size_t end = text.find('\n', at);
        end = end == std::string::npos ? text.size() : end + 1;
        const std::string ln = text.substr(at, end - at);
        at = end;
        if (ln == RC_IFNOT) { if (keep) out += "#if !RSQ_ROW_CELLS\n"; }
        else if (ln == RC_IF) { if (keep) out += "#if RSQ_ROW_CELLS\n"; else drop = true; }
        else if (ln == RC_ELSE) { if (keep) out += "#else\n"; else drop = true; }
        else if (ln == RC_END) { if (keep) out += "#endif\n"; drop = false; }
        else if (!drop) out += ln;
    }
    text = out;
}

void Walker::finishPipeline() {
    while (indent > 1) closeScope();
    addArg("n_rows", "i64", (uint64_t)pipe.src->nRows);
    addArg("row0", "i64", (uint64_t)pipe.src->row0);
    addArg("err", "u32*", (uint64_t)(uintptr_t)q.ctx.dErr);
    // Bytes in flight: a CU streams fastest with ~40 KB of loads outstanding (8 waves x one 128-row tile of TPC-H Q1's
    // 38 B rows).  Narrower rows keep the same amount in flight with more tiles per wave: Q6 (28 B/row) went
    // 0.293 -> 0.254 ms with two tiles, the 32 B synthetic rows gained ~1.5 %; Q1 itself is slower with two (0.363 vs 0.348).
    // (the bytes the scan fetches: a narrow image counts at its width)
    if (pipe.gridPerCU == 2 && pipe.storedBytesPerRow > 0)
        pipe.unroll = (int)std::max<int64_t>(1, std::min<int64_t>(foldTile.empty() ? 4 : 2, (4608 + pipe.storedBytesPerRow * 128 - 1) / (pipe.storedBytesPerRow * 128)));
    // (... at most two with 32-bit partial sums, which hold a register per sum and group: TPC-H Q1 SF10 with its 24 partials, ms per
    // step - four tiles 0.815 (256 VGPRs, scratch), two 0.253, one 0.290)
    // A pipeline behind a wave compaction waits twice per tile — for the key columns, then (join probes) for the bitmap words their
    // values address — and few of its rows go further: it wants several tiles in flight per wave.  TPC-H Q3 at SF10, all kernels:
    // 0.415 ms with one tile, 0.381 with two, 0.367 with three, 0.363 with four (RSQ_COMPACT_UNROLL).
    if (pipe.compact) pipe.unroll = 4;
    const bool mat = pipe.sink == SinkKind::MATERIALIZE;
    std::ostringstream s;
    s << "// generated by resql_amd/csrc/codegen.cpp\n//   ";
    // (the header comment names the steps WITHOUT the row counts: the source text is the code-object cache key, and a plan
    // shape must find its kernel whatever the table sizes — the cache filled at build time from SF 0.01 tables serves SF 10)
    for (size_t i = 0; i < explainSteps.size(); i++) {
        std::string step = explainSteps[i];
        const size_t lb = step.find(" [");
        if (step.compare(0, 5, "scan ") == 0 && lb != std::string::npos) step = step.substr(0, lb);
        const size_t kb = step.find(", key bitmap of ");      // (... nor the key range the column statistics gave: "key bitmap of 59970 bits" was the ONLY
        if (kb != std::string::npos) {                         // difference between TPC-H Q3's kernels at SF 0.01 and SF 10, and cost 0.3 s of hiprtc per box)
            const size_t ke = step.find(" bits", kb);
            if (ke != std::string::npos) step = step.substr(0, kb) + ", key bitmap" + step.substr(ke + 5);
        }
        s << (i ? " -> " : "") << step;
    }
    s << "\n";
    if (1) s << "#define RSQ_NT_LOADS 1\n";
    s << "#include \"rsq_device.h\"\n";
    s << fileScope;
    if (nDictTables) {
        s << "__shared__ u64 s_dt[" << 4 * nDictTables << "];      // truth tables over dictionary-coded columns: 256 bits each, filled in the kernel's prologue\n";
        prologue += "    __syncthreads();\n";
        pipe.extraLdsBytes += 32 * nDictTables;
    }
    const bool cq = pipe.compact;
    // (measurement only, RSQ_DEBUG_TAIL=1: device timestamps per workgroup - [0] start, [1] rows done, [2] drains done, [3] end)
    const bool dbgStamps = sw::num<sw::RSQ_DEBUG_TAIL>() != 0 && !(pipe.sink == SinkKind::AGGREGATE && q.aggMode == AggMode::DENSE_REG);
    if (dbgStamps) addArg("dbg", "u64*", 0);
    // (the staged form's round loop knows neither the compaction queues nor prefetched bitmap words nor string columns)
    if (pipe.staged && (cq || mat || !bitmapPrefetch.empty() || !pipe.lazyCols.empty() ||
                        std::find(colIsString.begin(), colIsString.end(), true) != colIsString.end())) pipe.staged = false;
    // Late loads: the columns the leading selection does not read are loaded only by lanes that hold a passing row.  Memory
    // is fetched in 128-byte lines (16 rows of an 8-byte column): at 1 % selectivity 85 % of those columns' lines are never
    // fetched (measured: 1.25 B rows x 4 int64 at 1 %: 6.0 -> 3.5 ms, TPC-H Q6 SF10 0.259 -> 0.207 ms), at 10 % 19 % (-1..4 %);
    // above that the second, dependent round of loads costs more than it saves.  Decided here from the column statistics,
    // values taken as uniform (RSQ_LATE_LOADS: 0 never, 2 whenever there is a leading selection; RSQ_LATE_LOADS_BELOW percent).
    std::vector<char> lateCol(colTypes.size(), 0);
    bool late = false;
    {
        const int mode = sw::num<sw::RSQ_LATE_LOADS>();
        const double below = (double)12 / 100.0;
        if (mode && !cq && !mat && !leadCond.empty() && bitmapPrefetch.empty() && pipe.lazyCols.empty() && (mode == 2 || leadPass <= below)) {
            for (size_t k = 0; k < colTypes.size(); k++)
                if (!colIsString[k] && std::find(leadCols.begin(), leadCols.end(), (int)k) == leadCols.end()) { lateCol[k] = 1; late = true; }
        }
    }
    pipe.lateLoads = late;
    // The late-load form keeps the LEADING columns in flight, so its tiles per wave follow their width, not the row's (1.25 B
    // synthetic rows: 8 of 32 bytes lead -> four tiles).  It is software-pipelined (the main loop below): not for the few
    // shapes whose tile loads carry more than plain columns.
    // Measured (MI355X, 1.25 B synthetic rows, G = 8; kernel ms, plain order with two tiles -> pipelined with 2 / 3 / 4 tiles):
    // 1 %: 3.51 -> 2.48 / 2.40 / 2.24; 10 %: 5.86 -> 5.17 / 5.21 / 5.35; TPC-H Q6 SF10 (2 %, 20 leading bytes): 0.206 -> 0.192 / 0.191
    // / 0.197.  The more rows pass, the more of the late registers are really in use and the fewer tiles pay.
    const bool latePipelined = late;
    // ... and so is the loop of a pipeline behind a wave compaction, where its tiles are narrow (below).  Measured at SF10, whole
    // statements: TPC-H Q5 0.707 -> 0.687 ms, Q14 0.289 -> 0.276, Q3 0.289 -> 0.285, the others within noise: these pipelines are
    // bound by the dependent accesses of stage 2 (Q5's lineitem pipeline as two kernels: scan 81 us, stage 2 363 us), not by the stream.
    const bool cqPipelined = pipe.compact && !late && pipe.sink != SinkKind::MATERIALIZE;
    if (late && pipe.gridPerCU == 2) {
        int64_t leadBytes = 0;
        for (int k : leadCols) leadBytes += storedWidth(k);
        if (leadBytes > 0) pipe.unroll = (int)std::max<int64_t>(1, std::min<int64_t>(leadPass <= 0.04 ? 4 : 2, (4608 + leadBytes * 128 - 1) / (leadBytes * 128)));
    }
    pipe.leadPass = leadCond.empty() || !leadPassComplete ? -1.0 : leadPass;      // (for the engine's first layout of staged regions: only a complete estimate)
    // VGPRs of one tile's columns: all of them / without the lazily loaded ones (the loop forms are chosen by them, below)
    int eagerRegs = 0, lazyRegs = 0;
    for (size_t k = 0; k < colTypes.size(); k++) if (!colIsString[k]) {
        const int r = colTypes[k] == "i64" ? 4 : colTypes[k] == "i32" ? 2 : 1;
        eagerRegs += r;
        if (std::find(pipe.lazyCols.begin(), pipe.lazyCols.end(), (int)k) == pipe.lazyCols.end()) lazyRegs += r;
    }
    for (auto& sp : strPrefetch) { const int r = strStaged.count(sp.first) ? 4 * stagedRounds(sp.first) : 4 * ((sp.second + 7) / 8); eagerRegs += r; lazyRegs += r; }
    const int budget = 24;      // (64: TPC-H Q5 0.69 -> 0.78 ms, the eager form's 133 -> 183 VGPRs)
    // ... and the plain register aggregation over typed narrow columns (codegen_agg.cpp typeScanColumns): its arithmetic no longer
    // covers the other wave's load latency, and its tiles, counted at the decoded types, fit the budget (TPC-H Q1: 12 VGPRs a tile).
    const bool regPipelined = std::find(colTyped.begin(), colTyped.end(), 1) != colTyped.end() && pipe.sink == SinkKind::AGGREGATE &&
                              q.aggMode == AggMode::DENSE_REG && !pipe.compact && !late && bitmapPrefetch.empty() && strPrefetch.empty() && !pipe.staged &&
                              eagerRegs * pipe.unroll <= budget;
    // With 32-bit partial sums that loop is bound by its instructions, not by the stream, and what it lacks is waves to cover each
    // other's branches, hazards and load waits.  Its fold targets live in LDS (codegen_agg.cpp), so it can fit 128 VGPRs: TWO
    // 512-thread workgroups per CU, four waves per SIMD, and the compiler held to that.  Set here, behind the choice of the tiles in
    // flight above, which reads gridPerCU == 2 as "a streaming pipeline": the grid alone must not change them.
    // What the plan holds per lane decides it: the State's accumulators (accRegs), the tiles of this and the next iteration and four
    // registers a group for the row function's branches, against 128 less three allocation granules.  The sum is a fit, off by up
    // to 14 registers either way, hence the margin: a statement held to 128 VGPRs that needs 131 spills.  A plan that does not fit
    // gives up tiles in flight first; one that does not fit with one tile keeps its grid and gets no launch bound.  (The
    // statements the fit was made over, and TPC-H Q1 with one and two tiles: docs/KERNELS.md, "Partial sums folded into LDS ...".)
    const int fourWaveRegs = 128 - 24;
    bool fourWaves = regPipelined && !foldTile.empty();
    if (fourWaves) {
        auto held = [&](int u) { return accRegs + 2 * eagerRegs * u + 4 * (int)q.denseGroups; };
        int u = pipe.unroll;
        while (u > 1 && held(u) > fourWaveRegs) u--;
        fourWaves = held(u) <= fourWaveRegs;
        if (fourWaves) { pipe.unroll = u; pipe.gridPerCU = 4; }
    }
    // ... and those statements carry the second form, rows into per-lane LDS cells, under #if RSQ_ROW_CELLS: same tiles in flight, same
    // grid, same launch bound (it allocates 40 VGPRs where form 0 takes 104; docs/KERNELS.md has the other geometries measured)
    rowCells = rowCells && fourWaves && pipe.sink == SinkKind::AGGREGATE;
    for (std::string* text : {&stateDecl, &prologue, &body, &foldTile, &epilogue}) resolveRowCells(*text, rowCells);
    if (!rowCells) pipe.rowCellsEnvelopes.clear();
    const int U = pipe.unroll;
    if (strStagedBytes > 0) {
        pipe.extraLdsBytes += (pipe.blockThreads / 64) * strStagedBytes;
        prologue += "    __shared__ __attribute__((aligned(16))) char s_strt[(RSQ_BLOCK_THREADS / 64) * " + std::to_string(strStagedBytes) + "];\n    char* const strt = s_strt + (threadIdx.x >> 6) * " +
                    std::to_string(strStagedBytes) + ";\n";
    }
    // 63 left over + 128 pushed by one tile, rounded up.  (RSQ_QCAP=128 drains after every row_fn call instead: smaller
    // queues, 7 instead of 4 workgroups of a five-word pipeline per CU — measured slower: Q3's orders pipeline 0.24 ->
    // 0.31 ms, its inserts do not want more waves.)
    const int NV = 1 + pipe.compactWords;       // the row index + the carried values
    // (... unless the queues are what limits the workgroups per CU: with six or more words per row three workgroups fit next to each
    // other at 192 entries; at 128 four or five do, and TPC-H Q5's lineitem pipeline - five probes per surviving row - went from
    // 0.55 to 0.46 ms.  Pipelines whose registers set the limit - Q10, Q3 - lose 2-3 % to the extra drains and keep 192.)
    const bool queuesLimit = (144 * 1024) / std::max(1, (pipe.blockThreads / 64) * NV * 192 * 8 + pipe.extraLdsBytes) < 4;
    const int QCAP = (queuesLimit ? 128 : 192);
    const int NVL = 1 + pipe.compactWordsLazy;  // ... in the RSQ_LAZY 1 form
    const bool twoForms = !pipe.lazyCols.empty();
    if (cq) {
        // the queues take LDS: as many workgroups per CU as fit next to each other, at most the 8 of a random-access pipeline
        const int ldsPerWG = (pipe.blockThreads / 64) * NV * QCAP * 8 + pipe.extraLdsBytes;
        const int ldsPerWGLazy = (pipe.blockThreads / 64) * NVL * QCAP * 8 + pipe.extraLdsBytes;
        // (at most 6: with four tiles in flight these kernels hold 70-80 VGPRs, and a seventh workgroup per CU is not resident
        // whatever the occupancy query says - TPC-H Q3's lineitem pipeline started 256 of 1792 workgroups 67 us late; the
        // engine also clamps every grid to the query's answer, engine.cpp residentWorkgroupsPerCU)
        const int wgCap = pipe.unroll >= 3 ? 6 : 8;
        pipe.gridPerCU = std::max(2, std::min(wgCap, (144 * 1024) / std::max(1, ldsPerWG)));
        pipe.gridPerCULazy = std::max(2, std::min(wgCap, (144 * 1024) / std::max(1, ldsPerWGLazy)));
        stateDecl += "    int cq_n = 0;\n    u32 cq_rows = 0;\n    i64* cq;\n";
        // rows that reached stage 2, for the host's choice between the two forms of the kernel (see compactThen).  Only
        // the first 64 workgroups report (tiles are dealt round-robin, so they are a fair sample; the host scales): every
        // wave of the grid adding to one word cost 90 us — atomics on one address serialise
        addArg("cq_total", "unsigned long long*", 0);
        epilogue += "    if (blockIdx.x < 64) {\n        const u64 v = rsq::wave_sum((u64)st.cq_rows);\n        if ((threadIdx.x & 63) == 0 && v) atomicAdd(a.cq_total, (unsigned long long)v);\n    }\n";
        const std::string nv = twoForms ? "RSQ_CQ_NV" : std::to_string(NV);
        prologue += "    __shared__ i64 s_cq[(RSQ_BLOCK_THREADS / 64) * " + nv + " * " + std::to_string(QCAP) + "];\n";
        prologue += "    st.cq = s_cq + (threadIdx.x >> 6) * " + nv + " * " + std::to_string(QCAP) + ";\n";
    }
    if (twoForms) s << "#if RSQ_LAZY\n#define RSQ_CQ_NV " << NVL << "\n#else\n#define RSQ_CQ_NV " << NV << "\n#endif\n";
    s << "#ifndef RSQ_BLOCK_THREADS\n#define RSQ_BLOCK_THREADS " << pipe.blockThreads << "\n#endif\n";
    // (RSQ_MIN_WG is the second argument of __launch_bounds__, which counts WAVES PER SIMD: two 512-thread workgroups per CU are
    // 2 x 512 / 256 = 4, and 2 would leave the compiler 256 VGPRs)
    if (fourWaves) s << "#define RSQ_MIN_WG 4\n";
    s << "struct Args {\n";
    for (auto& a : pipe.args) s << "    " << a.ctype << " " << a.name << ";\n";
    s << "};\nstruct State {\n" << stateDecl << "};\n";
    s << helperFns;
    if (cq) {
        // stage 2: everything behind the compaction point, called with dense lanes
        // (Stage 2 as a real function CALLED from the drains instead of inlined at every drain site compiles three times faster - TPC-H
        // Q5's lineitem kernel: 72 KB of code and 1.9 s of hiprtc against 24 KB and 0.66 s - and runs 40-65 % slower: Q5 0.69 -> 1.14 ms,
        // Q10 0.92 -> 1.29, Q3 0.29 -> 0.40 at SF10 (the State lives in scratch memory across the call).  Inlined.)
        // ... which is why a statement whose kernels are not in the code-object cache gets them in TWO TIERS (engine.cpp): the same text with
        // RSQ_STAGE2_CALL defined - stage 2 a real call, ready in a third of the time - runs first, the inlined kernel replaces it when ready.
        s << "#ifdef RSQ_STAGE2_CALL\nstatic __device__ __attribute__((noinline)) void stage2(const Args& a, State& st, const i64 row";
        for (int k = 0; k < pipe.compactWords; k++) s << ", const i64 qw_" << k;
        s << ")\n#else\n";
        s << "static RSQ_DEV void stage2(const Args& a, State& st, const i64 row";
        for (int k = 0; k < pipe.compactWords; k++) s << ", const i64 qw_" << k;
        s << ")\n#endif\n{\n" << stage2Body << "}\n";
        pipe.hasStage2 = true;
        s << "static RSQ_DEV void cq_drain(const Args& a, State& st, const int count) {\n";
        s << "    const int lane = threadIdx.x & 63;\n    const int i = st.cq_n - count + lane;\n    rsq::wave_lds_order();      // (the entries were pushed by other lanes)\n";
        s << "    if (lane < count) {\n        stage2(a, st, st.cq[i]";
        for (int k = 0; k < pipe.compactWordsLazy; k++) s << ", st.cq[" << (k + 1) * QCAP << " + i]";
        if (pipe.compactWords > pipe.compactWordsLazy) {
            s << "\n#if RSQ_LAZY\n            ";
            for (int k = pipe.compactWordsLazy; k < pipe.compactWords; k++) s << ", 0";
            s << "\n#else\n            ";
            for (int k = pipe.compactWordsLazy; k < pipe.compactWords; k++) s << ", st.cq[" << (k + 1) * QCAP << " + i]";
            s << "\n#endif\n        ";
        }
        s << ");\n        st.cq_rows++;\n    }\n    st.cq_n -= count;\n}\n";
    }
    if (late) {
        s << "static RSQ_DEV bool lead_pred(const Args& a";
        for (int k : leadCols) s << ", " << colTypes[(size_t)k] << " " << paramName(k);
        s << ") { ";
        for (int k : leadCols) if (coded(k)) s << "const rsq::Str v_" << k << " = " << dictDecode(k, paramName(k)) << "; (void)v_" << k << "; ";
        for (int k : leadCols) if (typedCol(k)) s << "const i64 v_" << k << " = (i64)n_" << k << "; ";
        s << "return " << leadCond << "; }\n";
    }
    if (pipe.staged) s << "#if RSQ_AGG_VARIANT == 3\ntemplate <int SP_SLOT>       // the row's place among the rows a thread handles per round\n#endif\n";
    s << "static RSQ_DEV void row_fn(const Args& a, State& st, const i64 lr" << (cq ? ", const bool valid" : "") << rowParams << ") {\n";
    s << "    const i64 row = a.row0 + lr;\n";
    if (cq) {
        s << "    bool cq_pass = false;\n";
        for (int k = 0; k < pipe.compactWords; k++) s << "    i64 cq_" << k << " = 0;\n";
        s << "    if (valid) {\n" << body << "    }\n";
        // push: every lane of the wave is here (the callers keep the control flow wave-uniform)
        s << "    {\n        const int lane = threadIdx.x & 63;\n        const u64 m = __ballot(cq_pass);\n";
        s << "        if (cq_pass) {\n            const int s = st.cq_n + (int)__popcll(m & ((1ull << lane) - 1ull));\n            st.cq[s] = row;\n";
        for (int k = 0; k < pipe.compactWords; k++) {
            if (k == pipe.compactWordsLazy && pipe.compactWords > pipe.compactWordsLazy) s << "#if !RSQ_LAZY\n";
            s << "            st.cq[" << (k + 1) * QCAP << " + s] = cq_" << k << ";\n";
        }
        if (pipe.compactWords > pipe.compactWordsLazy) s << "#endif\n";
        s << "        }\n        st.cq_n += (int)__popcll(m);\n    }\n}\n";
    } else s << body << "}\n";
    // The count pass of a materialisation behind a selection that stands directly above the scan evaluates that selection for BOTH rows of the
    // lane first and runs what follows it - the probes: a chain of dependent random accesses - once, for whichever row passed (and a second time
    // in the lanes where both did: rare exactly where this matters).  The two row functions of a lane otherwise run one after the other, each
    // with its own few active lanes and its own chain latency per tile, and nothing of the next tile is in flight meanwhile: TPC-H Q19's count
    // pass (7 % of the rows pass the string selection, 47 B per row) ran at 4.5 TB/s.  Counting does not care about the order of the two rows;
    // the write pass, whose positions do, keeps the two calls.
    bool pairOk = false;
    if (mat && !cq && !late && U == 1 && !pipe.staged && pairSplit != std::string::npos && pairSplit <= body.size()) {
        const std::string ifLine = "    if (" + pairCond + ") {\n", closeLine = "    }\n";
        if (body.compare(pairSplit, ifLine.size(), ifLine) == 0 && body.size() >= pairSplit + ifLine.size() + closeLine.size() &&
            body.compare(body.size() - closeLine.size(), closeLine.size(), closeLine) == 0) {
            const std::string pre = body.substr(0, pairSplit);
            const std::string rest = body.substr(pairSplit + ifLine.size(), body.size() - closeLine.size() - pairSplit - ifLine.size());
            s << "#if RSQ_PASS == 1\n";
            s << "static RSQ_DEV bool lead_any(const Args& a, const i64 lr" << rowParams << ") {\n    const i64 row = a.row0 + lr; (void)row;\n" << pre << "    return " << pairCond << ";\n}\n";
            s << "static RSQ_DEV void rest_fn(const Args& a, State& st, const i64 lr" << rowParams << ") {\n    const i64 row = a.row0 + lr; (void)row;\n" << pre << rest << "}\n";
            s << "#endif\n";
            pairOk = true;
        }
    }
    // one kernel name per pipeline — rsq_p<index>_<scanned table>_<sink> — so that a kernel trace (rocprofv3
    // --kernel-trace --stats) splits a multi-pipeline query into its phases
    {
        std::string tn;
        for (char c : pipe.src->name) tn += (isalnum((unsigned char)c) ? c : '_');
        const char* sk = pipe.sink == SinkKind::BUILD ? "build" : pipe.sink == SinkKind::MATERIALIZE ? "materialize" : "aggregate";
        pipe.entry = "rsq_p" + std::to_string(q.pipelines.size()) + "_" + tn + "_" + sk;
        if (pipe.sink == SinkKind::BUILD) pipe.entry += "_ht" + std::to_string(pipe.buildTable);
    }
    s << "#ifdef RSQ_MIN_WG\nextern \"C\" __global__ void __launch_bounds__(RSQ_BLOCK_THREADS, RSQ_MIN_WG) " << pipe.entry << "(Args a) {\n#else\n";
    s << "extern \"C\" __global__ void __launch_bounds__(RSQ_BLOCK_THREADS) " << pipe.entry << "(Args a) {\n#endif\n";
    s << "    State st;\n" << prologue;
    if (dbgStamps) s << "    if (a.dbg && threadIdx.x == 0) a.dbg[(u64)blockIdx.x * 8 + 0] = (u64)wall_clock64();\n";
    s << "    const int lane = threadIdx.x & 63;\n";
    // (a sliced pair loop, codegen.cpp consumeNestedLoops: the outer side's tiles and tail rows are dealt to the VIRTUAL workgroups, so that
    // every slice of the inner range meets every row once; whatever identifies the real workgroup - the ticket of the last one, the
    // debug stamps, per-wave regions - keeps blockIdx.x / gridDim.x)
    const std::string bx = pipe.nljSliced >= 0 ? "nlj_vb" : "blockIdx.x", gx = pipe.nljSliced >= 0 ? "nlj_vg" : "gridDim.x";
    s << "    const i64 wave = (i64)" << bx << " * (blockDim.x >> 6) + (threadIdx.x >> 6);\n";
    s << "    const i64 nwaves = (i64)" << gx << " * (blockDim.x >> 6);\n";
    s << "    const i64 ntiles = a.n_rows >> 7;\n";
    if (pipe.partitioned) s << "#if RSQ_AGG_VARIANT == 1\n    const i64 tstep = a.tile_step;      // > 1: sample every n-th tile\n#else\n    const i64 tstep = 1;\n#endif\n";
    else s << "    const i64 tstep = 1;\n";
    const int ncols = (int)colTypes.size();
    if (pipe.staged) {
        // Form 3 walks the table in ROUNDS of blockDim.x * RPT rows with the workgroup in step (every thread reaches the
        // barriers of stage_commit): wave w of the workgroup takes RPT/2 consecutive 128-row tiles of the round.
        const int H = pipe.stagedRows / 2;
        s << "#if RSQ_AGG_VARIANT == 3\n";
        s << "    const i64 tpr = (i64)(blockDim.x >> 6) * " << H << ";        // tiles per round\n";
        s << "    const i64 nrounds = (ntiles + tpr - 1) / tpr;\n";
        s << "    for (i64 round = blockIdx.x; round < nrounds; round += gridDim.x) {\n";
        s << "        st.sp_pending = 0u; st.sp_wm = s_stage.wm;\n";
        s << "        const i64 t0 = round * tpr + (i64)(threadIdx.x >> 6) * " << H << ";\n";
        for (int u = 0; u < H; u++) {
            for (int k = 0; k < ncols; k++) if (!colIsString[(size_t)k]) s << "        " << colTypes[(size_t)k] << " t" << k << "_" << u << "[2]" << (lateCol[(size_t)k] ? " = {0, 0}" : "") << ";\n";
            s << "        if (t0 + " << u << " < ntiles) {\n            const i64 b = ((t0 + " << u << ") << 7) + lane * 2;\n";
            for (int k = 0; k < ncols; k++) if (!colIsString[(size_t)k] && !lateCol[(size_t)k]) s << "            " << tileLoad(k, "t" + std::to_string(k) + "_" + std::to_string(u)) << "\n";
            s << "        }\n";
        }
        if (late) for (int u = 0; u < H; u++) emitLateLoads(s, "t0 + " + std::to_string(u), u, lateCol);
        for (int u = 0; u < H; u++) {
            s << "        if (t0 + " << u << " < ntiles) {\n";
            for (int j = 0; j < 2; j++) {
                s << "            row_fn<" << (2 * u + j) << ">(a, st, ((t0 + " << u << ") << 7) + lane * 2 + " << j;
                for (int k = 0; k < ncols; k++) if (!colIsString[(size_t)k]) s << ", t" << k << "_" << u << "[" << j << "]";
                s << ");\n";
            }
            s << "        }\n";
        }
        s << "        if (!a.sp_mode) rsq::stage_commit<" << pipe.stagedRecWords << ", " << pipe.partCount << ", " << pipe.stagedRows
          << ">(s_stage, st.sp_rec, st.sp_k, st.sp_p, st.sp_pending, a.sp_rec, a.sp_ctl, " << q.denseGroups << "u);\n";
        s << "    }\n";
        s << "    if (blockIdx.x == 0 && (a.n_rows & 127)) {        // the rows behind the last whole tile: one more round of workgroup 0\n";
        s << "        st.sp_pending = 0u; st.sp_wm = s_stage.wm;\n";
        s << "        const i64 r = (ntiles << 7) + threadIdx.x;\n";
        s << "        if (r < a.n_rows) row_fn<0>(a, st, r" << rowArgsTail << ");\n";
        s << "        if (!a.sp_mode) rsq::stage_commit<" << pipe.stagedRecWords << ", " << pipe.partCount << ", " << pipe.stagedRows
          << ">(s_stage, st.sp_rec, st.sp_k, st.sp_p, st.sp_pending, a.sp_rec, a.sp_ctl, " << q.denseGroups << "u);\n";
        s << "    }\n";
        s << "    rsq::stage_finish(s_stage, a.sp_rec, a.sp_counts, a.sp_ctl, a.sp_mode != 0u);\n";
        s << "#else\n";
    }
    // main loop, textually unrolled: the loads of U tiles are issued before the first row is processed
    // (Tiles handed out DYNAMICALLY - per-pool counters, a wave drawing its next chunk one iteration ahead - were built and measured
    // slower: TPC-H Q1 SF10 370 instead of 338 us, Q3 0.341 instead of 0.302 ms, Q6 0.24 instead of 0.207 ms; the returning atomics
    // cost more than the tail they remove.  Tiles are dealt to the waves round-robin.)
    auto emitPipelinedLoop = [&]() {
        // The software-pipelined main loop.  Per iteration a wave
        //   (1) works on its U tiles whose columns were requested ONE ITERATION AGO: the late-load form decides the leading
        //       selection and requests the other columns for the lanes that hold a passing row; a pipeline behind a wave
        //       compaction requests the key-bitmap words its rows address;
        //   (2) requests the NEXT iteration's tile columns;
        //   (3) runs the row function (and the drains of the compaction queues).
        // Memory operations return in issue order, so (2) must stand behind (1): whoever waits for the dependent loads of (1) waits
        // for everything issued before them, never for what was issued after.  The wave then stalls once per iteration with the
        // next tiles' stream in flight the whole time; the plain order - tile loads, wait, dependent loads, wait, rows - had
        // nothing streaming during the second wait and the drains (1.25 B rows at 1 %: 3.69 ms for 14.5 GB fetched, 0.49 of peak).
        // The loads of (2) are unconditional, their tile index clamped to the last tile: the compiler counts the loads it KNOWS
        // stand behind the dependent ones when it places the wait in front of the row function - a load under a condition
        // would not count and the wait would cover the next tiles too.
        std::vector<int> tileCols;
        if (late) tileCols = leadCols;
        else for (int k = 0; k < ncols; k++) if (!colIsString[(size_t)k]) tileCols.push_back(k);
        auto isLazy = [&](int k) { return std::find(pipe.lazyCols.begin(), pipe.lazyCols.end(), k) != pipe.lazyCols.end(); };
        auto tileLoads = [&](const std::string& ind, const char* pre, int u) {      // pre: "t" / "s" (this iteration's) or "n" / "ns" (the next one's)
            const std::string spre = pre[0] == 'n' ? "ns" : "s";
            for (auto& sp : strPrefetch) {
                if (strStaged.count(sp.first)) { stagedChunkLoads(s, ind, pre[0] == 'n' ? "nq" : "q", sp.first, u); continue; }
                for (int j = 0; j < 2; j++)
                    for (int w = 0; w * 8 < sp.second; w++)
                        s << ind << spre << sp.first << "_" << u << "_" << j << "_" << w << " = rsq::ld_bytes<" << std::min(8, sp.second - w * 8) << ">(a.c" << sp.first
                          << " + (b + " << j << ") * " << strPrefetchWidth[sp.first] << " + " << w * 8 << ");\n";
            }
            for (int k : tileCols) {
                if (isLazy(k)) s << "#if !RSQ_LAZY\n";
                s << ind << tileLoad(k, pre + std::to_string(k) + "_" + std::to_string(u)) << "\n";
                if (isLazy(k)) s << "#endif\n";
            }
        };
        s << "    const i64 tend = ntiles;\n";
        for (int u = 0; u < U; u++) {
            for (int k : tileCols) s << "    " << colTypes[(size_t)k] << " t" << k << "_" << u << "[2] = {0, 0};\n";
            for (auto& sp : strPrefetch) {
                if (strStaged.count(sp.first)) { stagedChunkDecls(s, "    ", "q", sp.first, u); continue; }
                for (int j = 0; j < 2; j++) for (int w = 0; w * 8 < sp.second; w++) s << "    u64 s" << sp.first << "_" << u << "_" << j << "_" << w << " = 0;\n";
            }
        }
        for (int u = 0; u < U; u++) {
            s << "    {\n        const i64 p = wave * tstep + " << u << " * nwaves * tstep;\n        if (p < tend) {\n            const i64 b = (p << 7) + lane * 2;\n";
            tileLoads("            ", "t", u);
            s << "        }\n    }\n";
        }
        s << "    for (i64 t = wave * tstep; t < ntiles; t += nwaves * tstep * " << U << ") {\n";
        for (int u = 0; u < U; u++) {
            s << "        const i64 tt" << u << " = t + " << u << " * nwaves * tstep;\n";
            for (int k = 0; k < ncols; k++) if (!colIsString[(size_t)k] && lateCol[(size_t)k]) s << "        " << colTypes[(size_t)k] << " t" << k << "_" << u << "[2] = {0, 0};\n";
        }
        if (late) for (int u = 0; u < U; u++) emitLateLoads(s, "tt" + std::to_string(u), u, lateCol, "tend");
        for (int u = 0; u < U; u++)
            for (auto& pf : bitmapPrefetch) {
                s << "        u32 pf_" << pf.first << "_" << u << "[2] = {0u, 0u};\n";
                s << "        if (tt" << u << " < tend) {\n";
                for (int j = 0; j < 2; j++)
                    s << "            pf_" << pf.first << "_" << u << "[" << j << "] = " << (pf.interleaved ? "rsq::bmi_load(a." : "rsq::bm_word(a.") << pf.first << "_bm, a." << pf.first
                      << "_bmmin, a." << pf.first << "_bmbits, (i64)t" << pf.second << "_" << u << "[" << j << "]);\n";
                s << "        }\n";
            }
        for (int u = 0; u < U; u++) {
            for (int k : tileCols) s << "        " << colTypes[(size_t)k] << " n" << k << "_" << u << "[2] = {0, 0};\n";
            for (auto& sp : strPrefetch) {
                if (strStaged.count(sp.first)) { stagedChunkDecls(s, "        ", "nq", sp.first, u); continue; }
                for (int j = 0; j < 2; j++) for (int w = 0; w * 8 < sp.second; w++) s << "        u64 ns" << sp.first << "_" << u << "_" << j << "_" << w << " = 0;\n";
            }
            s << "        {\n            const i64 nt = tt" << u << " + nwaves * tstep * " << U << ";\n            const i64 b = ((nt < tend ? nt : tend - 1) << 7) + lane * 2;\n";
            tileLoads("            ", "n", u);
            s << "        }\n";
        }
        for (int u = 0; u < U; u++) {
            s << "        if (tt" << u << " < tend) {\n";
            stagedUnstage(s, "            ", u);
            for (int j = 0; j < 2; j++) {
                s << "            row_fn(a, st, (tt" << u << " << 7) + lane * 2 + " << j << (cq ? ", true" : "");
                for (int k = 0; k < ncols; k++) if (!colIsString[(size_t)k]) s << ", t" << k << "_" << u << "[" << j << "]";
                for (auto& sp : strPrefetch) for (int w = 0; w * 8 < sp.second; w++) s << ", s" << sp.first << "_" << u << "_" << j << "_" << w;
                for (auto& pf : bitmapPrefetch) s << ", pf_" << pf.first << "_" << u << "[" << j << "]";
                s << ");\n";
                if (cq && (QCAP < 192 || j == 1)) s << "            while (st.cq_n >= 64) cq_drain(a, st, 64);\n";
            }
            s << postTileFor("tt" + std::to_string(u));
            s << foldTile;
            s << "        }\n";
        }
        for (int u = 0; u < U; u++) {
            for (int k : tileCols) s << "        t" << k << "_" << u << "[0] = n" << k << "_" << u << "[0]; t" << k << "_" << u << "[1] = n" << k << "_" << u << "[1];\n";
            for (auto& sp : strPrefetch) {
                if (strStaged.count(sp.first)) {
                    for (int r = 0; r < stagedRounds(sp.first); r++) s << "        q" << sp.first << "_" << u << "_" << r << " = nq" << sp.first << "_" << u << "_" << r << ";\n";
                    continue;
                }
                for (int j = 0; j < 2; j++) for (int w = 0; w * 8 < sp.second; w++)
                    s << "        s" << sp.first << "_" << u << "_" << j << "_" << w << " = ns" << sp.first << "_" << u << "_" << j << "_" << w << ";\n";
            }
        }
        s << "    }\n";
    };
    auto emitPlainLoop = [&]() {
    s << "    const i64 tend = ntiles;\n";
    const bool matSkip = mat && !cq && !late && 1 != 0;
    pipe.matSkip = matSkip;
    // The write pass looks at the counts of 64 of the wave's tiles with ONE load and walks the tiles that counted something: asking tile by
    // tile was a chain of dependent 4-byte loads - TPC-H Q19's write pass, 1107 rows in 1100 of 468 750 tiles, spent 32 us on 57 of them per wave.
    const bool liveWalk = matSkip && U == 1;
    if (liveWalk) {
        s << "#if RSQ_PASS == 2\n    for (i64 tg = wave * tstep; tg < ntiles; tg += nwaves * tstep * 64) {\n";
        s << "        const i64 tl = tg + (i64)lane * nwaves * tstep;\n        u64 live_m = __ballot(tl < ntiles && a.tcnt[tl < ntiles ? tl : 0] != 0u);\n";
        s << "        while (live_m) {\n        const i64 t = tg + (i64)(__ffsll((long long)live_m) - 1) * nwaves * tstep;\n        live_m &= live_m - 1;\n";
        s << "#else\n    for (i64 t = wave * tstep; t < ntiles; t += nwaves * tstep * " << U << ") {\n        {\n#endif\n";
    } else
    s << "    for (i64 t = wave * tstep; t < ntiles; t += nwaves * tstep * " << U << ") {\n";
    auto tileLive = [&](int u) { return matSkip ? "live" + std::to_string(u) : "tt" + std::to_string(u) + " < tend"; };
    for (int u = 0; u < U; u++) {
        s << "        const i64 tt" << u << " = t + " << u << " * nwaves * tstep;\n";
        for (int k = 0; k < ncols; k++) if (!colIsString[(size_t)k]) s << "        " << colTypes[(size_t)k] << " t" << k << "_" << u << "[2]" << (lateCol[(size_t)k] ? " = {0, 0}" : "") << ";\n";
        for (auto& sp : strPrefetch) {
            if (strStaged.count(sp.first)) { stagedChunkDecls(s, "        ", "q", sp.first, u); continue; }
            for (int j = 0; j < 2; j++)
                for (int w = 0; w * 8 < sp.second; w++) s << "        u64 s" << sp.first << "_" << u << "_" << j << "_" << w << " = 0;\n";
        }
        // The write pass of a materialisation skips every tile whose 64 lane slots counted nothing in the count pass: a selective
        // statement (TPC-H Q19: 1107 rows out of 60 M) then reads its columns once, not twice.
        if (liveWalk) s << "#if RSQ_PASS == 2\n        const bool live" << u << " = true;\n#else\n"
                       << "        const bool live" << u << " = tt" << u << " < tend;\n#endif\n";
        else
        if (matSkip) s << "#if RSQ_PASS == 2\n        const bool live" << u << " = tt" << u << " < tend && a.tcnt[tt" << u << "] != 0u;\n#else\n"
                       << "        const bool live" << u << " = tt" << u << " < tend;\n#endif\n";
        s << "        if (" << tileLive(u) << ") {\n            const i64 b = (tt" << u << " << 7) + lane * 2;\n";
        for (auto& sp : strPrefetch) {
            if (strStaged.count(sp.first)) { stagedChunkLoads(s, "            ", "q", sp.first, u); continue; }
            for (int j = 0; j < 2; j++)
                for (int w = 0; w * 8 < sp.second; w++)
                    s << "            s" << sp.first << "_" << u << "_" << j << "_" << w << " = rsq::ld_bytes<" << std::min(8, sp.second - w * 8) << ">(a.c" << sp.first
                      << " + (b + " << j << ") * " << strPrefetchWidth[sp.first] << " + " << w * 8 << ");\n";
        }
        for (int k = 0; k < ncols; k++) if (!colIsString[(size_t)k] && !lateCol[(size_t)k]) {
            const bool lazy = std::find(pipe.lazyCols.begin(), pipe.lazyCols.end(), k) != pipe.lazyCols.end();
            if (lazy) s << "#if !RSQ_LAZY\n";
            s << "            " << tileLoad(k, "t" + std::to_string(k) + "_" + std::to_string(u)) << "\n";
            if (lazy) s << "#else\n            t" << k << "_" << u << "[0] = t" << k << "_" << u << "[1] = 0;\n#endif\n";
        }
        s << "        }\n";
    }
    if (late) for (int u = 0; u < U; u++) emitLateLoads(s, "tt" + std::to_string(u), u, lateCol, "tend");
    for (int u = 0; u < U; u++)
        for (auto& pf : bitmapPrefetch) {
            s << "        u32 pf_" << pf.first << "_" << u << "[2] = {0u, 0u};\n";
            s << "        if (" << tileLive(u) << ") {\n";
            for (int j = 0; j < 2; j++) {
                s << "            pf_" << pf.first << "_" << u << "[" << j << "] = ";
                s << (pf.interleaved ? "rsq::bmi_load(a." : "rsq::bm_word(a.") << pf.first << "_bm, a." << pf.first << "_bmmin, a." << pf.first
                  << "_bmbits, (i64)t" << pf.second << "_" << u << "[" << j << "]);\n";
            }
            s << "        }\n";
        }
    for (int u = 0; u < U; u++) {
        s << "        if (" << tileLive(u) << ") {\n";
        stagedUnstage(s, "            ", u);
        if (mat) s << "            const i64 slot = tt" << u << " * 64 + lane;\n#if RSQ_PASS == 2\n            st.pos = a.toffs[tt" << u << "] + (u64)rsq::wave_excl_sum_u32(a.cnt[slot]);\n#endif\n";
        if (pairOk) {
            std::vector<std::string> av[2];
            for (int j = 0; j < 2; j++) {
                for (int k = 0; k < ncols; k++) if (!colIsString[(size_t)k]) av[j].push_back("t" + std::to_string(k) + "_" + std::to_string(u) + "[" + std::to_string(j) + "]");
                for (auto& sp : strPrefetch) for (int w = 0; w * 8 < sp.second; w++) av[j].push_back("s" + std::to_string(sp.first) + "_" + std::to_string(u) + "_" + std::to_string(j) + "_" + std::to_string(w));
                for (auto& pf : bitmapPrefetch) av[j].push_back("pf_" + pf.first + "_" + std::to_string(u) + "[" + std::to_string(j) + "]");
            }
            s << "#if RSQ_PASS == 1\n            {\n                const i64 lr0 = (tt" << u << " << 7) + lane * 2, lr1 = lr0 + 1;\n";
            for (int j = 0; j < 2; j++) {
                s << "                const bool lp" << j << " = lead_any(a, lr" << j;
                for (auto& x : av[j]) s << ", " << x;
                s << ");\n";
            }
            s << "                if (lp0 | lp1) {\n                    rest_fn(a, st, lp0 ? lr0 : lr1";
            for (size_t i = 0; i < av[0].size(); i++) s << ", lp0 ? " << av[0][i] << " : " << av[1][i];
            s << ");\n                    if (lp0 & lp1) rest_fn(a, st, lr1";
            for (auto& x : av[1]) s << ", " << x;
            s << ");\n                }\n            }\n#else\n";
        }
        for (int j = 0; j < 2; j++) {
            s << "            row_fn(a, st, (tt" << u << " << 7) + lane * 2 + " << j << (cq ? ", true" : "");
            for (int k = 0; k < ncols; k++) if (!colIsString[(size_t)k]) s << ", t" << k << "_" << u << "[" << j << "]";
            for (auto& sp : strPrefetch) for (int w = 0; w * 8 < sp.second; w++) s << ", s" << sp.first << "_" << u << "_" << j << "_" << w;
            for (auto& pf : bitmapPrefetch) s << ", pf_" << pf.first << "_" << u << "[" << j << "]";
            s << ");\n";
            if (cq && (QCAP < 192 || j == 1)) s << "            while (st.cq_n >= 64) cq_drain(a, st, 64);\n";
        }
        if (pairOk) s << "#endif\n";
        if (mat) s << "#if RSQ_PASS == 1\n            a.cnt[slot] = st.cnt;\n            { const u32 ts = (u32)rsq::wave_sum((u64)st.cnt); if (lane == 0) a.tcnt[tt" << u << "] = ts; }\n            st.cnt = 0;\n#endif\n";
        s << postTileFor("tt" + std::to_string(u));
        s << foldTile;
        s << "        }\n";
    }
    if (liveWalk) s << "        }\n";
    s << "    }\n";
    };
    // Double-buffered tile registers pay where the tiles are narrow: the late-load form (leading columns only), the RSQ_LAZY 1
    // form of a compaction pipeline (the columns stage 1 reads), any compaction pipeline whose tiles take few registers.  A
    // wide eager tile set would cost the occupancy the plan needs (TPC-H Q5 / Q10 lineitem: 133 -> 183 VGPRs).
    {
        const bool eagerOk = cqPipelined && eagerRegs * U <= budget, lazyOk = cqPipelined && lazyRegs * U <= budget;
        if (latePipelined || regPipelined || (eagerOk && (lazyOk || pipe.lazyCols.empty()))) emitPipelinedLoop();
        else if (lazyOk && !pipe.lazyCols.empty()) { s << "#if RSQ_LAZY\n"; emitPipelinedLoop(); s << "#else\n"; emitPlainLoop(); s << "#endif\n"; }
        else emitPlainLoop();
    }
    if (dbgStamps) s << "    if (a.dbg && threadIdx.x == 0) a.dbg[(u64)blockIdx.x * 8 + 1] = (u64)wall_clock64();\n";
    if (!postTile.empty()) s << "    st.in_tile = false;\n";
    if (cq) {
        // tail rows with a wave-uniform trip count (the push votes across the wave)
        s << "    for (i64 rb = (ntiles << 7) + (i64)" << bx << " * blockDim.x; rb < a.n_rows; rb += (i64)" << gx << " * blockDim.x) {\n";
        s << "        const i64 r = rb + threadIdx.x;\n        const bool valid = r < a.n_rows;\n";
        s << "        row_fn(a, st, r, valid" << rowArgsTailGuarded << ");\n";
        s << "        while (st.cq_n >= 64) cq_drain(a, st, 64);\n    }\n";
        s << "    while (st.cq_n > 0) cq_drain(a, st, st.cq_n < 64 ? st.cq_n : 64);\n";
    } else {
        if (mat) {
            // the rows behind the last whole tile, 64 to a wave: pseudo-tiles ntiles and ntiles + 1 of the count arrays (wave-uniform trip count)
            s << "    for (i64 rb = (ntiles << 7) + (i64)blockIdx.x * blockDim.x + (i64)(threadIdx.x & ~63u); rb < a.n_rows; rb += (i64)gridDim.x * blockDim.x) {\n";
            s << "        const i64 r = rb + lane;\n        const bool valid = r < a.n_rows;\n";
            s << "        const i64 ttile = ntiles + ((rb - (ntiles << 7)) >> 6);\n        const i64 slot = ttile * 64 + lane;\n";
            s << "#if RSQ_PASS == 2\n        st.pos = a.toffs[ttile] + (u64)rsq::wave_excl_sum_u32(valid ? a.cnt[slot] : 0u);\n#endif\n";
            s << "        if (valid) row_fn(a, st, r" << rowArgsTail << ");\n";
            s << "#if RSQ_PASS == 1\n        a.cnt[slot] = st.cnt;\n        { const u32 ts = (u32)rsq::wave_sum((u64)st.cnt); if (lane == 0) a.tcnt[ttile] = ts; }\n        st.cnt = 0;\n#endif\n";
            s << "    }\n";
        } else {
        s << "    for (i64 r = (ntiles << 7) + (i64)" << bx << " * blockDim.x + threadIdx.x; r < a.n_rows; r += (i64)" << gx << " * blockDim.x) {\n";
        s << "        row_fn(a, st, r" << rowArgsTail << ");\n";
        s << "    }\n";
        }
    }
    if (pipe.staged) s << "#endif\n";
    if (dbgStamps) s << "    if (a.dbg && threadIdx.x == 0) a.dbg[(u64)blockIdx.x * 8 + 2] = (u64)wall_clock64();\n";
    s << epilogue;
    if (dbgStamps) s << "    __syncthreads();\n    if (a.dbg && threadIdx.x == 0) a.dbg[(u64)blockIdx.x * 8 + 3] = (u64)wall_clock64();\n";
    s << "}\n";
    pipe.source = s.str();
    if (!pipe.lazyCols.empty()) pipe.source = "#define RSQ_LAZY 0\n" + pipe.source;
    if (mat) {   // two code objects from one source
        pipe.sourcePass1 = "#define RSQ_PASS 1\n" + pipe.source;
        pipe.source = "#define RSQ_PASS 2\n" + pipe.source;
    }
    if (q.aggPad > 1 && pipe.sink == SinkKind::AGGREGATE && !pipe.partitioned) {
        // padded flush for full executions, flat flush (straight into the [block][group] table that is merged
        // across GPUs) for partial ones
        pipe.sourceFlat = "#define RSQ_OUT_STRIDE 1\n" + pipe.source;
        pipe.source = "#define RSQ_OUT_STRIDE " + std::to_string(q.aggPad) + "\n" + pipe.source;
    }
    if (rowCells) {           // the second form of the register aggregation: same texts, RSQ_ROW_CELLS 1 (the engine picks per execution)
        const std::string guard = "#ifndef RSQ_ROW_CELLS\n#define RSQ_ROW_CELLS 0\n#endif\n";
        pipe.sourceCells = "#define RSQ_ROW_CELLS 1\n" + guard + pipe.source;
        pipe.source = guard + pipe.source;
        if (!pipe.sourceFlat.empty()) { pipe.sourceFlatCells = "#define RSQ_ROW_CELLS 1\n" + guard + pipe.sourceFlat; pipe.sourceFlat = guard + pipe.sourceFlat; }
    }
    if (pipe.partitioned) {   // three code objects from one source (see emitDenseAggregation)
        // count and scatter run as ONE 1024-thread workgroup per CU (see the note at the record stores)
        pipe.sourcePartCount = "#define RSQ_AGG_VARIANT 1\n#define RSQ_BLOCK_THREADS 1024\n" + pipe.source;
        pipe.sourcePartScatter = "#define RSQ_AGG_VARIANT 2\n#define RSQ_BLOCK_THREADS 1024\n" + pipe.source;
        if (pipe.staged) pipe.sourceStagedScatter = "#define RSQ_AGG_VARIANT 3\n#define RSQ_BLOCK_THREADS 1024\n" + pipe.source;
        pipe.source = "#define RSQ_AGG_VARIANT 0\n" + pipe.source;
    }
    if (!pipe.lazyCols.empty()) {          // the late-load form of the full-execution kernel: same text, RSQ_LAZY 1
        pipe.sourceLazy = pipe.source;
        const std::string off = "#define RSQ_LAZY 0\n";
        const size_t at = pipe.sourceLazy.find(off);
        if (at == std::string::npos) pipe.sourceLazy.clear();
        else {
            // The late-load form runs stage 2 for a few per cent of the rows, but its registers are the kernel's: a hash aggregation
            // with dozens of carried words holds 160 VGPRs and leaves the scan three waves per SIMD.  minWg = n asks the compiler
            // for n waves per SIMD (RSQ_MIN_WG, the launch bound's second argument: n resident 256-thread workgroups per CU; it spills
            // in stage 2 instead).
            const int minWg = 0;
            pipe.sourceLazy.replace(at, off.size(), "#define RSQ_LAZY 1\n" + (minWg ? "#define RSQ_MIN_WG " + std::to_string(minWg) + "\n" : std::string()));
        }
    }
    std::string ex = "pipeline " + std::to_string(q.pipelines.size()) + ": ";
    for (size_t i = 0; i < explainSteps.size(); i++) ex += (i ? " -> " : "") + explainSteps[i];
    if (pipe.lateLoads) {
        char buf[96];
        snprintf(buf, sizeof buf, " [late loads: ~%.1f %% of the rows expected to pass the leading selection]", leadPass * 100.0);
        ex += buf;
    }
    if (rowCells) ex += " [second form: rows into per-lane LDS cells, chosen by the executions' kernel times]";
    if (pipe.staged) ex += " [partitioned as packed " + std::to_string(8 * pipe.stagedRecWords) + "-byte records staged through LDS rings]";
    pipe.explain = ex;
    q.pipelines.push_back(pipe);
}

}  // namespace cg
}  // namespace rsq
