// engine.cpp — describe -> compile -> execute -> retrieve for one query
// (the call sequence of the reference's executeSelectPlan, reference src/execute.h:213-247).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <functional>
#include <sstream>

#include "engine_internal.h"

namespace rsq {

namespace {

// multiplicative inverse of an odd number modulo 2^64 (Newton: every step doubles the correct low bits)
uint64_t inverseOdd64(uint64_t a) { uint64_t x = a; for (int i = 0; i < 6; i++) x *= 2 - a * x; return x; }

// ================================================================================================
// plan construction + typing
// ================================================================================================
void buildOps(Query& q, const rsq_plan_desc& p) {
    int extra = 0;
    for (int i = 0; i < p.n_ops; i++) if (p.ops[i].tag == RSQ_OP_ORDERBY) extra++;
    for (int i = 0; i < p.n_ops + extra; i++) q.ops.emplace_back(new OpNode());
    int nextExtra = p.n_ops;
    for (int i = 0; i < p.n_ops; i++) {
        const rsq_op& d = p.ops[i];
        OpNode* o = q.ops[(size_t)i].get();
        o->tag = d.tag;
        if (d.n_exprs < 0 || d.n_exprs > RSQ_MAX_OP_EXPRS || d.n_exprs2 < 0 || d.n_exprs2 > RSQ_MAX_OP_EXPRS) failInvalid("bad expression count");
        for (int k = 0; k < d.n_exprs; k++) { if (d.exprs[k] < 0 || d.exprs[k] >= p.n_exprs) failInvalid("bad expression index"); o->exprs.push_back(q.exprs[(size_t)d.exprs[k]]); }
        for (int k = 0; k < d.n_exprs2; k++) { if (d.exprs2[k] < 0 || d.exprs2[k] >= p.n_exprs) failInvalid("bad expression index"); o->exprs2.push_back(q.exprs[(size_t)d.exprs2[k]]); }
        o->singleMatch = d.single_match != 0;
        switch (d.tag) {
            case RSQ_OP_SCAN:
                if (d.table < 0 || d.table >= (int)q.tables.size()) failInvalid("bad table index");
                o->table = q.tables[(size_t)d.table]; o->nChildren = 0; break;
            case RSQ_OP_HASHJOIN: o->nChildren = 2; if (d.n_exprs < 1) failInvalid("hash join needs an equality"); break;
            case RSQ_OP_SELECTION: if (d.n_exprs != 1) failInvalid("selection needs one condition"); o->nChildren = 1; break;
            case RSQ_OP_PROJECTION: case RSQ_OP_AGGREGATION: case RSQ_OP_MATERIALIZE: case RSQ_OP_ORDERBY: o->nChildren = 1; break;
            case RSQ_OP_NESTEDLOOPSJOIN:
                if (!(q.ctx.cfg.engine_flags & RSQ_ENGINE_NESTED_LOOPS)) failUnsupported("NestedLoopsJoin is outside the hot path (SURVEY §2)");
                if (d.n_exprs > 1) failInvalid("nested-loops join takes at most one condition");
                o->nChildren = 2; o->nlj = (int)q.nljs.size(); q.nljs.emplace_back(); q.nljs.back().op = o;
                break;
            default: failInvalid("unknown operator tag");
        }
        for (int k = 0; k < o->nChildren; k++) {
            int ci = d.child[k];
            if (ci < 0 || ci >= p.n_ops || ci == i) failInvalid("bad child operator index");
            o->child[k] = q.ops[(size_t)ci].get();
        }
        if (d.tag == RSQ_OP_ORDERBY) {   // OrderByOp wraps its child into a MaterializeOp (orderby.h:32-38)
            OpNode* m = q.ops[(size_t)nextExtra++].get();
            m->tag = RSQ_OP_MATERIALIZE; m->nChildren = 1; m->child[0] = o->child[0];
            o->child[0] = m;
        }
    }
    for (auto& o : q.ops)
        for (int k = 0; k < o->nChildren; k++) {
            if (o->child[k]->parent && o->child[k]->parent != o.get()) failInvalid("operator has two parents");
            o->child[k]->parent = o.get();
        }
    if (p.root < 0 || p.root >= p.n_ops) failInvalid("bad root");
    q.root = q.ops[(size_t)p.root].get();
    if (q.root->tag != RSQ_OP_MATERIALIZE && q.root->tag != RSQ_OP_ORDERBY)
        failInvalid("Calling retrieveResult on non-materialized operator");
    if (p.has_limit) { q.root->hasLimit = true; q.root->limit = p.limit; }
}

// defineExpressionsForPlan (RelOperator.h:203-208) + deriveExpressionTypes in definition order
void defineAndDerive(Query& q, OpNode* o) {
    for (int i = 0; i < o->nChildren; i++) defineAndDerive(q, o->child[i]);
    auto all = [&](std::vector<Expr*>& v) { for (Expr* e : v) q.pool.derive(e); };
    switch (o->tag) {
        case RSQ_OP_SCAN: case RSQ_OP_MATERIALIZE: break;
        case RSQ_OP_SELECTION: case RSQ_OP_PROJECTION: case RSQ_OP_HASHJOIN: case RSQ_OP_NESTEDLOOPSJOIN: all(o->exprs); break;
        case RSQ_OP_AGGREGATION:
            for (Expr* e : o->exprs) {
                if (e->tag == RSQ_E_AVG) {
                    o->splitAgg.push_back(q.pool.unary(RSQ_E_SUM, "sum", e->child));
                    o->splitAgg.push_back(q.pool.unary(RSQ_E_COUNT, "count", e->child));
                } else o->splitAgg.push_back(e);
            }
            all(o->exprs2); all(o->splitAgg); all(o->exprs);
            break;
        case RSQ_OP_ORDERBY:
            for (auto& e : o->exprs) if (e->tag != RSQ_E_ASC && e->tag != RSQ_E_DESC) e = q.pool.unary(RSQ_E_ASC, "asc", e);
            for (Expr* e : o->exprs)
                if (e->child->tag != RSQ_E_ATTRIBUTE) failType("Order by only supports attribute expressions currently." + serializeExpr(e->child));
            all(o->exprs);
            break;
        default: failInvalid("unsupported operator in plan");
    }
}

}  // namespace

// getSize() estimates (reference src/operators/*.h).  local: over this shard's own rows (sizing of the device's tables) instead of the
// whole table's (everything that replays the reference: its table sizes decide the emission order)
uint64_t opSize(OpNode* o, bool local) {
    switch (o->tag) {
        case RSQ_OP_SCAN:
            if (o->table->derived) return o->table->derivedEstimate;      // the replaced aggregation's estimate, not the rows it gave
            return (uint64_t)(local ? o->table->nRows : o->table->totalRows());      // a shard sizes like the table it is a range of (Table::nRowsTotal)
        case RSQ_OP_SELECTION: return opSize(o->child[0], local) / 2;
        case RSQ_OP_PROJECTION: case RSQ_OP_ORDERBY: return opSize(o->child[0], local);
        case RSQ_OP_HASHJOIN: return opSize(o->child[0], local) + opSize(o->child[1], local) / 2;
        case RSQ_OP_AGGREGATION: {
            if (o->exprs2.empty()) return 1;
            int red = 512;
            for (size_t i = 1; i < o->exprs2.size() && red > 2; i++) red /= 2;
            return opSize(o->child[0], local) / (uint64_t)red;
        }
        case RSQ_OP_MATERIALIZE: { uint64_t s = opSize(o->child[0], local); if (o->hasLimit && (uint64_t)o->limit < s) s = (uint64_t)o->limit; return s; }
        case RSQ_OP_NESTEDLOOPSJOIN: {            // nestedloopsjoin.h getSize
            const uint64_t l = opSize(o->child[0], local), r = opSize(o->child[1], local);
            return l + r <= 10000 ? l * r : (l + r) * 2;
        }
        default: return 0;
    }
}

Query::~Query() {
    if (bgCompiler.joinable()) bgCompiler.join();
    for (NljState& n : nljs) n.sub.freeColumns(ctx);
    for (DerivedState& d : derived) { d.sub.freeColumns(ctx); if (d.dTuples) ctx.free(d.dTuples); if (d.dMerge) ctx.free(d.dMerge); }
    destroyTailState(tailState);
    if (dtArena.dev || dtArena.pinned) {
        // the arenas go back to the context for the next query, unless it already holds a pair
        if (!ctx.spareTailArena.dev && !ctx.spareTailArena.pinned) ctx.spareTailArena = dtArena;
        else { if (dtArena.dev) ctx.free(dtArena.dev); if (dtArena.pinned) ctx.freePinned(dtArena.pinned); }
    }
    if (rtDev) ctx.free(rtDev);
    if (rtPinned) ctx.freePinned(rtPinned);
    if (dGenericCode) ctx.free(dGenericCode);
    for (auto& gp : generic2Progs) { if (gp.dCode) ctx.free(gp.dCode); if (gp.dProbes) ctx.free(gp.dProbes); if (gp.dConstPool) ctx.free(gp.dConstPool); }
    if (dG2Cnt) ctx.free(dG2Cnt);
    if (dG2Offs) ctx.free(dG2Offs);
    if (dG2ScanTemp) ctx.free(dG2ScanTemp);
    if (dAgg && dAggOwned) ctx.free(dAgg);
    if (dAggInit) ctx.free(dAggInit);
    if (dAggWork) ctx.free(dAggWork);
    if (dAggWorkInit) ctx.free(dAggWorkInit);
    if (hPinned) ctx.freePinned(hPinned);
    if (hGroupRows) ctx.freePinned(hGroupRows);
    if (hCandRows) ctx.freePinned(hCandRows);
    if (dFinTicket) ctx.free(dFinTicket);
    // (events not read yet belong to work that may still run: they go back to the pool all the same - a record on a recorded event
    // simply replaces it, and nobody reads the old pair any more)
    ctx.giveEvent(gev0); ctx.giveEvent(gev1);
    for (auto& e : evRing) { ctx.giveEvent(e.first); ctx.giveEvent(e.second); }
    if (dMatCnt) ctx.free(dMatCnt);
    if (dMatOffs) ctx.free(dMatOffs);
    if (dMatTileCnt) ctx.free(dMatTileCnt);
    if (dScanTemp) ctx.free(dScanTemp);
    freeMatCols(*this);
    if (dGroupRows) ctx.free(dGroupRows);
    if (dNarrowRows) ctx.free(dNarrowRows);
    if (hInlineRows) ctx.freePinned(hInlineRows);
    if (dPipeStats) ctx.free(dPipeStats);
    if (dGroupCount) ctx.free(dGroupCount);
    releaseMaterializeTails(*this);
    if (dTopkImages) ctx.free(dTopkImages);
    if (dTopkHists) ctx.free(dTopkHists);
    if (dCandRows) ctx.free(dCandRows);
    if (dPartCounts) ctx.free(dPartCounts);
    if (dPartStart) ctx.free(dPartStart);
    if (dDebugStamps) ctx.free(dDebugStamps);
    if (dStageBase) ctx.free(dStageBase);
    if (dStageCap) ctx.free(dStageCap);
    if (dStageCtl) ctx.free(dStageCtl);
    if (hStageLayout) ctx.freePinned(hStageLayout);
    if (dStageCounts) ctx.free(dStageCounts);
    if (dPartTotals) ctx.free(dPartTotals);
    for (void* r : dPartRecords) if (r) ctx.scratchFree(r);
    for (auto& h : hashTables) {
        if (h->dState) ctx.free(h->dState);
        if (h->dWords) ctx.free(h->dWords);
        if (h->dAcc) ctx.free(h->dAcc);
        if (h->dCount) ctx.free(h->dCount);
        if (h->keyIndex) ctx.releaseKeyIndex(h->keyIndex);      // (the bitmap is the context's key index then)
        else if (h->dBitmap) ctx.free(h->dBitmap);
        if (h->dCompBitmap) ctx.free(h->dCompBitmap);
        if (h->dDeref) ctx.free(h->dDeref);
        if (h->dTemp) ctx.free(h->dTemp);
        if (h->dTempUsed) ctx.free(h->dTempUsed);
        if (h->dChunkTotal) ctx.free(h->dChunkTotal);
        if (h->dChunkBase) ctx.free(h->dChunkBase);
    }
}

// ================================================================================================
// compile
// ================================================================================================
bool denseMode(const Query& q) {
    return q.aggMode == AggMode::DENSE_REG || q.aggMode == AggMode::DENSE_LDS_PRIVATE ||
           q.aggMode == AggMode::DENSE_LDS_SHARED || q.aggMode == AggMode::DENSE_GLOBAL;
}

// A dense table that other ranks' tables may be merged into: not one keyed by a dictionary code.  The dictionary is this process's own
// (another rank's holds other values under the same codes), so the partial entry points - execute_partial*, partial_layout, bind_partial,
// merge_gathered, finalize* - answer such a statement as they answer the hash aggregation it was before the codes became ranks.
// Unless every coded key's dictionary is the one all shards hold (DenseKey::shared, unifyShardDictionaries): then a rank is the same value
// everywhere, and the table merges like any other (rsq_multi_query_compile compares the shards' dictionaries once more: queryPartialLayoutText).
static bool partialCapable(const Query& q) {
    if (!denseMode(q)) return false;
    for (auto& k : q.denseKeys) if (k.coded && !k.shared) return false;
    return true;
}

// Device-resident identity image of the dense aggregate table (0 for sums, +/-inf for min/max) and a pinned
// host buffer for the read-back: one execute is then {D2D init, kernel(s), D2H} on one stream with a single
// host synchronisation at the end.
static void prepareDenseBuffers(Query& q) {
    const int64_t D = q.denseGroups;
    const size_t words = q.accums.size() * (size_t)D;
    std::vector<uint64_t> init(words);
    for (size_t w = 0; w < q.accums.size(); w++) {
        uint64_t idv = q.accums[w].merge == 0 ? 0ull : q.accums[w].merge == 2 ? 0x7fffffffffffffffull : 0x8000000000000000ull;
        for (int64_t g = 0; g < D; g++) init[(size_t)(q.accumSlot[w] * D + g)] = idv;
    }
    q.dAgg = (uint64_t*)q.ctx.alloc(words * 8);
    q.dAggInit = (uint64_t*)q.ctx.alloc(words * 8);
    RSQ_HIP(hipMemcpy(q.dAggInit, init.data(), words * 8, hipMemcpyHostToDevice));
    q.hAgg.assign(words, 0);
    q.pinnedWords = words;
    q.tableWords = words;
    if (q.aggPad > 1) {
        // padded working table (one cell per 64-byte line) the register-mode kernels flush into
        q.padWords = words * (size_t)q.aggPad;
        std::vector<uint64_t> pinit(q.padWords + 1, 0);        // + one word: the device error word of graph replays
        for (size_t i = 0; i < words; i++) pinit[i * (size_t)q.aggPad] = init[i];
        q.dAggWork = (uint64_t*)q.ctx.alloc((q.padWords + 1) * 8);
        q.dAggWorkInit = (uint64_t*)q.ctx.alloc((q.padWords + 1) * 8);
        RSQ_HIP(hipMemcpy(q.dAggWorkInit, pinit.data(), (q.padWords + 1) * 8, hipMemcpyHostToDevice));
        q.pinnedWords = q.padWords;          // the read-back of a full execution takes the padded table
    }
}

// every kernel source a query's execution may need right away (lazily chosen forms are compiled when first chosen).
// quick: the tier a statement with a cold code-object cache runs on first - the pipelines that have a stage 2 with RSQ_STAGE2_CALL
// (stage 2 a real call instead of inlined at every drain site: a third of the compile time, 40-65 % slower to run; codegen_loop.cpp)
std::string tierSource(const Pipeline& p, const std::string& source, bool quick) {
    return quick && p.hasStage2 ? "#define RSQ_STAGE2_CALL 1\n" + source : source;
}
static std::vector<std::string> kernelSources(const Query& q, bool quick = false) {
    std::vector<std::string> v;
    for (auto& p : q.pipelines) {
        auto T = [&](const std::string& s) { return tierSource(p, s, quick); };
        if (!p.sourcePass1.empty()) v.push_back(T(p.sourcePass1));
        if (!p.sourceFlat.empty()) v.push_back(T(p.sourceFlat));
        if (p.partitioned) { v.push_back(T(p.sourcePartCount)); v.push_back(T(p.sourcePartScatter)); v.push_back(p.sourcePartAgg); }
        if (p.staged) { v.push_back(T(p.sourceStagedScatter)); v.push_back(p.sourceStagedAgg); }
        v.push_back(T(p.source));
        if (!p.sourceCells.empty()) v.push_back(T(p.sourceCells));              // (the second form of a register aggregation: compiled with the first, chosen per execution)
        if (!p.sourceFlatCells.empty()) v.push_back(T(p.sourceFlatCells));
        if (!p.sourceLazy.empty()) v.push_back(T(p.sourceLazy));      // (chosen at run time; compiled with the others so that choosing it never blocks an execution)
        // ... and so is the 64-slot front table of a hash aggregation that turns out to have a handful of groups (engine_pipelines.cpp
        // fewGroupsKernel): compiled when first wanted it cost TPC-H Q12's second query 0.57 s of hiprtc in the middle of an execution
        if (p.ldsSlots > 64 && q.aggMode == AggMode::HASH && p.sink == SinkKind::AGGREGATE && q.aggTable >= 0) {
            v.push_back(T("#define RSQ_LC_SLOTS 64\n" + p.source));
            if (!p.sourceLazy.empty()) v.push_back(T("#define RSQ_LC_SLOTS 64\n" + p.sourceLazy));
        }
    }
    return v;
}
static void resolveKernels(Query& q, bool quick = false) {
    Context& ctx = q.ctx;
    // (compiling a query's kernels on one host thread each was tried: hiprtc serialises internally, TPC-H Q3's three kernels took
    // 548 ms in parallel against 448 ms one after the other.  What is not in the cache is therefore compiled in helper PROCESSES
    // first, all at once - runtime.cpp compileManyToCache - and the loop below finds it there)
    ctx.compileManyToCache(kernelSources(q, quick));
    q.quickTier = quick;
    for (auto& p : q.pipelines) {
        auto T = [&](const std::string& s) { return tierSource(p, s, quick); };
        p.fewGroupKernels.clear();                // (kernels of the other tier)
        if (!p.sourcePass1.empty()) p.kernelPass1 = &ctx.getKernel(T(p.sourcePass1), p.entry);
        if (!p.sourceFlat.empty()) p.kernelFlat = &ctx.getKernel(T(p.sourceFlat), p.entry);
        if (p.partitioned) {
            p.kernelPartCount = &ctx.getKernel(T(p.sourcePartCount), p.entry);
            p.kernelPartScatter = &ctx.getKernel(T(p.sourcePartScatter), p.entry);
            p.kernelPartAgg = &ctx.getKernel(p.sourcePartAgg, "rsq_part_agg");
        }
        if (p.staged) {
            p.kernelStagedScatter = &ctx.getKernel(T(p.sourceStagedScatter), p.entry);
            p.kernelStagedAgg = &ctx.getKernel(p.sourceStagedAgg, "rsq_staged_agg");
        }
        p.kernel = &ctx.getKernel(T(p.source), p.entry);
        if (!p.sourceCells.empty()) p.kernelCells = &ctx.getKernel(T(p.sourceCells), p.entry);
        if (!p.sourceFlatCells.empty()) p.kernelFlatCells = &ctx.getKernel(T(p.sourceFlatCells), p.entry);
        // both forms are loaded now: the first execution that chooses the late-load form must not read and load a code object
        // (TPC-H Q3 at SF10: 0.86 ms for the execution that first chose it, 0.32 ms after)
        if (!p.sourceLazy.empty()) p.kernelLazy = &ctx.getKernel(T(p.sourceLazy), p.entry);
        if (ctx.device < 0 && p.ldsSlots > 64 && q.aggMode == AggMode::HASH && p.sink == SinkKind::AGGREGATE && q.aggTable >= 0) {      // build(): the few-groups forms too
            (void)ctx.getKernel("#define RSQ_LC_SLOTS 64\n" + p.source, p.entry);
            if (!p.sourceLazy.empty()) (void)ctx.getKernel("#define RSQ_LC_SLOTS 64\n" + p.sourceLazy, p.entry);
        }
    }
}


// ================================================================================================
// the context's plan memo (engine.h Context::PlanMemo)
// ================================================================================================
static uint64_t fnv1a64(const std::string& s, uint64_t h = 1469598103934665603ull) {
    for (unsigned char c : s) { h ^= c; h *= 1099511628211ull; }
    return h;
}
// (kernel texts - they carry every constant of the plan and everything the planner took from the column statistics -, then identity
// and version of every table in plan order)
static std::string planMemoKey(const Query& q) {
    uint64_t h = 1469598103934665603ull;
    for (auto& p : q.pipelines) h = fnv1a64(p.source, h) * 0x9E3779B97F4A7C15ull;
    std::string k = std::to_string(h);
    if (q.maxGrid) k += "|g" + std::to_string(q.maxGrid);      // (RSQ_MAX_GRID: what a query learnt under one grid - staged regions per workgroup - is not another's)
    for (Table* t : q.tables) k += "|" + std::to_string(t->uid) + "." + std::to_string(t->version) + "." + std::to_string(t->nRows) + "." + std::to_string(t->row0) + "." + std::to_string(t->nRowsTotal);
    return k;
}

// a freshly compiled query takes what an earlier one with the same key has learnt: its join tables are sized and allocated (no counting
// pass, no read-back), its hash aggregation starts with the table that held the groups, late-load / staged / materialisation choices and
// the forms that timed out once are the earlier query's.  Runs at compile time, where the arenas make the allocations cheap.
static void applyPlanMemo(Query& q) {
    Context& ctx = q.ctx;
    if (ctx.planMemoOff || ctx.device < 0 || q.genericActive) return;
    if (!q.derived.empty()) return;          // (what this query learns depends on the derived tables' rows: no memo entry, no key)
    q.memoKey = planMemoKey(q);
    auto it = ctx.planMemo.find(q.memoKey);
    if (it == ctx.planMemo.end()) return;
    Context::PlanMemo& m = it->second;
    if (m.joins.size() != q.hashTables.size() || m.pipes.size() != q.pipelines.size()) return;
    m.stamp = ++ctx.planMemoClock;
    for (size_t i = 0; i < q.pipelines.size(); i++) {
        Pipeline& p = q.pipelines[i];
        p.stage2Rows = m.pipes[i].stage2Rows;
        if (!p.sourceCells.empty()) p.cellsChoice = m.pipes[i].cellsChoice;
        p.stagedExact = m.pipes[i].stagedExact; p.stagedCaps = m.pipes[i].stagedCaps; p.stagedCapsRows = m.pipes[i].stagedCapsRows;
        if (p.sink != SinkKind::BUILD) continue;
        HashTable& h = *q.hashTables[(size_t)p.buildTable];
        const Context::PlanMemo::Join& j = m.joins[(size_t)p.buildTable];
        if (j.buildRows < 0 || h.capacity != 0) continue;
        sizeJoinTable(q, p, h, (uint32_t)j.buildRows, j.dupKeys);
    }
    for (size_t i = 0; i < q.hashTables.size(); i++) q.hashTables[i]->lastCount = m.joins[i].lastCount;
    if (q.aggMode == AggMode::HASH && q.aggTable >= 0 && m.hashCapacity > 0) {
        HashTable& h = *q.hashTables[(size_t)q.aggTable];
        if (h.capacity == 0 && !h.dState) {
            h.capacity = m.hashCapacity; h.lastCount = m.hashCount;
            h.dState = (uint32_t*)ctx.alloc((size_t)h.capacity * 4);
            h.dWords = (int64_t*)ctx.alloc((size_t)h.capacity * 8 * (h.keys.size() + h.payload.size()));
            h.dAcc = (int64_t*)ctx.alloc((size_t)h.capacity * 8 * (size_t)h.nAccBlocks);
        }
        q.charGroupsNeedMerge = m.charGroupsNeedMerge;
        for (auto& p : q.pipelines)         // a handful of groups: the 64-slot front table's kernel is loaded now (engine_pipelines.cpp fewGroupsKernel)
            if (p.sink == SinkKind::AGGREGATE) {
                const bool lazy = !p.sourceLazy.empty() && p.stage2Rows >= 0 && p.stage2Rows * 32 < p.src->nRows;
                (void)fewGroupsKernel(q, p, lazy ? p.sourceLazy : p.source, lazy ? "lazy" : "eager", lazy ? p.kernelLazy : p.kernel);
            }
    }
    q.matLastTotal = m.matLastTotal;
    if (q.matOp && !q.agg && m.matLastTotal >= 0) {
        uint64_t keep = (uint64_t)m.matLastTotal;
        if (q.matOp->hasLimit) keep = std::min<uint64_t>(keep, (uint64_t)std::max<int64_t>(q.matOp->limit, 1));
        if (q.dMatCols.empty()) allocMatCols(q, std::max<int64_t>((int64_t)keep, 1));
    }
    q.narrowRowsOff = m.narrowRowsOff; q.fusedSelectOff = m.fusedSelectOff; q.chainedIndexOff = m.chainedIndexOff; q.scanChainedOff = m.scanChainedOff;
    q.stageWorkgroups = m.stageWorkgroups;
    q.memoApplied = true;
    ctx.planMemoHits++;
}

// after an execution that ran to its end: the key bitmaps of its direct join tables stay as they are for the next execution, and go to the
// context for every other query over the same table version (Context::keyIndexes)
static void keepKeyIndexes(Query& q) {
    Context& ctx = q.ctx;
    if (q.genericActive) return;
    for (auto& p : q.pipelines) {
        if (p.sink != SinkKind::BUILD) continue;
        HashTable& h = *q.hashTables[(size_t)p.buildTable];
        if (!h.direct || h.dense || !h.rank || !h.dBitmap || h.directKeyCol < 0 || h.directSrc != p.src) continue;
        if (!h.keyIndexReady) { h.keyIndexReady = true; h.keyIndexVersion = p.src->version; }
        if (h.keyIndex || ctx.planMemoOff || h.keyIndexVersion != p.src->version) continue;
        const Context::KeyIndexKey key{p.src->uid, p.src->version, p.src->nRows, p.src->row0, h.directKeyCol};
        if (ctx.keyIndexes.count(key)) continue;      // (another query was first: this one keeps its own)
        Context::KeyIndex& k = ctx.keyIndexes[key];
        k.dBitmap = h.dBitmap; k.bmBlocks = h.bmBlocks; k.bmMin = h.bmMin; k.bmBits = h.bmBits; k.refs = 1; k.uid = p.src->uid;
        h.keyIndex = &k;
    }
}

// after an execution that ran to its end: what it knows now
static void rememberPlan(Query& q) {
    Context& ctx = q.ctx;
    if (ctx.planMemoOff || q.memoKey.empty() || q.genericActive) return;
    Context::PlanMemo& m = ctx.planMemo[q.memoKey];
    m.stamp = ++ctx.planMemoClock;
    m.joins.resize(q.hashTables.size()); m.pipes.resize(q.pipelines.size());
    for (size_t i = 0; i < q.hashTables.size(); i++) {
        const HashTable& h = *q.hashTables[i];
        m.joins[i].buildRows = h.capacity != 0 ? h.buildRows : -1; m.joins[i].dupKeys = h.dupKeys; m.joins[i].lastCount = h.lastCount;
    }
    for (size_t i = 0; i < q.pipelines.size(); i++) {
        const Pipeline& p = q.pipelines[i];
        Context::PlanMemo::Pipe& mp = m.pipes[i];
        mp.cellsChoice = p.cellsChoice;
        mp.stage2Rows = p.stage2Rows; mp.stagedExact = p.stagedExact; mp.stagedCapsRows = p.stagedCapsRows;
        if (mp.stagedCaps != p.stagedCaps) mp.stagedCaps = p.stagedCaps;
    }
    if (q.aggMode == AggMode::HASH && q.aggTable >= 0) {
        const HashTable& h = *q.hashTables[(size_t)q.aggTable];
        m.hashCapacity = h.dState ? h.capacity : 0; m.hashCount = h.lastCount; m.charGroupsNeedMerge = q.charGroupsNeedMerge;
    }
    m.matLastTotal = q.matLastTotal;
    m.narrowRowsOff = q.narrowRowsOff; m.fusedSelectOff = q.fusedSelectOff; m.chainedIndexOff = q.chainedIndexOff; m.scanChainedOff = q.scanChainedOff;
    m.stageWorkgroups = q.stageWorkgroups;
    if (ctx.planMemo.size() > 512) {          // the least recently used half goes
        std::vector<std::pair<uint64_t, std::string>> byAge;
        for (auto& kv : ctx.planMemo) byAge.emplace_back(kv.second.stamp, kv.first);
        std::sort(byAge.begin(), byAge.end());
        for (size_t i = 0; i < byAge.size() / 2; i++) ctx.planMemo.erase(byAge[i].second);
    }
}

// A sub-query (engine_internal.h SubQuery): the subtree under plan op `at` under a MATERIALIZE (the reference's own wrapper where the
// subtree's root is one), every attribute, no limit - a plan description of its own, compiled as a query of its own.  The copy keeps the
// plan's op order (children first), which fixes the sub-query's expression ids and hence its kernel text.
static Query* compileSubQuery(Context& ctx, const rsq_plan_desc& plan, int at, rsq_table* const* tables, int nTables) {
    std::vector<rsq_op> ops;
    std::map<int, int> remap;
    std::function<int(int)> copy = [&](int i) -> int {
        auto it = remap.find(i);
        if (it != remap.end()) return it->second;
        rsq_op d = plan.ops[i];
        for (int k = 0; k < 2; k++) if (d.child[k] >= 0) d.child[k] = copy(d.child[k]);
        ops.push_back(d);
        return remap[i] = (int)ops.size() - 1;
    };
    int root = copy(at);
    if (ops[(size_t)root].tag != RSQ_OP_MATERIALIZE) {
        rsq_op m;
        memset(&m, 0, sizeof m);
        m.tag = RSQ_OP_MATERIALIZE; m.child[0] = root; m.child[1] = -1; m.table = -1;
        ops.push_back(m);
        root = (int)ops.size() - 1;
    }
    rsq_plan_desc sub = plan;
    sub.ops = ops.data(); sub.n_ops = (int32_t)ops.size(); sub.root = root;
    sub.request_all = 1; sub.has_limit = 0; sub.limit = 0;
    Query* q = compileQuery(ctx, sub, tables, nTables);
    q->subQuery = true;          // (rsq_ctx_set_result_pack: its columns or host tuples are what the outer statement reads)
    return q;
}

// The inner side of a nested-loops join: the sub-query of its left subtree
static void compileNestedLoopsInner(Query& q, NljState& n, const rsq_plan_desc& plan, rsq_table* const* tables, int nTables) {
    int left = -1;
    for (int i = 0; i < plan.n_ops; i++) if (q.ops[(size_t)i].get() == n.op) left = plan.ops[i].child[0];
    if (left < 0) failInvalid("nested-loops join without a left child");
    n.sub.query.reset(compileSubQuery(q.ctx, plan, left, tables, nTables));
}

// Derived aggregations (engine_internal.h DerivedState): every AGGREGATION with an ancestor other than PROJECTION / MATERIALIZE / ORDERBY
// and no such aggregation above it is cut out as a sub-query, which compiles the aggregations below it the same way.  The node becomes a scan of the derived table.
static bool isDerivedAggregation(const OpNode* o) {
    if (o->tag != RSQ_OP_AGGREGATION) return false;
    for (const OpNode* a = o->parent; a; a = a->parent)
        if (a->tag != RSQ_OP_PROJECTION && a->tag != RSQ_OP_MATERIALIZE && a->tag != RSQ_OP_ORDERBY) return true;
    return false;
}

static std::string derivedName(const std::vector<Expr*>& groups) {
    std::string g;
    for (Expr* e : groups) g += (g.empty() ? "" : ", ") + expressionName(e);
    return "the derived aggregation grouped by [" + g + "]";
}

static void compileDerived(Query& q, const rsq_plan_desc& plan, rsq_table* const* tables, int nTables) {
    std::vector<int> cut;
    for (int i = 0; i < plan.n_ops; i++) {
        OpNode* o = q.ops[(size_t)i].get();
        if (!isDerivedAggregation(o)) continue;
        if (!q.nljs.empty()) failUnsupported(derivedName(o->exprs2) + ": a derived aggregation inside a nested-loops plan");
        bool top = true;
        for (OpNode* a = o->parent; a; a = a->parent) if (isDerivedAggregation(a)) top = false;      // (that one's sub-query cuts this one)
        if (top) cut.push_back(i);
    }
    for (int i : cut) {
        OpNode* o = q.ops[(size_t)i].get();
        DerivedState d;
        d.op = o; d.groups = o->exprs2; d.aggs = o->exprs;
        const uint64_t estimate = opSize(o);      // (operators above size their tables from it, as the reference's do)
        d.sub.query.reset(compileSubQuery(q.ctx, plan, i, tables, nTables));
        Query& s = *d.sub.query;
        if (s.agg == nullptr) failInvalid("derived aggregation without an aggregation");
        // mergeAverages names an AVG when the aggregation's rows are made (tail.cpp): its id is taken now, so that the counter this
        // query continues from (Walker::produceScan) has counted it
        for (Expr* a : s.agg->exprs) if (a->tag == RSQ_E_AVG) s.pool.addId(a);
        d.table.reset(new Table());
        Table& t = *d.table;
        t.ctx = &q.ctx; t.derived = true; t.derivedEstimate = estimate;
        t.name = "derived" + std::to_string(q.derived.size());
        for (Expr* g : d.groups) { TableColumn c; c.type = g->type; t.cols.push_back(c); }
        for (Expr* a : d.aggs) { TableColumn c; c.type = a->type; t.cols.push_back(c); }
        if (t.cols.size() > 32) failUnsupported(derivedName(d.groups) + " has more than 32 columns");
        for (auto& c : t.cols) (void)columnWidth(c.type);
        // the node is a scan from now on (DerivedState keeps its expressions: they name the columns)
        o->tag = RSQ_OP_SCAN; o->nChildren = 0; o->child[0] = o->child[1] = nullptr; o->table = &t;
        o->exprs.clear(); o->exprs2.clear(); o->splitAgg.clear();
        o->derived = (int)q.derived.size();
        q.derived.push_back(std::move(d));
    }
}

// The reference numbers expressions with one counter in produce order, and the derived aggregation's subtree is produced where its scan
// now stands: the sub-query's names continue this query's counter from here (the `exprN` of an aggregate above it, the fixtures'
// #schema lines), and the columns take the names this query knows the aggregation's outputs by.
void nameDerivedColumns(Query& q, OpNode* scan) {
    DerivedState& d = q.derived[(size_t)scan->derived];
    if (d.named) return;
    d.named = true;
    Query& s = *d.sub.query;
    const size_t base = (size_t)q.pool.exprIdGen - 1;
    for (size_t i = 0; i < q.exprs.size() && i < s.exprs.size(); i++)
        if (s.exprs[i]->id != 0 && q.exprs[i]->id == 0) q.exprs[i]->id = s.exprs[i]->id + base;
    q.pool.exprIdGen += s.pool.exprIdGen - 1;                       // (both counters start at 1)
    Table& t = *d.table;
    size_t k = 0;
    for (Expr* g : d.groups) t.cols[k++].name = expressionName(g);
    for (Expr* a : d.aggs) t.cols[k++].name = expressionName(a);
}

void refuseDerived(const Query& q, const std::string& what) {
    failUnsupported(what + " of a plan with " + derivedName(q.derived.at(0).groups) + " (" + q.derived[0].table->name + "): only whole executions on one context run derived tables");
}

bool queryHasDerived(const Query& q) {
    if (!q.derived.empty()) return true;
    for (const NljState& n : q.nljs) if (n.sub.query && queryHasDerived(*n.sub.query)) return true;
    return false;
}

Query* compileQuery(Context& ctx, const rsq_plan_desc& plan, rsq_table* const* tables, int nTables) {
    double t0 = nowMs();
    std::unique_ptr<Query> q(new Query(ctx));
    int hits0 = ctx.jitCacheHits, comp0 = ctx.jitCompiles;
    q->maxGrid = (unsigned)sw::num<sw::RSQ_MAX_GRID>();
    for (int i = 0; i < nTables; i++) {
        Table* t = reinterpret_cast<Table*>(tables[i]);
        if (!t) failInvalid("null table");
        q->tables.push_back(t);
        q->tableLayouts.push_back(t->layoutVersion);
        for (auto& c : t->cols) q->pool.identTypes[c.name] = c.type;
    }
    q->requestAll = plan.request_all != 0;
    q->exprs = q->pool.build(plan);
    buildOps(*q, plan);
    defineAndDerive(*q, q->root);
    compileDerived(*q, plan, tables, nTables);
    // (a join in the left subtree of another one belongs to that one's inner query, which compiles it itself)
    for (NljState& n : q->nljs) {
        bool inInner = false;
        for (OpNode* c = n.op; c->parent; c = c->parent)
            if (c->parent->tag == RSQ_OP_NESTEDLOOPSJOIN && c->parent->child[0] == c) inInner = true;
        if (!inInner) {
            compileNestedLoopsInner(*q, n, plan, tables, nTables);
            // The reference numbers expressions with one counter in produce order, and NestedLoopsJoinOp produces its left child first:
            // the names of this query's expressions (`exprN` of an aggregate's column) come after the inner side's
            q->pool.exprIdGen += n.sub.query->pool.exprIdGen - 1;        // (both counters start at 1)
        }
    }
    const double tBuilt0 = nowMs();
    buildPipelines(*q);
    planMaterializeTails(*q);
    const double tBuilt = nowMs();
    // A plan shape whose specialised kernels are not in the code-object cache starts on the pre-compiled generic pipeline
    // (generic.cpp) while hiprtc builds them on a host thread; RSQ_FORCE_GENERIC=1 keeps every eligible plan there (tests),
    // RSQ_GENERIC=0 restores the blocking compile.
    const bool forceGeneric = sw::flag<sw::RSQ_FORCE_GENERIC>();
    const bool allowGeneric = ctx.device >= 0 && sw::flag<sw::RSQ_GENERIC>();
    bool cached = true;
    if (allowGeneric) for (const std::string& src : kernelSources(*q)) cached = cached && ctx.kernelCached(src);
    traceLine("[rsq trace] compile: code-object cache looked up at +%.3f ms\n", nowMs() - tBuilt);
    if (allowGeneric && (forceGeneric || !cached)) {
        std::string why, why2;
        bool ok = buildGenericProgram(*q, q->generic, why);
        if (ok) {
            q->dGenericCode = (GenericInstr*)ctx.alloc(std::max<size_t>(1, q->generic.code.size()) * sizeof(GenericInstr));
            RSQ_HIP(hipMemcpy(q->dGenericCode, q->generic.code.data(), q->generic.code.size() * sizeof(GenericInstr), hipMemcpyHostToDevice));
            q->explainText += "generic pre-compiled pipeline (" + std::to_string(q->generic.code.size()) + " instructions, " + std::to_string(q->generic.cols.size()) +
                              " columns)" + (forceGeneric ? " forced" : " until hiprtc has built the specialised kernel") + "\n";
        } else if (sw::flag<sw::RSQ_GENERIC2>() && buildGenericPlan(*q, q->generic2Progs, why2)) {
            // joins, strings, hash aggregation, materialisation: the interpreter for whole pipelines, one program per pipeline
            ok = true; q->generic2 = true;
            size_t instr = 0;
            traceLine("[rsq trace] compile: interpreter programs built at +%.3f ms\n", nowMs() - tBuilt);
            for (auto& gp : q->generic2Progs) {
                instr += gp.code.size();
                gp.dCode = (GenericInstr*)ctx.alloc(std::max<size_t>(1, gp.code.size()) * sizeof(GenericInstr));
                RSQ_HIP(hipMemcpy(gp.dCode, gp.code.data(), gp.code.size() * sizeof(GenericInstr), hipMemcpyHostToDevice));
                gp.dProbes = (GenericProbeDesc*)ctx.alloc(std::max<size_t>(1, gp.probes.size()) * sizeof(GenericProbeDesc));
                if (!gp.probes.empty()) RSQ_HIP(hipMemcpy(gp.dProbes, gp.probes.data(), gp.probes.size() * sizeof(GenericProbeDesc), hipMemcpyHostToDevice));
                gp.dConstPool = (char*)ctx.alloc(std::max<size_t>(8, gp.constPool.size()));
                if (!gp.constPool.empty()) RSQ_HIP(hipMemcpy(gp.dConstPool, gp.constPool.data(), gp.constPool.size(), hipMemcpyHostToDevice));
            }
            for (auto& h : q->hashTables) q->savedAos.push_back(h->aos);
            traceLine("[rsq trace] compile: interpreter programs on the device at +%.3f ms\n", nowMs() - tBuilt);
            q->explainText += "generic pre-compiled interpreter for " + std::to_string(q->generic2Progs.size()) + " pipeline(s) (" + std::to_string(instr) +
                              " instructions)" + (forceGeneric ? " forced" : " until hiprtc has built the specialised kernels") + "\n";
        } else if (!why2.empty()) traceLine("[rsq trace] not interpreted: %s\n", why2.c_str());
        if (ok) {
            q->genericActive = true; q->genericForced = forceGeneric;
            if (!cached) {
                (void)ctx.cacheKey("");            // fills the header text the compiler thread reads
                const std::vector<std::string> sources = kernelSources(*q);
                // ... in two tiers where a pipeline has a stage 2: the quick tier's kernels first (ready in a third of the time: the
                // executions leave the interpreter for them), then the full ones (the executions move on to those when they are ready)
                bool twoTiers = false;
                for (auto& p : q->pipelines) twoTiers = twoTiers || p.hasStage2;
                const std::vector<std::string> quick = twoTiers ? kernelSources(*q, true) : std::vector<std::string>();
                Query* qp = q.get();
                q->bgState = 1;
                q->bgCompiler = std::thread([qp, sources, quick] {
                    // (one helper process per kernel: hiprtc serialises inside a process.  Both tiers' helpers start together - the quick
                    // tier is ready after its own slowest kernel, not after the full tier's)
                    std::string fullError;
                    std::thread full([&] {
                        try { qp->ctx.compileManyToCache(sources); }
                        catch (const std::exception& e) { fullError = e.what(); if (fullError.empty()) fullError = "kernel compilation failed"; }
                    });
                    try {
                        if (!quick.empty()) { qp->ctx.compileManyToCache(quick); qp->bgState = 2; }
                        full.join();
                        if (!fullError.empty()) throw Error(RSQ_ERR_DEVICE, fullError);
                        qp->bgState = 4;
                    }
                    catch (const std::exception& e) { if (full.joinable()) full.join(); qp->bgError = e.what(); qp->bgState = 3; }
                });
            }
        }
    }
    const double tGeneric = nowMs();
    if (!q->genericActive) resolveKernels(*q);
    traceLine("[rsq trace] compile: typing %.3f ms, pipelines + kernel text %.3f ms, cache lookup + interpreter programs %.3f ms, kernels %.3f ms\n",
              tBuilt0 - t0, tBuilt - tBuilt0, tGeneric - tBuilt, nowMs() - tGeneric);
    for (auto& p : q->pipelines) {
        q->allSource += p.source + "\n";
        q->explainText += p.explain + "\n";
    }
    if (denseMode(*q)) {
        // layout of the (partial) aggregate table, for hosts that merge it across GPUs
        std::ostringstream d;
        d << "partial table: groups=" << q->denseGroups << " keys=[";
        for (size_t i = 0; i < q->denseKeys.size(); i++) {
            const DenseKey& k = q->denseKeys[i];
            d << (i ? " x " : "") << k.expr->symbol;
            if (k.coded) d << "{dictionary code, " << k.card << (k.card == 1 ? " entry}" : " entries}");
            else if (k.byteSet) { d << "{"; for (size_t v = 0; v < k.values.size(); v++) d << (v ? "," : "") << (int)k.values[v]; d << "}"; }
            else d << "[" << k.min << ".." << (k.min + k.card - 1) << "]";
        }
        d << "] blocks=[";
        std::vector<std::string> names(q->accums.size());
        for (size_t w = 0; w < q->accums.size(); w++)
            names[(size_t)q->accumSlot[w]] = std::string(q->accums[w].merge == 0 ? "sum:" : q->accums[w].merge == 2 ? "min:" : "max:") + q->accums[w].key;
        for (size_t b = 0; b < names.size(); b++) d << (b ? " | " : "") << names[b];
        d << "] (word = block * groups + group)";
        q->explainText += d.str() + "\n";
    }
    for (size_t i = 0; i < q->derived.size(); i++) {
        const DerivedState& d = q->derived[i];
        std::string cols;
        for (auto& c : d.table->cols) cols += (cols.empty() ? "" : "|") + c.name + ":" + serializeType(c.type);
        q->explainText += "derived table " + d.table->name + " (" + derivedName(d.groups).substr(4) + ", estimate " + std::to_string(d.table->derivedEstimate) +
                          " rows, columns " + cols + ", row count and addresses bound per execution) from its sub-query:\n";
        std::istringstream in(d.sub.query->explainText);
        for (std::string l; std::getline(in, l);) q->explainText += "  | " + l + "\n";
    }
    if (ctx.device >= 0) {
        if (denseMode(*q)) prepareDenseBuffers(*q);
        for (auto& p : q->pipelines) if (p.partitioned) prepareStageBuffers(*q, p);
        for (auto& h : q->hashTables) {
            h->dCount = (uint32_t*)ctx.alloc(sizeof(uint32_t));
            if (!h->derefCodes.empty()) {           // (string group values kept by address: what the row-making kernels rebuild, aot_kernels.hip table_word)
                h->dDeref = (int*)ctx.alloc(h->derefCodes.size() * sizeof(int));
                RSQ_HIP(hipMemcpyAsync(h->dDeref, h->derefCodes.data(), h->derefCodes.size() * sizeof(int), hipMemcpyHostToDevice, ctx.stream));
            }
        }
        if (q->aggMode == AggMode::AT_JOIN_ENTRY || q->aggMode == AggMode::HASH) q->dGroupCount = (uint32_t*)ctx.alloc(sizeof(uint32_t));
        q->dPipeStats = (uint64_t*)ctx.alloc(std::max<size_t>(1, q->pipelines.size()) * 8);
        size_t pw = q->pinnedWords + 8 + q->pipelines.size();
        q->hPinned = (uint64_t*)ctx.allocPinned(pw * 8);
        memset(q->hPinned, 0, pw * 8);
        {   // the device's view of the pinned words: status words are published by one kernel instead of one copy each
            void* dv = nullptr;
            if (hipHostGetDevicePointer(&dv, q->hPinned, 0) == hipSuccess && dv) q->dPinnedDev = (uint64_t*)dv; else (void)hipGetLastError();
        }
        if (q->aggMode == AggMode::DENSE_REG && q->aggPad > 1) {
            void* dv = q->dPinnedDev;
            if (dv) {
                q->dFinHost = (uint64_t*)dv;
                q->dFinTicket = (uint32_t*)ctx.alloc(16);        // [0] the ticket, [2..3] the resident step's doorbell as the workgroups see it
                RSQ_HIP(hipMemset(q->dFinTicket, 0, 16));
            }
        }
    }
    applyPlanMemo(*q);
    q->report.compilation_time_ms = nowMs() - t0;
    q->report.jit_cache_hits = ctx.jitCacheHits - hits0;
    q->report.jit_compiles = ctx.jitCompiles - comp0;
    if (ctx.cfg.print_assembly) fprintf(stderr, "%s\n", q->allSource.c_str());
    if (ctx.cfg.print_flounder) fprintf(stderr, "%s\n", q->explainText.c_str());
    return q.release();
}

// blocks until the query runs on its specialised kernels (joins the compiler thread of a query that started on the generic pipeline)
void awaitKernels(Query& q) {
    if ((!q.genericActive && !q.quickTier) || q.genericForced) return;
    if (q.bgCompiler.joinable()) q.bgCompiler.join();
    if (q.bgState.load() == 3) throw Error(RSQ_ERR_DEVICE, q.bgError);
    const bool wasGeneric = q.genericActive;
    resolveKernels(q);
    q.genericActive = false;
    if (wasGeneric && q.generic2) leaveGeneric2(q);
    if (wasGeneric) applyPlanMemo(q);
    q.explainText += "kernel tier: full (awaited)\n";
    q.report.jit_compiles = (int32_t)kernelSources(q).size();
}

// kernel time of a fused step: its events are read when somebody asks (the report) or before they are recorded again
void resolveKernelTime(Query& q) {
    // the one-launch steps that ran to their end record into a ring of event pairs, read here in one go: reading a pair costs the
    // host 2.4 us, which a benchmark loop would otherwise pay between every two steps
    if (q.evHead < q.evTail) RSQ_HIP(hipSetDevice(q.ctx.device));
    for (; q.evHead < q.evTail; q.evHead++) {
        auto& e = q.evRing[q.evHead % q.evRing.size()];
        RSQ_HIP(hipEventSynchronize(e.second));
        float ems = 0;
        RSQ_HIP(hipEventElapsedTime(&ems, e.first, e.second));
        q.report.kernel_time_ms = ems; q.kernelTimeSumMs += ems; q.kernelTimeLaunches++;
        if (!q.ringForms.empty()) { noteRowCellsTime(q, q.ringForms.front(), ems); q.ringForms.pop_front(); }
        q.report.hbm_gbps = ems > 0 ? (double)q.report.bytes_read / (ems * 1e-3) / 1e9 : 0;
    }
    if (!q.kernelTimePending || q.pendingAsync) return;
    q.kernelTimePending = false;
    RSQ_HIP(hipSetDevice(q.ctx.device));
    RSQ_HIP(hipEventSynchronize(q.gev1));
    float ms = 0;
    RSQ_HIP(hipEventElapsedTime(&ms, q.gev0, q.gev1));
    q.report.kernel_time_ms = ms; q.kernelTimeSumMs += ms; q.kernelTimeLaunches++;
    noteRowCellsTime(q, q.pairForm, ms); q.pairForm = -1;
    q.report.hbm_gbps = ms > 0 ? (double)q.report.bytes_read / (ms * 1e-3) / 1e9 : 0;
}

// The pinned host copy of the group rows, made when rows are first read back and as large as that read-back: a statement that ends on
// a handful of candidates (TPC-H Q10: 380 K groups of 40 words, LIMIT 20) never pins the 121 MB its full rows would take (7 ms of
// hipHostMalloc in the first execution on a fresh context).  Non-coherent: cached on the host (the tail reads every word), valid after
// the copy's synchronisation.
static void ensureHostGroupRows(Query& q, size_t words) {
    if (q.hGroupRowsWords >= words && q.hGroupRows) return;
    if (q.hGroupRows) q.ctx.freePinned(q.hGroupRows);
    q.hGroupRows = nullptr; q.hGroupRowsWords = 0;
    q.hGroupRows = (int64_t*)q.ctx.allocPinned(std::max<size_t>(words, 8) * 8, true);
    q.hGroupRowsWords = words;
}

// a single register-mode pipeline: its kernel carries the whole step (codegen.cpp, "The step in ONE launch")
static bool fusedEligible(const Query& q) {
    return sw::flag<sw::RSQ_FUSED_STEP>() && q.aggMode == AggMode::DENSE_REG && q.pipelines.size() == 1 && q.pipelines[0].sink == SinkKind::AGGREGATE &&
           !q.pipelines[0].partitioned && q.dFinTicket != nullptr;
}

// a shard of a multi-GPU plan that does not end in a dense partial table runs its pipelines and reads the group rows (or the
// materialised columns) back, but leaves the tail to the root, which merges all shards' groups first (tail.cpp runTailMerged)
static void tailUnlessHeld(Query& q) { if (!q.holdTail) runTail(q); }

void fetchHeldGroupRows(Query& q) {
    if (q.nGroupRows <= 0) return;
    ensureHostGroupRows(q, (size_t)q.nGroupRows * (size_t)q.groupRowWords);
    RSQ_HIP(hipSetDevice(q.ctx.device));
    RSQ_HIP(hipMemcpy(q.hGroupRows, q.dGroupRows, (size_t)q.nGroupRows * (size_t)q.groupRowWords * 8, hipMemcpyDeviceToHost));
}

// rsq_multi_* builds the derived tables in front of the execution (engine_derived_multi.cpp marks every one of them)
static bool derivedExternal(const Query& q) {
    for (const DerivedState& d : q.derived) if (!d.sub.external) return false;
    return true;
}

static void executeQueryBody(Query& q, bool partialOnly, bool async);
void executeQuery(Query& q, bool partialOnly, bool async) {
    // rows appended to a table move its columns (rsq_table_append): the kernels' arguments of a statement compiled before point at memory
    // that has been given back.  A ReSQL host compiles per statement (execute.h:213-247); whoever keeps a compiled query across a
    // BULK INSERT is told to compile it again instead of being answered from freed memory.
    for (size_t i = 0; i < q.tables.size() && i < q.tableLayouts.size(); i++)
        if (q.tables[i]->layoutVersion != q.tableLayouts[i])
            throw Error(RSQ_ERR_INVALID, "rows were appended to table " + q.tables[i]->name + " (or its narrow column images were rebuilt) after this statement was compiled: compile it again");
    if ((partialOnly || async) && !q.derived.empty() && !(derivedExternal(q) && !async)) refuseDerived(q, "partial / asynchronous execution");
    executeQueryBody(q, partialOnly, async);
    keepKeyIndexes(q);
    rememberPlan(q);
}

void runSubQuery(SubQuery& s, bool partialOnly) {
    executeQuery(*s.query, partialOnly);
    s.kernels = s.query->report.num_kernels; s.bytes = s.query->report.bytes_read;
}

// The inner side of a nested-loops join, and the pair budget: outer rows x inner rows above rsq_config.nested_loops_max_pairs ends the
// execution before the outer pipeline starts.  Across GPUs multi.cpp runs the steps itself: every shard's inner part, then the budget over
// the whole statement, then the all-gather of the parts into the bound columns.
void runNestedLoopsInner(NljState& n, bool run) {
    n.nInner = 0; n.sub.kernels = 0; n.sub.bytes = 0;
    if (!run) return;
    runSubQuery(n.sub);
    n.nInner = n.sub.query->matRows;
}

void bindNestedLoops(Query& q, NljState& n, int64_t outer, int64_t nInner) {
    Context& ctx = q.ctx;
    n.nInner = nInner;
    const int64_t budget = ctx.cfg.nested_loops_max_pairs;
    const long double pairs = (long double)outer * (long double)n.nInner;
    if (pairs > (long double)budget)
        failUnsupported("nested-loops join: " + std::to_string((long long)outer) + " outer rows x " + std::to_string((long long)n.nInner) +
                        " inner rows is more than rsq_config.nested_loops_max_pairs (" + std::to_string((long long)budget) + " pairs)");
    // a materialisation counts tuples per lane and per 128-row tile in 32 bits: 128 outer rows x the inner rows must stay below 2^32
    if (n.pipeline >= 0 && q.pipelines[(size_t)n.pipeline].sink == SinkKind::MATERIALIZE && 128.0L * (long double)n.nInner >= 4294967296.0L)
        failUnsupported("nested-loops join: " + std::to_string((long long)n.nInner) + " inner rows - a 128-row tile of the outer side could emit "
                        "2^32 or more tuples, beyond the materialisation's 32-bit tile counts");
    n.sub.ensureColumns(ctx, n.innerSchema, n.nInner, std::max<int64_t>(n.nInner, 64));
    // the slices of the inner range in this execution's launch (an aggregating pipeline: codegen.cpp consumeNestedLoops), from the grid the
    // outer rows ask for, the most the pipeline launches and the inner rows; pipelineGrid and the kernel's argument read it from here
    n.slices = 1;
    if (n.sliced && n.pipeline >= 0 && q.pipelines[(size_t)n.pipeline].nljSliced >= 0) {
        int64_t want, cap;
        pipelineGridLimits(q, q.pipelines[(size_t)n.pipeline], false, want, cap);
        n.slices = rsq_nested_loops_slices(want, cap, n.nInner, ctx.cfg.nested_loops_inner_slices);
    }
}

NljState& topNestedLoops(Query& q) {
    NljState* top = nullptr;
    for (NljState& n : q.nljs)
        if (n.sub.query && n.outerSrc) {
            if (top) failUnsupported("more than one nested-loops join outside each other's inner side");
            top = &n;
        }
    if (!top) failInvalid("the plan has no nested-loops join");
    return *top;
}

// The writer for derived table `d` of `q`: `s`'s packed tuples (its own sub-query's, or the root's after a merge across shards) into
// d's columns on q's context - read where the device tail left them (deviceTuples, same device), or uploaded once from the host's - and
// the scan's row count and column addresses bound (engine_pipelines.cpp argValue).  Its launch and the tuples it reads are d.sub's work.
void writeDerivedFrom(Query& q, DerivedState& d, Query& s, bool deviceTuples) {
    Context& ctx = q.ctx;
    Table& t = *d.table;
    if (s.resultSchema.size() != t.cols.size()) failRuntime("internal error: " + t.name + " has " + std::to_string(t.cols.size()) +
                                                             " columns, its sub-query gave " + std::to_string(s.resultSchema.size()));
    std::vector<DerivedColumn> cols;
    int off = 0;
    for (size_t c = 0; c < t.cols.size(); c++) {
        if (!equalTypes(s.resultSchema[c].type, t.cols[c].type)) failRuntime("internal error: column " + std::to_string(c) + " of " + t.name + " changed its type");
        cols.push_back({off, columnWidth(t.cols[c].type), nullptr});
        off += sizeInTuple(t.cols[c].type, true);
    }
    const int tupleSize = off;
    const int64_t n = s.resultRows;
    d.sub.ensureColumns(ctx, t.cols, std::max<int64_t>(n, 1), std::max<int64_t>(n + n / 8, 64));      // (an empty table has its columns too)
    for (size_t c = 0; c < cols.size(); c++) { cols[c].out = d.sub.dCols[c]; t.cols[c].dptr = d.sub.dCols[c]; }
    // (two producers of resultDev, told apart by pointer: derived sub-queries always have an aggregation, and a sub-query's materialisation
    // never takes the result-pack tail - RSQ_RESULT_PACK_FALLBACK_SHAPE - so its buffer is not a third case here)
    const uint8_t* tuples = deviceTuples && s.resultInPinned ? s.resultDev : nullptr;
    if (tuples) {      // (the device tail's layout must be the one the writer decodes)
        const int devTuple = tuples == s.dtRows ? s.dtTupleSize : s.rtTupleSize;
        if (devTuple != tupleSize) failRuntime("internal error: the device tail of " + t.name + " made " + std::to_string(devTuple) +
                                               "-byte tuples, the derived table's columns take " + std::to_string(tupleSize));
    }
    if (n > 0 && !tuples) {
        const size_t b = (size_t)n * (size_t)tupleSize;
        if ((int64_t)b > d.tupleCapacity) {
            if (d.dTuples) ctx.free(d.dTuples);
            d.tupleCapacity = (int64_t)(b + b / 8);
            d.dTuples = ctx.alloc((size_t)d.tupleCapacity);
        }
        const uint8_t* host = s.resultInPinned ? s.resultPinned : s.resultTuples.data();
        RSQ_HIP(hipMemcpyAsync(d.dTuples, host, b, hipMemcpyHostToDevice, ctx.stream));
        tuples = (const uint8_t*)d.dTuples;
    }
    if (n > 0) {
        derivedColumns(ctx, tuples, n, tupleSize, cols);
        d.sub.kernels += 1;
        d.sub.bytes += (uint64_t)n * (uint64_t)tupleSize;
    }
    t.nRows = n; t.row0 = 0; t.nRowsTotal = -1;
}

void buildDerived(Query& q, DerivedState& d) {
    runSubQuery(d.sub);
    writeDerivedFrom(q, d, *d.sub.query, true);
}

// The sub-queries, in front of this query's pipelines at every execution (the host may have rewritten adopted input columns in place, so
// nothing is kept from the previous one).  Each runs here, or rsq_multi_* has run it (external); either way its recorded work is this
// execution's.  A derived table: its sub-query (its own derived tables first), then the writer.  A nested-loops join: the inner side, its
// work counted even when the pair budget then ends the execution, then its result columns (struct of arrays, strings by value) copied
// into the bound columns.
static void runSubQueries(Query& q) {
    Context& ctx = q.ctx;
    auto account = [&](const SubQuery& s) { q.report.num_kernels += s.kernels; q.report.bytes_read += s.bytes; };
    for (DerivedState& d : q.derived) {              // (the interpreters decline plans over derived tables: generic*.cpp)
        if (!d.sub.external) {
            buildDerived(q, d);
            traceLine("[rsq trace] %s: %lld rows written from the %s tail's tuples\n", d.table->name.c_str(), (long long)d.table->nRows,
                      d.sub.query->resultInPinned && d.sub.query->resultDev ? "device" : "host");
        }
        account(d.sub);
    }
    for (NljState& n : q.nljs) {                     // (nested-loops plans never run on the interpreters: generic*.cpp decline them)
        if (!n.sub.query || !n.outerSrc) continue;   // (a join of an inner side: that side's query runs it)
        const int64_t outer = n.outerSrc->nRows;
        if (!n.sub.external) runNestedLoopsInner(n, outer > 0);      // (an empty outer side needs no inner rows)
        account(n.sub);
        if (n.sub.external) continue;
        bindNestedLoops(q, n, outer, n.nInner);
        const Query& in = *n.sub.query;
        for (size_t k = 0; k < n.innerSchema.size() && n.nInner > 0; k++) {
            const void* src = in.dMatCols[(size_t)n.innerCol[k]];
            RSQ_HIP(hipMemcpyAsync(n.sub.dCols[k], src, (size_t)n.nInner * (size_t)columnWidth(n.innerSchema[k].type), hipMemcpyDefault, ctx.stream));
        }
    }
}

static void executeQueryBody(Query& q, bool partialOnly, bool async) {
    Context& ctx = q.ctx;
    if (ctx.device < 0) throw Error(RSQ_ERR_DEVICE, "this context has no device (compile-only)");
    RSQ_HIP(hipSetDevice(ctx.device));
    const uint64_t epochAtEntry = ctx.execEpoch++;
    q.hRowsView = nullptr;          // (set around a candidate run of the tail only; an execution that did not come back must not leave it)
    if (async) {
        if (!partialOnly || !partialCapable(q)) failUnsupported("asynchronous execution is available for dense partial aggregation only");
        for (auto& p : q.pipelines)
            if (p.sink != SinkKind::AGGREGATE) failUnsupported("asynchronous execution needs a plan without join / materialize pipelines");
    }
    double t0 = nowMs();
    const size_t words = q.pinnedWords;
    q.report.num_kernels = 0; q.report.bytes_read = 0;
    resetMaterializeReports(q);
    runSubQueries(q);
    if (!q.genericActive && q.quickTier && q.bgState.load() >= 3) {
        // the full kernels are in the cache now: the quick tier's are replaced (same arguments, same tables - nothing else changes).
        // (A full tier that failed to compile leaves the query on the quick one.)
        const int st = q.bgState.load();
        if (q.bgCompiler.joinable()) q.bgCompiler.join();
        if (st == 4) { resolveKernels(q); q.explainText += "kernel tier: full\n"; }
        else q.bgState = 0;
    }
    if (q.genericActive) {
        if (!q.genericForced && q.bgState.load() >= 2) {
            // the specialised kernels are in the code-object cache now (or their compilation failed): switch over
            const int st = q.bgState.load();
            if (st != 2 && q.bgCompiler.joinable()) q.bgCompiler.join();      // (2: the thread is still compiling the full tier)
            if (st == 3) throw Error(RSQ_ERR_DEVICE, q.bgError);
            resolveKernels(q, st == 2);
            q.explainText += st == 2 ? "kernel tier: quick (stage 2 called) until the inlined kernels are ready\n" : "kernel tier: full\n";
            q.genericActive = false;
            if (q.generic2) leaveGeneric2(q);
            applyPlanMemo(q);
            q.report.jit_compiles = (int32_t)kernelSources(q).size();       // built by the compiler thread since rsq_query_compile returned
        } else if (!q.generic2) {
            // ---- the generic pipeline: table init, ONE interpreter launch, read-back ----
            Pipeline& p = q.pipelines[0];
            q.fusedReady = false;
            ctx.errWordClean = false;
            RSQ_HIP(hipMemcpyAsync(q.dAgg, q.dAggInit, q.tableWords * 8, hipMemcpyDeviceToDevice, ctx.stream));
            RSQ_HIP(hipMemsetAsync(ctx.dErr, 0, 4, ctx.stream));
            RSQ_HIP(hipEventRecord(ctx.ev0, ctx.stream));
            launchGenericAggregate(ctx, q.generic, q.dGenericCode, p.src->nRows, p.src->row0, q.dAgg, q.denseGroups, (int64_t)q.tableWords);
            RSQ_HIP(hipEventRecord(ctx.ev1, ctx.stream));
            q.report.num_kernels = 1;
            q.report.bytes_read = (uint64_t)(p.bytesPerRow * p.src->nRows);
            RSQ_HIP(hipMemcpyAsync(q.hPinned + words, ctx.dErr, 4, hipMemcpyDeviceToHost, ctx.stream));
            if (!partialOnly) RSQ_HIP(hipMemcpyAsync(q.hPinned, q.dAgg, q.tableWords * 8, hipMemcpyDeviceToHost, ctx.stream));
            if (async && partialOnly) { q.pendingAsync = true; q.pendingFused = false; q.report.execution_time_ms = nowMs() - t0; return; }
            waitForStream(ctx);
            float gms = 0; RSQ_HIP(hipEventElapsedTime(&gms, ctx.ev0, ctx.ev1));
            q.report.kernel_time_ms = gms; q.kernelTimeSumMs += gms; q.kernelTimeLaunches++;
            q.report.hbm_gbps = gms > 0 ? (double)q.report.bytes_read / (gms * 1e-3) / 1e9 : 0;
            ctx.errWordClean = (uint32_t)q.hPinned[words] == 0;
            checkDeviceError((uint32_t)q.hPinned[words]);
            if (!partialOnly) {
                double t1 = nowMs();
                q.hAggView = nullptr;
                memcpy(q.hAgg.data(), q.hPinned, q.tableWords * 8);
                tailUnlessHeld(q);
                q.report.finalize_time_ms = nowMs() - t1;
            }
            q.report.execution_time_ms = nowMs() - t0;
            return;
        }
    }
    const bool interp = q.genericActive && q.generic2;      // this execution's pipelines run on the interpreter for whole pipelines
    q.flatRun = (partialOnly || interp) && q.aggPad > 1;      // (the interpreter aggregates into the unpadded table)
    const sw::Level traceLevel = sw::level<sw::RSQ_TRACE>();
    const bool trace = traceLevel.on;      // per-pipeline wall time (synchronises after each one)
    uint32_t topkCapacity = 0, topkSpec = 0;      // > 0: this execution pre-selects ORDER BY ... LIMIT candidates on the device
    bool topkRange = false;                       // ... with the short form (one histogram over the images' range)
    uint32_t groupRowsAllocated = 0;              // rows the group-row buffers of this execution can take
    uint64_t selectSeq = 0;                       // ... announced by this sequence number in pinned word 4
    bool selectPublished = false;                 // ... and the selection's launch has delivered candidates and status words to the host
    bool narrowRows = false;                      // ... from narrow group rows [slot | sort key]: q.dGroupRows was NOT written by this execution
    // ---- the step in one launch: a single register-mode pipeline whose last workgroup publishes the table ----
    if (fusedEligible(q) && !trace && !interp) {
        Pipeline& p = q.pipelines[0];
        // the kernel leaves its working table, the error word and the ticket at their identities; make them so the first
        // time, after an execution that did not come back (an exception between launch and synchronisation), and whenever
        // another query of this context may have left the shared error word set
        if (!q.fusedReady || !ctx.errWordClean) {
            RSQ_HIP(hipMemcpyAsync(q.dAggWork, q.dAggWorkInit, q.padWords * 8, hipMemcpyDeviceToDevice, ctx.stream));
            RSQ_HIP(hipMemsetAsync(q.dFinTicket, 0, 4, ctx.stream));
            RSQ_HIP(hipMemsetAsync(ctx.dErr, 0, 4, ctx.stream));
            ctx.errWordClean = true;
        }
        // a step that runs to its end here takes the next pair of the event ring (read when somebody asks, or when the ring is
        // full); an asynchronous partial step keeps the single pair finalize / settle read
        const bool ringEvents = !(async && partialOnly);
        if (ringEvents) {
            // the ring grows with the steps nobody has read yet: 8 pairs, doubled when full, up to 256 (a statement that is executed once
            // takes 16 events from the context's pool, a loop of steps ends up with the 512 it had from the start before round 5)
            const bool full = q.evTail - q.evHead == q.evRing.size();      // (an empty ring is full too)
            if (q.kernelTimePending || full) resolveKernelTime(q);          // everything recorded so far is read: head == tail
            if (full && q.evRing.size() < 256) {
                const size_t more = q.evRing.empty() ? 8 : q.evRing.size();
                q.evHead = q.evTail = 0;
                for (size_t i = 0; i < more; i++) { hipEvent_t a = ctx.takeEvent(), b = ctx.takeEvent(); q.evRing.emplace_back(a, b); }
            }
        } else resolveKernelTime(q);                           // the previous step's events, before they are recorded again
        q.fusedReady = false;
        q.flatRun = false;                                     // always the padded kernel: the last workgroup unpads
        const bool poll = sw::flag<sw::RSQ_POLL>() && !partialOnly;
        const uint64_t seq = poll ? ++q.finSeqCounter : 0;
        q.finSeq = seq;
        q.finOut = partialOnly ? q.dAgg : q.dFinHost;          // device partial table | host-mapped pinned read-back buffer
        q.finErr = q.dFinHost + q.pinnedWords;
        if (!q.gev0) { q.gev0 = ctx.takeEvent(); q.gev1 = ctx.takeEvent(); }
        hipEvent_t evA = q.gev0, evB = q.gev1;
        prepareRowCellsForm(q, p);                             // (may read the earlier steps' events: before this step's pair is picked and recorded)
        if (ringEvents) { auto& e = q.evRing[q.evTail % q.evRing.size()]; evA = e.first; evB = e.second; }
        // two event records around the launch.  (An extended launch that takes the events itself costs the host 3 us more per step
        // and the tail another 1.5: measured 16 us of step overhead against 11.5.)
        RSQ_HIP(hipEventRecord(evA, ctx.stream));
        launchPipelineKernel(q, p, *p.kernel, -1);
        RSQ_HIP(hipEventRecord(evB, ctx.stream));
        {
            const int timedForm = p.measuring ? p.lastForm : -1;
            if (p.measuring) { p.cellsLaunched[p.lastForm]++; p.measuring = false; p.measureForm = 0; }
            if (ringEvents) q.ringForms.push_back(timedForm); else q.pairForm = timedForm;
        }
        q.finOut = nullptr;
        q.finSeq = 0;
        if (ringEvents) q.evTail++; else q.kernelTimePending = true;
        q.report.bytes_read = (uint64_t)(p.bytesPerRow * p.src->nRows);
        if (async && partialOnly) {
            // (the kernel leaves its working table reset, and whatever comes next on this stream is ordered behind it)
            q.fusedReady = true;
            q.pendingAsync = true; q.pendingFused = true; q.report.execution_time_ms = nowMs() - t0; return;
        }
        if (poll) {
            // the finished table is in host memory as soon as the last workgroup's stores have landed: watch the sequence
            // number instead of waiting for the stream's completion signal (saves the interrupt path, ~8 us per step);
            // hipStreamQuery now and then notices a failed launch, and a kernel that takes long is waited for properly
            volatile uint64_t* flag = q.hPinned + q.pinnedWords + 1;
            const double deadline = nowMs() + 5.0;
            unsigned spins = 0;
            while (*flag != seq) {
                if ((++spins & 1023u) == 0) {
                    hipError_t e = hipStreamQuery(ctx.stream);
                    if (e != hipSuccess && e != hipErrorNotReady) RSQ_HIP(e);
                    if (e == hipSuccess || nowMs() > deadline) { waitForStream(ctx); break; }
                }
                __builtin_ia32_pause();
            }
            if (*flag != seq) failRuntime("internal error: the fused step finished without publishing its table");
            std::atomic_thread_fence(std::memory_order_acquire);
        } else waitForStream(ctx);
        q.fusedReady = true;
        if (q.dDebugStamps) {
            static int nPrinted = 0;
            waitForStream(ctx);
            std::vector<uint64_t> st((size_t)p.lastGrid * 8);
            RSQ_HIP(hipMemcpy(st.data(), q.dDebugStamps, st.size() * 8, hipMemcpyDeviceToHost));
            uint64_t t0s = ~0ull, endLoop = 0, endRed = 0, endFlush = 0, endTicket = 0, last5 = 0, last6 = 0, last7 = 0;
            for (unsigned w = 0; w < p.lastGrid; w++) {
                t0s = std::min(t0s, st[w * 8 + 0]); endLoop = std::max(endLoop, st[w * 8 + 1]); endRed = std::max(endRed, st[w * 8 + 2]);
                endFlush = std::max(endFlush, st[w * 8 + 3]); endTicket = std::max(endTicket, st[w * 8 + 4]);
                last5 = std::max(last5, st[w * 8 + 5]); last6 = std::max(last6, st[w * 8 + 6]); last7 = std::max(last7, st[w * 8 + 7]);
            }
            if ((nPrinted + 1) % 50 == 0) {
                std::vector<uint64_t> ends;
                for (unsigned w = 0; w < p.lastGrid; w++) ends.push_back(st[w * 8 + 2]);
                std::sort(ends.begin(), ends.end());
                fprintf(stderr, "[rsq tail] workgroups done with their rows and reductions at: first %.2f, 10 %% %.2f, median %.2f, 90 %% %.2f, last %.2f us\n",
                        (ends.front() - t0s) / 100.0, (ends[ends.size() / 10] - t0s) / 100.0, (ends[ends.size() / 2] - t0s) / 100.0,
                        (ends[ends.size() * 9 / 10] - t0s) / 100.0, (ends.back() - t0s) / 100.0);
            }
            if (++nPrinted % 50 == 0)
                fprintf(stderr, "[rsq tail] %u workgroups; us since the first workgroup started: last loop end %.2f, wave reductions %.2f, flush issued %.2f, "
                                "ticket taken %.2f, cells exchanged + stored to host %.2f, stores acknowledged %.2f, flag stored %.2f\n", p.lastGrid,
                        (endLoop - t0s) / 100.0, (endRed - t0s) / 100.0, (endFlush - t0s) / 100.0, (endTicket - t0s) / 100.0, (last5 - t0s) / 100.0,
                        (last6 - t0s) / 100.0, (last7 - t0s) / 100.0);
            RSQ_HIP(hipMemset(q.dDebugStamps, 0, st.size() * 8));
        }
        checkDeviceError((uint32_t)q.hPinned[q.pinnedWords]);
        if (!partialOnly) {
            double t1 = nowMs();
            q.hAggView = nullptr;
            memcpy(q.hAgg.data(), q.hPinned, q.tableWords * 8);
            tailUnlessHeld(q);
            q.report.finalize_time_ms = nowMs() - t1;
        }
        q.report.execution_time_ms = nowMs() - t0;
        return;
    }
    // (read behind the one-launch step, which asks for neither)
    const bool publishStatus = q.dPinnedDev && sw::flag<sw::RSQ_PUBLISH_STATUS>();      // status words by a kernel's stores into pinned memory
    const bool fusedSelectOn = sw::flag<sw::RSQ_FUSED_SELECT>();
    auto ensureCandHost = [&]() {        // coherent pinned rows for topkCapacity candidates, and the device's view of them
        const size_t need = (size_t)topkCapacity * (size_t)q.groupRowWords;
        if (q.hCandRowsWords >= need && q.dHostCandRows) return;
        if (q.hCandRows) ctx.freePinned(q.hCandRows);
        q.hCandRows = nullptr; q.dHostCandRows = nullptr; q.hCandRowsWords = 0;
        q.hCandRows = (int64_t*)ctx.allocPinned(std::max<size_t>(need, 8) * 8);
        q.hCandRowsWords = need;
        void* dv = nullptr;
        if (hipHostGetDevicePointer(&dv, q.hCandRows, 0) == hipSuccess && dv) q.dHostCandRows = (int64_t*)dv; else (void)hipGetLastError();
    };
    auto fusedSelectOk = [&]() {
        if (!fusedSelectOn || q.fusedSelectOff || !publishStatus || partialOnly || async || trace) return false;
        ensureCandHost();
        return q.dHostCandRows != nullptr;
    };
    if (denseMode(q)) enqueueTableInit(q);
    ctx.errWordClean = false;      // until this execution has read the word back as 0
    bool anyCompaction = false;
    for (auto& p : q.pipelines) anyCompaction |= p.compact;
    // everything small this execution wants cleared, in one launch (aot_kernels.hip k_fill_batch): the error word, the pipelines'
    // row counters, the group counter and the candidate selection's scratch of a compaction behind the last pipeline
    bool groupCountCleared = false, topkScratchCleared = false;
    bool accumulatorsCleared = false;       // the aggregates beside a join table's entries are at their identities (AT_JOIN_ENTRY)
    // A hash aggregation that has run before: its table is readied with everything else in the first fill (or behind the previous
    // execution's last kernel), the group count is the remembered one, and whether the table overflowed or CHAR groups need merging
    // is read from the FINAL status words - no synchronisation between the pipelines and the group rows.  (TPC-H Q10 at SF10: two 4-byte
    // read-backs with a stream synchronisation each and three clearing launches, ~40 of 590 us.)  Whatever turns out different from the
    // remembered state starts the execution over on the careful path (lastCount = 0).
    bool hashWarm = false;
    std::vector<FillItem> f;                // (kept: an execution that ends on its candidates enqueues the same clears for the next one)
    {
        f.push_back(FillItem{ctx.dErr, 4, 0});
        if (anyCompaction) f.push_back(FillItem{q.dPipeStats, q.pipelines.size() * 8, 0});
        if (q.dGroupCount) { f.push_back(FillItem{q.dGroupCount, 4, 0}); groupCountCleared = true; }
        if (q.dTopkHists) { f.push_back(FillItem{q.dTopkHists, topkRangeScratchBytes(), 0}); topkScratchCleared = true; }
        // Join tables that have been sized (every execution but a query's first) are readied HERE, all of them in this one launch,
        // instead of one launch in front of every build (TPC-H Q5 builds five tables, Q3 two); likewise the aggregates kept beside
        // a join table's entries.  Nothing touches a table between this fill and its build pipeline.
        const bool prologueOk = true;
        for (auto& hp : q.hashTables) hp->prepared = false;       // (an execution that did not come back must not leave a table marked as readied)
        if (prologueOk && !trace && !interp)
            for (auto& p : q.pipelines) {
                if (p.sink != SinkKind::BUILD) continue;
                HashTable& h = *q.hashTables[(size_t)p.buildTable];
                h.prepared = false;
                if (h.capacity == 0) continue;
                if (h.direct && (h.dense || (h.keyIndexReady && h.keyIndexVersion == p.src->version))) continue;      // nothing is built: nothing to ready
                const size_t nWords = h.keys.size() + h.payload.size();
                const size_t bmBytes = h.hasBitmap && h.dBitmap ? (size_t)h.bmBlocks * 32 : 0;
                if (h.rank && h.setOnly) { if (!bmBytes) continue; }
                else if (h.rank) {
                    if (!h.dTempUsed || !h.dChunkTotal) continue;
                    f.push_back(FillItem{h.dTempUsed, (size_t)h.tempWaves * 4, 0});
                    f.push_back(FillItem{h.dChunkTotal, (size_t)((h.bmBlocks + RSQ_RANK_CHUNK_BLOCKS - 1) / RSQ_RANK_CHUNK_BLOCKS) * 4, 0});      // the chain of the one-launch index
                } else if (h.keyCas) {
                    if (!h.dWords) continue;
                    f.push_back(FillItem{h.dWords, (size_t)h.capacity * (h.aos ? std::max<size_t>(1, nWords) : 1) * 8, 0x8000000000000000ull});
                } else {
                    if (!h.dState) continue;
                    f.push_back(FillItem{h.dState, (size_t)h.capacity * 4, 0});
                }
                if (bmBytes) f.push_back(FillItem{h.dBitmap, bmBytes, 0});
                f.push_back(FillItem{h.dCount, 4, 0});
                h.prepared = true;
            }
        if (prologueOk && !trace && !interp && q.aggMode == AggMode::AT_JOIN_ENTRY) {
            HashTable& h = *q.hashTables[(size_t)q.aggTable];
            if (h.capacity > 0 && h.dAcc && h.prepared) {       // (sized, and not about to be re-sized by its build)
                for (int b = 0; b < h.nAccBlocks; b++) {
                    const uint64_t idv = b < q.nMinBlocks ? 0x7fffffffffffffffull : b < q.nMinBlocks + q.nMaxBlocks ? 0x8000000000000000ull : 0ull;
                    f.push_back(FillItem{(uint64_t*)h.dAcc + (size_t)b * (size_t)h.capacity, (size_t)h.capacity * 8, idv});
                }
                accumulatorsCleared = true;
            }
        }
        if (!trace && !interp && q.aggMode == AggMode::HASH && !partialOnly && !async && !q.holdTail && q.aggTable >= 0) {
            HashTable& h = *q.hashTables[(size_t)q.aggTable];
            if (h.capacity > 0 && h.dState && h.dAcc && h.lastCount > 0 && (int64_t)h.lastCount * 2 <= h.capacity) {
                f.push_back(FillItem{h.dState, (size_t)h.capacity * 4, 0});
                f.push_back(FillItem{h.dCount, 4, 0});
                for (int b = 0; b < h.nAccBlocks; b++) {
                    const uint64_t idv = b < q.nMinBlocks ? 0x7fffffffffffffffull : b < q.nMinBlocks + q.nMaxBlocks ? 0x8000000000000000ull : 0ull;
                    f.push_back(FillItem{(uint64_t*)h.dAcc + (size_t)b * (size_t)h.capacity, (size_t)h.capacity * 8, idv});
                }
                hashWarm = true;
            }
        }
        // ... unless the previous execution of this query has already enqueued exactly these clears behind its last kernel and
        // nothing else ran on the context since (RSQ_POST_CLEAR=0: never)
        auto same = [](const std::vector<FillItem>& a, const std::vector<FillItem>& b) {
            if (a.size() != b.size()) return false;
            for (size_t i = 0; i < a.size(); i++) if (a[i].p != b[i].p || a[i].bytes != b[i].bytes || a[i].value != b[i].value) return false;
            return true;
        };
        const bool readied = q.readied && q.readiedEpoch == epochAtEntry && same(f, q.readiedFill);
        q.readied = false;
        if (!readied) {
            fillBatchAsync(ctx, f.data(), (int)f.size());
            q.report.num_kernels += (f.size() + 23) / 24;
        }
    }
    // (the execution's event pair is the query's own, read when somebody asks: an execution that ends on the candidate selection's
    // sequence number returns before the stream has reported the second event)
    resolveKernelTime(q);
    if (!q.gev0) { q.gev0 = ctx.takeEvent(); q.gev1 = ctx.takeEvent(); }
    RSQ_HIP(hipEventRecord(q.gev0, ctx.stream));
    double tPipe = nowMs();
    auto tracePoint = [&](const Pipeline& p) {
        if (!trace) return;
        (void)hipStreamSynchronize(ctx.stream);
        double t = nowMs();
        fprintf(stderr, "[rsq trace] %.3f ms  %s\n", t - tPipe, p.explain.c_str());
        if (p.sink == SinkKind::BUILD) {
            HashTable& h = *q.hashTables[(size_t)p.buildTable];
            uint32_t n = 0;
            (void)hipMemcpy(&n, h.dCount, 4, hipMemcpyDeviceToHost);
            fprintf(stderr, "[rsq trace]     ht%d: %u entries in %lld slots\n", h.id, n, (long long)h.capacity);
        }
        tPipe = nowMs();
    };
    for (auto& p : q.pipelines) {
        if (interp) { runGeneric2Pipeline(q, (size_t)(&p - q.pipelines.data())); tracePoint(p); continue; }
        if (p.sink == SinkKind::BUILD) { buildHashTable(q, p); tracePoint(p); continue; }
        if (p.sink == SinkKind::MATERIALIZE) { materializePipeline(q, p); tracePoint(p); continue; }
        auto resetAccumulators = [&](HashTable& h) {
            // aggregate words beside the entries: first-row / min blocks to +inf, max blocks to -inf, sums to 0
            std::vector<FillItem> f;
            for (int b = 0; b < h.nAccBlocks; b++) {
                uint64_t idv = b < q.nMinBlocks ? 0x7fffffffffffffffull : b < q.nMinBlocks + q.nMaxBlocks ? 0x8000000000000000ull : 0ull;
                f.push_back(FillItem{(uint64_t*)h.dAcc + (size_t)b * (size_t)h.capacity, (size_t)h.capacity * 8, idv});
            }
            fillBatchAsync(ctx, f.data(), (int)f.size());
        };
        if (q.aggMode == AggMode::AT_JOIN_ENTRY && !accumulatorsCleared) { resetAccumulators(*q.hashTables[(size_t)q.aggTable]); q.report.num_kernels++; }
        if (q.aggMode == AggMode::HASH && hashWarm) {
            launchPipeline(q, p, -1);
            q.report.bytes_read += (uint64_t)(p.bytesPerRow * p.src->nRows);
            tracePoint(p);
            continue;
        }
        if (q.aggMode == AggMode::HASH) {
            // The number of groups is not known before the scan: start from the reference's own estimate
            // (AggregationOp::getSize, aggregation.h:81-92) and re-run the pipeline with a 4x larger table while
            // the kernel reports a full table.
            HashTable& h = *q.hashTables[(size_t)q.aggTable];
            if (h.capacity == 0) h.capacity = nextPow2(std::max<int64_t>(4096, 4 * (int64_t)opSize(q.agg, true)));
            if ((int64_t)h.lastCount * 2 > h.capacity) {        // the previous execution filled more than half of the table
                if (h.dState) { ctx.free(h.dState); ctx.free(h.dWords); ctx.free(h.dAcc); }
                h.dState = nullptr; h.dWords = nullptr; h.dAcc = nullptr;
                while ((int64_t)h.lastCount * 2 > h.capacity) h.capacity *= 2;
            }
            for (;;) {
                if (!h.dState) {
                    h.dState = (uint32_t*)ctx.alloc((size_t)h.capacity * 4);
                    h.dWords = (int64_t*)ctx.alloc((size_t)h.capacity * 8 * (h.keys.size() + h.payload.size()));      // key words, then carried group values
                    h.dAcc = (int64_t*)ctx.alloc((size_t)h.capacity * 8 * (size_t)h.nAccBlocks);
                }
                RSQ_HIP(hipMemsetAsync(h.dState, 0, (size_t)h.capacity * 4, ctx.stream));
                RSQ_HIP(hipMemsetAsync(h.dCount, 0, 4, ctx.stream));
                resetAccumulators(h);
                launchPipeline(q, p, -1);
                uint32_t err = 0;
                RSQ_HIP(hipMemcpyAsync(&err, ctx.dErr, 4, hipMemcpyDeviceToHost, ctx.stream));
                waitForStream(ctx);
                q.charGroupsNeedMerge = (err & 32u) != 0;
                if (trace) fprintf(stderr, "[rsq trace]     hash aggregation table ht%d: %lld slots%s\n", h.id, (long long)h.capacity, (err & 2) ? " - too small, four times as many next" : "");
                if (!(err & 2)) break;
                if (h.capacity >= ((int64_t)1 << 31)) failRuntime("Hash table full");
                ctx.free(h.dState); ctx.free(h.dWords); ctx.free(h.dAcc);
                h.dState = nullptr; h.dWords = nullptr; h.dAcc = nullptr;
                h.capacity *= 4;
                RSQ_HIP(hipMemsetAsync(ctx.dErr, 0, 4, ctx.stream));
            }
            q.report.bytes_read += (uint64_t)(p.bytesPerRow * p.src->nRows);
            tracePoint(p);
            continue;
        }
        if (p.partitioned) runLargeDenseAggregation(q, p);
        else launchPipeline(q, p, -1);
        q.report.bytes_read += (uint64_t)(p.bytesPerRow * p.src->nRows);
        tracePoint(p);
    }
    if ((q.aggMode == AggMode::AT_JOIN_ENTRY || q.aggMode == AggMode::HASH) && !partialOnly) {
        HashTable& h = *q.hashTables[(size_t)q.aggTable];
        const int nTab = (int)(h.keys.size() + h.payload.size());
        q.groupRowWords = 1 + nTab + h.nAccBlocks;
        // Rows to provide for: the number of occupied entries.  It is read back (one synchronisation) on the first
        // execution; later executions reuse it — the build reads the same table (hash aggregation: hashWarm above) — and the
        // compaction never writes beyond the buffer: a larger count is noticed after the final synchronisation and
        // the execution is repeated with a fresh count.
        uint32_t nEntries = h.lastCount;
        if ((q.aggMode != AggMode::AT_JOIN_ENTRY && !hashWarm) || nEntries == 0 || trace) {
            RSQ_HIP(hipMemcpyAsync(&nEntries, h.dCount, 4, hipMemcpyDeviceToHost, ctx.stream));
            waitForStream(ctx);
            h.lastCount = nEntries;
        }
        groupRowsAllocated = std::max<uint32_t>(1, nEntries);
        size_t need = (size_t)groupRowsAllocated * (size_t)q.groupRowWords;
        if (q.dGroupRowsWords < need) {
            if (q.dGroupRows) ctx.free(q.dGroupRows);
            q.dGroupRows = nullptr; q.dGroupRowsWords = 0;          // (nothing dangles if the allocation below throws)
            q.dGroupRows = (int64_t*)ctx.alloc(need * 8);
            q.dGroupRowsWords = need;
        }
        // ORDER BY ... LIMIT k over many groups: select the candidate rows on the device and read back only those
        if (q.topkWord == -2) planDeviceTopK(q);
        const bool preselect = !q.holdTail && q.topkWord >= 0 && nEntries >= 2048 && (uint64_t)nEntries > 4ull * q.topkWant && !(q.topkNeedsNoMerge && q.charGroupsNeedMerge);
        if (preselect) {
            topkCapacity = std::min<uint32_t>(nEntries, std::max<uint32_t>(1024, 4 * q.topkWant));
            if (!q.dTopkHists) { q.dTopkHists = (uint32_t*)ctx.alloc(topkHistBytes()); q.dCandCount = q.dTopkHists + 4; }
            if (q.candCapacity < topkCapacity || q.candRowWords != q.groupRowWords) {
                if (q.dCandRows) ctx.free(q.dCandRows);
                q.dCandRows = (int64_t*)ctx.alloc((size_t)topkCapacity * (size_t)q.groupRowWords * 8);
                q.candCapacity = topkCapacity; q.candRowWords = q.groupRowWords;
            }
            if (!topkScratchCleared) prepareTopCandidatesRange(ctx, q.dTopkHists);
        }
        if (!groupCountCleared) RSQ_HIP(hipMemsetAsync(q.dGroupCount, 0, 4, ctx.stream));
        // Wide group rows of which the statement wants a few (TPC-H Q10: 380 K groups of 40 words - string group values -, LIMIT 20): the
        // compaction writes [slot | sort key] per group, the one-launch selection fetches its candidates' rows from the table.  Whatever
        // then turns out to need every row (candidates that overflow or do not decide the answer) starts the execution over with full rows.
        narrowRows = preselect && q.groupRowWords > 8 && !q.narrowRowsOff && fusedSelectOk();
        if (narrowRows && q.narrowRowsCap < groupRowsAllocated) {
            if (q.dNarrowRows) ctx.free(q.dNarrowRows);
            q.dNarrowRows = nullptr; q.narrowRowsCap = 0;
            q.dNarrowRows = (int64_t*)ctx.alloc((size_t)groupRowsAllocated * 16);
            q.narrowRowsCap = groupRowsAllocated;
        }
        // string group values that stand in the entries by address (this execution's kernels wrote them so: not the interpreter's, and only
        // while every table of the dependency chain is a rank dictionary - the kernel's own run-time condition, codegen_agg.cpp)
        const int* deref = nullptr;
        int tabStride = nTab;
        if (h.dDeref && !interp) {
            bool holds = true;
            for (int t : h.derefCondTables) holds = holds && q.hashTables[(size_t)t]->rank;
            if (holds) { deref = h.dDeref; tabStride = h.compactStride > 0 ? h.compactStride : nTab; }
        }
        compactEntries(ctx, (const int64_t*)h.dAcc /* block 0 = first row */, h.capacity, h.dWords, nTab, h.aos, h.dAcc, h.nAccBlocks,
                       narrowRows ? q.dNarrowRows : q.dGroupRows, groupRowsAllocated, q.dGroupCount,
                       h.rank,
                       q.topkWord, q.topkIs32, q.topkDesc, preselect ? (uint64_t*)q.dTopkHists : nullptr, narrowRows, deref, tabStride);
        q.report.num_kernels++;
        if (narrowRows) {
            topkRange = true;
            const TableEntries te{(const int64_t*)h.dAcc, h.capacity, h.dWords, nTab, h.aos, h.dAcc, h.nAccBlocks, h.rank, deref, tabStride};
            selectTopCandidatesRangePublish(ctx, q.dNarrowRows, 2, 1, q.topkIs32, q.topkDesc, q.dGroupCount, groupRowsAllocated,
                                            q.topkWant, q.dTopkHists, q.dHostCandRows, topkCapacity, q.dPinnedDev + words, selectSeq = ++q.finSeqCounter, ctx.dErr, q.dGroupCount,
                                            anyCompaction ? q.dPipeStats : nullptr, (int)q.pipelines.size(), &te);
            q.report.num_kernels += 1;
            selectPublished = true;
            topkSpec = topkCapacity;
        } else
        if (preselect) {
            // the short form: the compaction collected the range of the sort key's images, ONE histogram over that range finds
            // the candidates (aot_kernels.hip); the exact radix select runs only if they overflow the buffer (below)
            topkRange = true;
            if (fusedSelectOk()) {
                // ... in one launch that also delivers the candidates and the status words to the host (aot_kernels.hip k_topk_range_select)
                selectTopCandidatesRangePublish(ctx, q.dGroupRows, q.groupRowWords, q.topkWord, q.topkIs32, q.topkDesc, q.dGroupCount, groupRowsAllocated,
                                                q.topkWant, q.dTopkHists, q.dHostCandRows, topkCapacity, q.dPinnedDev + words, selectSeq = ++q.finSeqCounter, ctx.dErr, q.dGroupCount,
                                                anyCompaction ? q.dPipeStats : nullptr, (int)q.pipelines.size());
                q.report.num_kernels += 1;
                selectPublished = true;
                topkSpec = topkCapacity;
            } else {
            selectTopCandidatesRange(ctx, q.dGroupRows, q.groupRowWords, q.topkWord, q.topkIs32, q.topkDesc, q.dGroupCount, groupRowsAllocated, q.topkWant,
                                     q.dTopkHists, q.dCandRows, topkCapacity);
            q.report.num_kernels += 2;
            // the leading candidates travel with the same synchronisation as the counts (usually that is all of them)
            topkSpec = std::min<uint32_t>(topkCapacity, std::max<uint32_t>(q.topkWant + 64, 65536u / (uint32_t)(q.groupRowWords * 8)));
            }
        }
    }
    // ORDER BY ... LIMIT k over a large DENSE aggregate table: the groups present are compacted into rows [first row | group id |
    // accumulator blocks] and go through the same candidate pre-selection; the table itself (tens of MB) is only read back
    // when the candidates do not decide the answer
    bool denseTopk = false;
    if (!partialOnly && !q.holdTail && q.aggMode == AggMode::DENSE_GLOBAL && q.aggPad == 1 && q.denseGroups >= 65536 && q.denseGroups <= (1 << 21)) {
        if (q.topkWord == -2) planDeviceTopK(q);
        if (q.topkWord >= 0) {
            const uint32_t D = (uint32_t)q.denseGroups;
            const int W = (int)q.accums.size();
            q.groupRowWords = 2 + W;
            groupRowsAllocated = D;
            const size_t need = (size_t)D * (size_t)q.groupRowWords;
            if (q.dGroupRowsWords < need) {
                if (q.dGroupRows) ctx.free(q.dGroupRows);
                q.dGroupRows = nullptr; q.dGroupRowsWords = 0;
                q.dGroupRows = (int64_t*)ctx.alloc(need * 8);
                q.dGroupRowsWords = need;
            }
            if (!q.dGroupCount) q.dGroupCount = (uint32_t*)ctx.alloc(sizeof(uint32_t));
            topkCapacity = std::min<uint32_t>(D, std::max<uint32_t>(1024, 4 * q.topkWant));
            if (!q.dTopkHists) { q.dTopkHists = (uint32_t*)ctx.alloc(topkHistBytes()); q.dCandCount = q.dTopkHists + 4; }
            if (q.candCapacity < topkCapacity || q.candRowWords != q.groupRowWords) {
                if (q.dCandRows) ctx.free(q.dCandRows);
                q.dCandRows = (int64_t*)ctx.alloc((size_t)topkCapacity * (size_t)q.groupRowWords * 8);
                q.candCapacity = topkCapacity; q.candRowWords = q.groupRowWords;
            }
            if (!topkScratchCleared) prepareTopCandidatesRange(ctx, q.dTopkHists);
            if (!groupCountCleared) RSQ_HIP(hipMemsetAsync(q.dGroupCount, 0, 4, ctx.stream));
            compactEntries(ctx, (const int64_t*)q.dAgg /* block 0 = first row */, (int64_t)D, nullptr, 1, false, (const int64_t*)q.dAgg, W,
                           q.dGroupRows, D, q.dGroupCount, false, q.topkWord, q.topkIs32, q.topkDesc, (uint64_t*)q.dTopkHists);
            topkRange = true;
            if (fusedSelectOk()) {
                selectTopCandidatesRangePublish(ctx, q.dGroupRows, q.groupRowWords, q.topkWord, q.topkIs32, q.topkDesc, q.dGroupCount, D, q.topkWant,
                                                q.dTopkHists, q.dHostCandRows, topkCapacity, q.dPinnedDev + words, selectSeq = ++q.finSeqCounter, ctx.dErr, q.dGroupCount,
                                                anyCompaction ? q.dPipeStats : nullptr, (int)q.pipelines.size());
                q.report.num_kernels += 2;
                selectPublished = true;
                topkSpec = topkCapacity;
            } else {
            selectTopCandidatesRange(ctx, q.dGroupRows, q.groupRowWords, q.topkWord, q.topkIs32, q.topkDesc, q.dGroupCount, D, q.topkWant,
                                     q.dTopkHists, q.dCandRows, topkCapacity);
            q.report.num_kernels += 3;
            topkSpec = std::min<uint32_t>(topkCapacity, std::max<uint32_t>(q.topkWant + 64, 65536u / (uint32_t)(q.groupRowWords * 8)));
            }
            denseTopk = true;
        }
    }
    // The execution's end event.  Where a status kernel follows, the event stands BEHIND it: an event between two kernels is a barrier
    // packet of its own and kept the status kernel waiting ~6 us (per-dispatch trace); behind the last kernel it delays nobody.
    const bool statusKernelFollows = !selectPublished && publishStatus;
    if (!statusKernelFollows) RSQ_HIP(hipEventRecord(q.gev1, ctx.stream));
    q.kernelTimePending = true;
    bool devTail = false;                   // the rows of a large dense aggregation are made on the device (runDenseDeviceTail)
    bool inlineRows = false;                // up to kInlineRows group rows arrive with the status words
    constexpr uint32_t kInlineRows = 64;
    // a small dense aggregate table (TPC-H Q14: one group behind a join) travels with the status words instead of a copy of its own
    const size_t tableInlineWords = q.aggPad > 1 && !q.flatRun ? (size_t)q.padWords : (size_t)q.tableWords;
    bool tableInline = false;
    if (!selectPublished) {
        const bool wantGroups = !partialOnly && (q.aggMode == AggMode::AT_JOIN_ENTRY || q.aggMode == AggMode::HASH || denseTopk);
        tableInline = statusKernelFollows && !partialOnly && denseMode(q) && !denseTopk && !trace && tableInlineWords > 0 && tableInlineWords <= 1024 && !(!async && denseDeviceTailWanted(q));
        if (publishStatus) {
            // error word, group count, candidate count and the pipelines' row counters: one kernel writes them into the pinned words
            if (wantGroups && !denseTopk && !topkCapacity && !q.holdTail && !trace && q.dGroupRows && q.groupRowWords > 0) {
                const size_t need = (size_t)kInlineRows * (size_t)q.groupRowWords;
                if (q.inlineRowsWords < need) {
                    if (q.hInlineRows) ctx.freePinned(q.hInlineRows);
                    q.hInlineRows = nullptr; q.dHostInlineRows = nullptr; q.inlineRowsWords = 0;
                    q.hInlineRows = (int64_t*)ctx.allocPinned(need * 8);
                    void* dv = nullptr;
                    if (hipHostGetDevicePointer(&dv, q.hInlineRows, 0) == hipSuccess && dv) { q.dHostInlineRows = (int64_t*)dv; q.inlineRowsWords = need; }
                    else (void)hipGetLastError();
                }
                inlineRows = q.dHostInlineRows != nullptr;
            }
            publishStatusAsync(ctx, q.dPinnedDev + words, ctx.dErr, wantGroups ? q.dGroupCount : nullptr, topkCapacity ? q.dCandCount : nullptr,
                               anyCompaction ? q.dPipeStats : nullptr, (int)q.pipelines.size(),
                               inlineRows ? q.dGroupRows : nullptr, q.groupRowWords, std::min<uint32_t>(kInlineRows, groupRowsAllocated), q.dHostInlineRows,
                               q.matWarmRun ? q.dMatTotal : nullptr,
                               tableInline ? (const uint64_t*)(q.aggPad > 1 && !q.flatRun ? q.dAggWork : q.dAgg) : nullptr, q.dPinnedDev, tableInline ? (uint32_t)tableInlineWords : 0u);
            RSQ_HIP(hipEventRecord(q.gev1, ctx.stream));
            q.report.num_kernels++;
        } else {
            RSQ_HIP(hipMemcpyAsync(q.hPinned + words, ctx.dErr, 4, hipMemcpyDeviceToHost, ctx.stream));
            if (wantGroups) RSQ_HIP(hipMemcpyAsync(q.hPinned + words + 1, q.dGroupCount, 4, hipMemcpyDeviceToHost, ctx.stream));
            if (anyCompaction) RSQ_HIP(hipMemcpyAsync(q.hPinned + words + 8, q.dPipeStats, q.pipelines.size() * 8, hipMemcpyDeviceToHost, ctx.stream));
            if (topkCapacity) RSQ_HIP(hipMemcpyAsync(q.hPinned + words + 2, q.dCandCount, 4, hipMemcpyDeviceToHost, ctx.stream));
        }
        devTail = !partialOnly && !async && denseMode(q) && !denseTopk && denseDeviceTailWanted(q);
        if (!partialOnly && denseMode(q) && !denseTopk && !devTail && !tableInline) enqueueTableReadback(q);
        if (topkCapacity) {
            ensureHostGroupRows(q, (size_t)topkCapacity * (size_t)q.groupRowWords);
            RSQ_HIP(hipMemcpyAsync(q.hGroupRows, q.dCandRows, (size_t)topkSpec * (size_t)q.groupRowWords * 8, hipMemcpyDeviceToHost, ctx.stream));
        }
    }
    if (async && partialOnly) {
        // everything is enqueued; the caller orders its own work (the group-by merge collective) behind it on the same
        // stream and finalizeQuery() does the one host synchronisation of the step
        q.pendingAsync = true; q.pendingFused = false;
        q.report.execution_time_ms = nowMs() - t0;
        return;
    }
    const bool execTraceOn = traceLevel.atLeast(2);       // host-side phases of an execution of the general path, averaged over 8
    const double tEnqueued = execTraceOn ? nowMs() : 0;
    bool sawSequence = false;
    if (selectPublished) {
        // candidates and status words are in host memory once the selection's sequence number is: watch that word instead of the
        // stream's completion (as the one-launch step does); hipStreamQuery now and then notices a failed launch
        volatile uint64_t* flag = q.hPinned + words + 4;
        const double deadline = nowMs() + 5.0;
        unsigned spins = 0;
        sawSequence = true;
        while (*flag != selectSeq) {
            if ((++spins & 1023u) == 0) {
                hipError_t e = hipStreamQuery(ctx.stream);
                if (e != hipSuccess && e != hipErrorNotReady) RSQ_HIP(e);
                if (e == hipSuccess || nowMs() > deadline) { waitForStream(ctx); sawSequence = false; break; }
            }
            __builtin_ia32_pause();
        }
        if (*flag != selectSeq) failRuntime("internal error: the candidate selection finished without publishing its sequence number");
        std::atomic_thread_fence(std::memory_order_acquire);
    } else waitForStream(ctx);
    if (!sawSequence) resolveKernelTime(q);      // (the stream is done: reading the events costs nothing now)
    const double tSeen = execTraceOn ? nowMs() : 0;
    auto execTrace = [&]() {
        if (!execTraceOn) return;
        static double acc[4] = {0, 0, 0, 0}; static int n = 0;
        const double tEnd = nowMs();
        resolveKernelTime(q);
        acc[0] += tEnqueued - t0; acc[1] += tSeen - tEnqueued; acc[2] += tEnd - tSeen; acc[3] += q.report.kernel_time_ms;
        if (++n == 8) {
            fprintf(stderr, "[rsq exec] enqueue %.1f us, enqueued -> stream done %.1f us, checks + tail %.1f us; first to last event on the stream %.1f us, %llu launches\n",
                    acc[0] / 8 * 1e3, acc[1] / 8 * 1e3, acc[2] / 8 * 1e3, acc[3] / 8 * 1e3, (unsigned long long)q.report.num_kernels);
            acc[0] = acc[1] = acc[2] = acc[3] = 0; n = 0;
        }
    };
    if (anyCompaction)      // a build pipeline that also ran its counting pass reports both passes: only ever an over-estimate
        for (size_t i = 0; i < q.pipelines.size(); i++) {
            Pipeline& p = q.pipelines[i];           // the first 64 workgroups report: scale to the grid
            if (p.compact) p.stage2Rows = (int64_t)((double)q.hPinned[words + 8 + i] * (double)std::max(1u, p.lastGrid) / (double)std::min(64u, std::max(1u, p.lastGrid)));
            // (every slice of a nested-loops join's inner range sends the same outer rows to stage 2: one of them counts)
            if (p.compact && p.nljSliced >= 0) p.stage2Rows /= std::max<int32_t>(1, q.nljs[(size_t)p.nljSliced].slices);
        }
    ctx.errWordClean = (uint32_t)q.hPinned[words] == 0;
    if (((uint32_t)q.hPinned[words] & 256u) && !async && !q.fusedSelectOff) {
        // a workgroup of the one-launch candidate selection gave up at a meeting point (aot_kernels.hip k_topk_range_select): its
        // candidates are void; this query takes the separate launches from now on and starts over
        q.fusedSelectOff = true;
        executeQuery(q, partialOnly, async);
        return;
    }
    if (((uint32_t)q.hPinned[words] & 128u) && !async) {
        // a workgroup of the one-launch rank index gave up waiting for its predecessor (aot_kernels.hip k_rank_blocks_chained): the
        // index is wrong (in range, never out of bounds); this query takes the two-launch index from now on and starts over
        q.chainedIndexOff = true;
        executeQuery(q, partialOnly, async);
        return;
    }
    if (((uint32_t)q.hPinned[words] & 64u) && !async) {
        // a rank dictionary met build rows it was not sized for (two rows with one key, or more rows than the sizing pass saw:
        // the build side's data changed): its tables go back to the hash form and the execution starts over
        bool any = false;
        for (auto& hp : q.hashTables) {
            HashTable& h = *hp;
            if (!h.rank) continue;
            any = true;
            ctx.free(h.dWords); ctx.free(h.dTemp); ctx.free(h.dTempUsed); ctx.free(h.dChunkTotal); ctx.free(h.dChunkBase);
            if (h.dAcc) ctx.free(h.dAcc);
            h.dWords = h.dTemp = nullptr; h.dAcc = nullptr; h.dTempUsed = h.dChunkTotal = h.dChunkBase = nullptr;
            h.rank = false; h.rankCapable = false; h.identity = false; h.capacity = 0; h.lastCount = 0;
            h.dupKeys = true;                      // (what the plan memo tells the next query of this shape)
        }
        if (any) { executeQuery(q, partialOnly, async); return; }
    }
    if (q.matWarmRun) {             // the write pass ran with the remembered total: it must be this execution's
        q.matWarmRun = false;
        if ((int64_t)q.hPinned[words + 3] != q.matLastTotal) { q.matLastTotal = -1; executeQuery(q, partialOnly, async); return; }
    }
    if (hashWarm) {
        HashTable& h = *q.hashTables[(size_t)q.aggTable];
        const uint32_t e = (uint32_t)q.hPinned[words];
        if (e & 2u) {               // the table overflowed (more groups than last time): four times the slots, on the careful path
            ctx.free(h.dState); ctx.free(h.dWords); ctx.free(h.dAcc);
            h.dState = nullptr; h.dWords = nullptr; h.dAcc = nullptr;
            if (h.capacity >= ((int64_t)1 << 31)) failRuntime("Hash table full");
            h.capacity *= 4; h.lastCount = 0;
            executeQuery(q, partialOnly, async);
            return;
        }
        if (((e & 32u) != 0) != q.charGroupsNeedMerge) { h.lastCount = 0; executeQuery(q, partialOnly, async); return; }      // (the careful path reads the note before it plans the tail)
    }
    checkDeviceError((uint32_t)q.hPinned[words]);
    // the short candidate selection overflowed its buffer (many rows share the leading bin): the exact radix select, now
    bool candOnHost = selectPublished;      // the candidates are in hCandRows (else: in hGroupRows, copied)
    auto exactCandidates = [&](uint32_t rowsBound) -> int64_t {
        candOnHost = false;
        if (q.topkImageRows < rowsBound) {
            if (q.dTopkImages) ctx.free(q.dTopkImages);
            q.dTopkImages = (uint64_t*)ctx.alloc((size_t)rowsBound * 8);
            q.topkImageRows = rowsBound;
        }
        selectTopCandidates(ctx, q.dGroupRows, q.groupRowWords, q.topkWord, q.topkIs32, q.topkDesc, q.dGroupCount, rowsBound, q.topkWant, q.dTopkImages,
                            q.dTopkHists, q.dCandRows, topkCapacity);
        uint32_t n = 0;
        RSQ_HIP(hipMemcpyAsync(&n, q.dCandCount, 4, hipMemcpyDeviceToHost, ctx.stream));
        waitForStream(ctx);
        if (n <= topkCapacity) {
            ensureHostGroupRows(q, (size_t)topkCapacity * (size_t)q.groupRowWords);
            RSQ_HIP(hipMemcpy(q.hGroupRows, q.dCandRows, (size_t)n * (size_t)q.groupRowWords * 8, hipMemcpyDeviceToHost));
        }
        return (int64_t)n;
    };
    if (!partialOnly) {
        double t1 = nowMs();
        if (denseTopk) {
            const int64_t nGroups = (int64_t)(uint32_t)q.hPinned[words + 1];
            if (nGroups == 0xffffffffll) failRuntime("internal error: the group-row compaction's look-back timed out");
            int64_t nCand = (int64_t)(uint32_t)q.hPinned[words + 2];
            if (topkRange && nCand > (int64_t)topkCapacity) { nCand = exactCandidates(groupRowsAllocated); topkSpec = topkCapacity; }
            const size_t rowBytes = (size_t)q.groupRowWords * 8;
            bool done = false;
            if (nCand <= (int64_t)topkCapacity && nCand < nGroups) {
                if (nCand > (int64_t)topkSpec)
                    RSQ_HIP(hipMemcpy((char*)q.hGroupRows + (size_t)topkSpec * rowBytes, (char*)q.dCandRows + (size_t)topkSpec * rowBytes,
                                      (size_t)(nCand - topkSpec) * rowBytes, hipMemcpyDeviceToHost));
                q.candidateRun = true;
                q.nGroupRows = nCand; q.totalGroups = nGroups;
                q.hRowsView = candOnHost ? q.hCandRows : nullptr;
                tailUnlessHeld(q);
                q.hRowsView = nullptr;
                q.candidateRun = false;
                done = !q.tailNeedsAllGroups;
            }
            if (!done) {            // the candidates do not decide it: the whole table after all
                enqueueTableReadback(q);
                waitForStream(ctx);
                tableFromPinned(q);
                tailUnlessHeld(q);
            }
            q.report.finalize_time_ms = nowMs() - t1;
            q.report.execution_time_ms = nowMs() - t0;
            return;
        }
        if (devTail) {
            q.report.finalize_time_ms = runDenseDeviceTail(q);
            checkDeviceError((uint32_t)q.hPinned[words]);
            q.report.execution_time_ms = nowMs() - t0;
            return;
        }
        if (denseMode(q)) tableFromPinned(q);
        else if (q.matOp && !q.agg) {
            if (runMaterializeDeviceTail(q)) {          // (a device tail made the result relation: no column travels whole)
                q.report.finalize_time_ms = nowMs() - t1;
                q.report.execution_time_ms = nowMs() - t0;
                execTrace();
                return;
            }
            q.hMatCols.resize(q.matSchema.size());
            for (size_t c = 0; c < q.matSchema.size(); c++) {
                size_t bytes = (size_t)q.matRows * (size_t)columnWidth(q.matSchema[c].type);
                q.hMatCols[c].resize(bytes);
                if (bytes && c < q.hMatMapped.size() && q.hMatMapped[c]) memcpy(q.hMatCols[c].data(), q.hMatMapped[c], bytes);      // (written by the device, complete with the stream)
                else if (bytes) RSQ_HIP(hipMemcpy(q.hMatCols[c].data(), q.dMatCols[c], bytes, hipMemcpyDeviceToHost));
            }
        } else {
            const int64_t nGroups = (int64_t)(uint32_t)q.hPinned[words + 1];
            if (nGroups == 0xffffffffll) failRuntime("internal error: the group-row compaction's look-back timed out");
            if (nGroups > (int64_t)groupRowsAllocated) {
                // more groups than the remembered entry count provided for (the build side changed under us): start over
                q.hashTables[(size_t)q.aggTable]->lastCount = 0;
                if (q.aggMode != AggMode::AT_JOIN_ENTRY && !hashWarm) failRuntime("internal error: more groups than hash-table entries");
                executeQuery(q, partialOnly, async);
                return;
            }
            if (q.aggMode == AggMode::HASH) q.hashTables[(size_t)q.aggTable]->lastCount = (uint32_t)nGroups;      // (what the next execution provides for)
            int64_t nCand = topkCapacity ? (int64_t)(uint32_t)q.hPinned[words + 2] : 0;
            if (narrowRows && nCand > (int64_t)topkCapacity) { q.narrowRowsOff = true; executeQuery(q, partialOnly, async); return; }      // (the exact selection reads full rows)
            if (topkRange && nCand > (int64_t)topkCapacity) { nCand = exactCandidates(groupRowsAllocated); topkSpec = topkCapacity; }
            const size_t rowBytes = (size_t)q.groupRowWords * 8;
            q.candidateRun = false;
            if (topkCapacity && nCand <= (int64_t)topkCapacity && nCand < nGroups) {
                const bool postClear = true;
                if (postClear && candOnHost && !trace && !interp && !q.holdTail) {
                    // the candidates are on the host and decide the answer (or the whole table is read below from buffers the clears
                    // leave alone): ready the next execution now, while the host does its tail
                    fillBatchAsync(ctx, f.data(), (int)f.size());
                    q.report.num_kernels += (f.size() + 23) / 24;
                    q.readied = true; q.readiedEpoch = ctx.execEpoch; q.readiedFill = f;
                }
                if (nCand > (int64_t)topkSpec)
                    RSQ_HIP(hipMemcpy((char*)q.hGroupRows + (size_t)topkSpec * rowBytes, (char*)q.dCandRows + (size_t)topkSpec * rowBytes,
                                      (size_t)(nCand - topkSpec) * rowBytes, hipMemcpyDeviceToHost));
                q.candidateRun = true;
                q.nGroupRows = nCand; q.totalGroups = nGroups;
                q.hRowsView = candOnHost ? q.hCandRows : nullptr;
                tailUnlessHeld(q);
                q.hRowsView = nullptr;
                q.candidateRun = false;
            }
            if (!topkCapacity || q.tailNeedsAllGroups || !(nCand <= (int64_t)topkCapacity && nCand < nGroups)) {
                if (narrowRows) { q.narrowRowsOff = true; executeQuery(q, partialOnly, async); return; }      // (every row is needed: none was written)
                q.nGroupRows = nGroups;
                if (rowsDeviceTailWanted(q, nGroups)) runRowsDeviceTail(q, nGroups);      // many groups: the rows are made on the device
                else if (inlineRows && nGroups <= (int64_t)std::min<uint32_t>(kInlineRows, groupRowsAllocated)) {      // (the rows came with the status words)
                    q.hRowsView = q.hInlineRows;
                    tailUnlessHeld(q);
                    q.hRowsView = nullptr;
                }
                else {
                    if (q.nGroupRows && !(q.holdTail && q.holdTailOnDevice)) {
                        ensureHostGroupRows(q, (size_t)q.nGroupRows * (size_t)q.groupRowWords);
                        RSQ_HIP(hipMemcpy(q.hGroupRows, q.dGroupRows, (size_t)q.nGroupRows * rowBytes, hipMemcpyDeviceToHost));
                    }
                    tailUnlessHeld(q);
                }
            }
            q.report.finalize_time_ms = nowMs() - t1;
            q.report.execution_time_ms = nowMs() - t0;
            execTrace();
            return;
        }
        tailUnlessHeld(q);
        resultPackHostRelation(q);
        q.report.finalize_time_ms = nowMs() - t1;
    }
    q.report.execution_time_ms = nowMs() - t0;
    execTrace();
}

void finalizeQuery(Query& q) {
    Context& ctx = q.ctx;
    if (!q.derived.empty() && !derivedExternal(q)) refuseDerived(q, "finalize");
    if (!partialCapable(q)) failUnsupported("partial execution / finalize is available for dense aggregations only");
    RSQ_HIP(hipSetDevice(ctx.device));
    double t1 = nowMs();
    const bool devTail = !q.mergePublishedSeq && denseDeviceTailWanted(q);
    double devTailMs = 0;
    if (q.mergePublishedSeq) {
        // the merge kernel stored the merged table into host-mapped memory: watch for its sequence number (see the fused step)
        const uint64_t seq = q.mergePublishedSeq;
        q.mergePublishedSeq = 0;
        volatile uint64_t* flag = q.hPinned + q.pinnedWords + 3;
        const double deadline = nowMs() + 5.0;
        unsigned spins = 0;
        while (*flag != seq) {
            if ((++spins & 1023u) == 0) {
                hipError_t e = hipStreamQuery(ctx.stream);
                if (e != hipSuccess && e != hipErrorNotReady) RSQ_HIP(e);
                if (e == hipSuccess || nowMs() > deadline) { waitForStream(ctx); break; }
            }
            __builtin_ia32_pause();
        }
        if (*flag != seq) failRuntime("internal error: the merge kernel finished without publishing its table");
        std::atomic_thread_fence(std::memory_order_acquire);
    } else if (devTail) {
        devTailMs = runDenseDeviceTail(q);          // (waits for the step's kernels and its merge first)
    } else {
        RSQ_HIP(hipMemcpyAsync(q.hPinned, q.dAgg, q.tableWords * 8, hipMemcpyDeviceToHost, ctx.stream));
        waitForStream(ctx);
    }
    if (q.pendingAsync) {         // the step was enqueued by rsq_query_execute_partial_async: account for it now
        q.pendingAsync = false;
        float ms = 0;
        RSQ_HIP(hipEventElapsedTime(&ms, q.gev0, q.gev1)); q.kernelTimePending = false;      // (one-launch step or not: the query's own event pair)
        if (q.pendingFused) q.fusedReady = true;
        q.report.kernel_time_ms = ms; q.kernelTimeSumMs += ms; q.kernelTimeLaunches++;
        noteRowCellsTime(q, q.pairForm, ms); q.pairForm = -1;
        q.report.hbm_gbps = ms > 0 ? (double)q.report.bytes_read / (ms * 1e-3) / 1e9 : 0;
        if (!q.pendingFused) ctx.errWordClean = (uint32_t)q.hPinned[q.pinnedWords] == 0;
        checkAsyncDeviceError((uint32_t)q.hPinned[q.pinnedWords]);
    }
    if (devTail) { checkDeviceError((uint32_t)q.hPinned[q.pinnedWords]); q.report.finalize_time_ms = devTailMs; return; }
    t1 = nowMs();          // (the wait for the step's kernels and its merge is not the host tail)
    if (q.tableWords >= (1u << 16)) q.hAggView = q.hPinned;      // (see tableFromPinned)
    else { q.hAggView = nullptr; memcpy(q.hAgg.data(), q.hPinned, q.tableWords * 8); }
    runTail(q);
    q.report.finalize_time_ms = nowMs() - t1;
}

// a rank of a multi-GPU step that does not finalise (only the root reads the merged table back): wait for its enqueued
// step, account for the kernel time, check its device error word
void settleAsync(Query& q) {
    Context& ctx = q.ctx;
    if (!q.pendingAsync) return;
    RSQ_HIP(hipSetDevice(ctx.device));
    waitForStream(ctx);
    q.pendingAsync = false;
    float ms = 0;
    RSQ_HIP(hipEventElapsedTime(&ms, q.gev0, q.gev1)); q.kernelTimePending = false;
    if (q.pendingFused) q.fusedReady = true;
    q.report.kernel_time_ms = ms; q.kernelTimeSumMs += ms; q.kernelTimeLaunches++;
    noteRowCellsTime(q, q.pairForm, ms); q.pairForm = -1;
    q.report.hbm_gbps = ms > 0 ? (double)q.report.bytes_read / (ms * 1e-3) / 1e9 : 0;
    if (!q.pendingFused) ctx.errWordClean = (uint32_t)q.hPinned[q.pinnedWords] == 0;
    checkAsyncDeviceError((uint32_t)q.hPinned[q.pinnedWords]);
}

// Results of the same plan over disjoint shards (every group lives in exactly one shard: the caller shards on the group key)
// become one result in `into`: the rows of all parts in part order, then the root's ORDER BY (multi-key, typed compare as
// the reference's Quicksorter, types.h:264-353; ties keep part order) and its LIMIT (orderby.h:87-93; materialize.h:197-206).
void mergeShardResults(Query& into, const std::vector<Query*>& parts) {
    const Schema& sch = into.resultSchema;
    const size_t ts = (size_t)schemaTupleSize(sch);
    std::vector<uint8_t> all;
    int64_t rows = 0;
    for (Query* p : parts) {
        if ((size_t)schemaTupleSize(p->resultSchema) != ts) failInvalid("shard results have different schemas");
        all.insert(all.end(), p->resultTuples.begin(), p->resultTuples.begin() + (size_t)p->resultRows * ts);
        rows += p->resultRows;
    }
    OpNode* root = into.root;
    if (root && root->tag == RSQ_OP_ORDERBY) {
        std::vector<OrderRequest> reqs;
        for (Expr* e : root->exprs) {
            const std::string& nm = e->child->symbol;
            bool found = false;
            for (auto& a : sch) if (a.name == nm) { reqs.push_back({schemaOffset(sch, nm), a.type, e->tag != RSQ_E_DESC}); found = true; break; }
            if (!found) failType("Order By attribute not found.");
        }
        std::vector<int64_t> idx((size_t)rows);
        for (int64_t i = 0; i < rows; i++) idx[(size_t)i] = i;
        std::stable_sort(idx.begin(), idx.end(), [&](int64_t a, int64_t b) {
            const uint8_t* l = all.data() + (size_t)a * ts; const uint8_t* r = all.data() + (size_t)b * ts;
            for (const auto& o : reqs) {
                int c = compareTyped(o.type, l + o.offset, r + o.offset);
                if (c) return o.asc ? c < 0 : c > 0;
            }
            return false;
        });
        if (root->hasLimit && rows > root->limit) rows = std::max<int64_t>(root->limit, 0);
        into.resultTuples.resize((size_t)rows * ts);
        for (int64_t i = 0; i < rows; i++) memcpy(&into.resultTuples[(size_t)i * ts], all.data() + (size_t)idx[(size_t)i] * ts, ts);
    } else {
        if (root && root->hasLimit) rows = std::min<int64_t>(rows, std::max<int64_t>(root->limit, 1));
        all.resize((size_t)rows * ts);
        into.resultTuples.swap(all);
    }
    into.resultRows = rows;
}

void setHoldTail(Query& q, bool hold) { q.holdTail = hold; }
bool queryOrderedWithLimit(const Query& q) { return q.root && q.root->tag == RSQ_OP_ORDERBY && q.root->hasLimit; }
bool queryAsyncCapable(const Query& q) {
    if (!partialCapable(q)) return false;
    for (auto& p : q.pipelines) if (p.sink != SinkKind::AGGREGATE) return false;
    return true;
}

// Can a group of this plan occur in two shards?  Not if one of the group-by values is a plain attribute of a scanned table whose
// [min, max] ranges (column statistics of every shard's instance of that table) do not overlap between the shards: the caller
// sharded on a boundary of that key.  `why` names the attribute, or says what was missing.
bool shardGroupsDisjoint(const std::vector<Query*>& parts, std::string& why) {
    if (parts.empty() || !parts[0]->agg) { why = "no aggregation"; return false; }
    const Query& q0 = *parts[0];
    for (Expr* g : q0.agg->exprs2) {
        if (g->tag != RSQ_E_ATTRIBUTE) continue;
        std::vector<std::pair<int64_t, int64_t>> ranges;
        bool usable = true;
        for (size_t i = 0; i < parts.size() && usable; i++) {
            const Table* tab = nullptr; int col = -1;
            for (Table* t : parts[i]->tables) { int c = t->findCol(g->symbol); if (c >= 0) { tab = t; col = c; break; } }
            for (const DerivedState& d : parts[i]->derived)
                if (d.table->findCol(g->symbol) >= 0) {
                    // (its columns have no statistics, and a merged or local derived table holds the same groups on every shard)
                    why = "group key " + g->symbol + " comes from a derived table"; tab = nullptr; break;
                }
            if (!tab) { usable = false; break; }
            if (std::find(parts[i]->gatheredTables.begin(), parts[i]->gatheredTables.end(), tab) != parts[i]->gatheredTables.end()) {
                // (the gathered inner side of a nested-loops join: every shard pairs with ALL of its rows, whatever its own rows hold)
                why = "group key " + g->symbol + " comes from a gathered inner side, which every shard sees whole";
                usable = false; break;
            }
            if (tab->nRows == 0) continue;
            const ColumnStats& st = tab->shardStats((size_t)col);      // what THIS shard's rows hold (stats may be the union over all shards)
            if (!st.valid || !st.distinctBytes.empty() || tab->cols[(size_t)col].type.isString()) { usable = false; break; }
            ranges.emplace_back(st.min, st.max);
        }
        if (!usable) continue;
        std::sort(ranges.begin(), ranges.end());
        bool disjoint = true;
        for (size_t i = 1; i < ranges.size(); i++) if (ranges[i].first <= ranges[i - 1].second) disjoint = false;
        if (disjoint) { why = "group key " + g->symbol + " has disjoint value ranges on the shards"; return true; }
        why = "the value ranges of group key " + g->symbol + " overlap between shards";
    }
    if (why.empty()) why = "no group key is a plain integer attribute with column statistics";
    return false;
}

void finalizeQueryHost(Query& q, const int64_t* words, size_t nWords) {
    if (!q.derived.empty()) refuseDerived(q, "finalize");
    if (!partialCapable(q)) failUnsupported("host finalize is available for dense aggregations only");
    size_t need = q.accums.size() * (size_t)q.denseGroups;
    if (nWords != need) failInvalid("partial table has " + std::to_string(nWords) + " words, expected " + std::to_string(need));
    q.hAgg.assign((const uint64_t*)words, (const uint64_t*)words + nWords);
    q.hAggView = nullptr;
    runTail(q);
}

void bindPartial(Query& q, void* dptr, size_t bytes) {
    if (!partialCapable(q)) failUnsupported("partial tables exist for dense aggregations only");
    size_t need = q.accums.size() * (size_t)q.denseGroups * 8;
    if (!dptr || bytes < need) failInvalid("partial buffer too small: need " + std::to_string(need) + " bytes");
    if (q.dAgg && q.dAggOwned) q.ctx.free(q.dAgg);
    q.dAgg = (uint64_t*)dptr;
    q.dAggOwned = false;
    for (auto& p : q.pipelines) if (p.sink == SinkKind::AGGREGATE && p.src->nRowsTotal < 0) q.firstRowsForeign = true;      // (the caller's collectives write into it)
}

// the kernel behind the merge collective: `gathered` = every rank's partial table back to back (one all-gather), reduced by
// segment into this query's own partial table; enqueued on the context's stream, no synchronisation
void mergeGathered(Query& q, const void* gathered, int nRanks) {
    if (!partialCapable(q)) failUnsupported("partial tables exist for dense aggregations only");
    if (!gathered || nRanks < 1) failInvalid("merge needs the gathered tables of at least one rank");
    if (q.ctx.device < 0) throw Error(RSQ_ERR_DEVICE, "this context has no device (compile-only)");
    RSQ_HIP(hipSetDevice(q.ctx.device));
    const int64_t G = q.denseGroups;
    if (nRanks > 1) for (auto& p : q.pipelines) if (p.sink == SinkKind::AGGREGATE && p.src->nRowsTotal < 0) q.firstRowsForeign = true;
    // small tables: the merge kernel also publishes the result to host-mapped memory (finalizeQuery polls for it)
    const bool publish = sw::flag<sw::RSQ_POLL>() && q.dFinHost && q.tableWords <= 2048;
    q.mergePublishedSeq = publish ? ++q.finSeqCounter : 0;
    mergePartialsAsync(q.ctx, (const int64_t*)gathered, nRanks, (int64_t)q.tableWords, q.nMinBlocks * G, q.nMaxBlocks * G, q.nSumBlocks * G, (int64_t*)q.dAgg,
                       publish ? (int64_t*)q.dFinHost : nullptr, publish ? q.dFinHost + q.pinnedWords + 3 : nullptr, q.mergePublishedSeq);
}

void partialBuffer(Query& q, void** dptr, int64_t* nMin, int64_t* nMax, int64_t* nSum) {
    if (!partialCapable(q)) failUnsupported("partial tables exist for dense aggregations only");
    *dptr = q.dAgg;
    *nMin = q.nMinBlocks * q.denseGroups;
    *nMax = q.nMaxBlocks * q.denseGroups;
    *nSum = q.nSumBlocks * q.denseGroups;
}

void queryResult(Query& q, rsq_result_view* out) {
    size_t n = q.resultSchema.size();
    q.rvNames.assign(n * RSQ_SYMBOL_MAX + 1, 0);
    q.rvTypes.resize(n); q.rvOffsets.resize(n);
    int off = 0;
    for (size_t i = 0; i < n; i++) {
        snprintf(&q.rvNames[i * RSQ_SYMBOL_MAX], RSQ_SYMBOL_MAX, "%s", q.resultSchema[i].name.c_str());
        q.rvTypes[i] = q.resultSchema[i].type.toC();
        q.rvOffsets[i] = off;
        off += sizeInTuple(q.resultSchema[i].type, true);
    }
    out->n_cols = (int32_t)n;
    out->names = reinterpret_cast<const char(*)[RSQ_SYMBOL_MAX]>(q.rvNames.data());
    out->types = q.rvTypes.data();
    out->offsets = q.rvOffsets.data();
    out->tuple_size = off;
    out->n_rows = q.resultRows;
    out->tuples = q.resultInPinned ? q.resultPinned : q.resultTuples.data();
}

void queryReport(const Query& q, rsq_report* out) {
    resolveKernelTime(const_cast<Query&>(q));
    *out = q.report;
}
int32_t queryNestedLoopsSlices(const Query& q) {
    for (const NljState& n : q.nljs) if (n.sub.query && n.outerSrc) return n.slices;      // (the top one: the others run inside its inner side)
    return 0;
}
void queryKernelTimeStats(Query& q, double* sumMs, uint64_t* executions, bool reset) {
    resolveKernelTime(q);
    if (sumMs) *sumMs = q.kernelTimeSumMs;
    if (executions) *executions = q.kernelTimeLaunches;
    if (reset) { q.kernelTimeSumMs = 0; q.kernelTimeLaunches = 0; }
}
bool queryIsDense(const Query& q) { return partialCapable(q); }
void queryDenseLayout(const Query& q, int64_t* nMin, int64_t* nMax, int64_t* nSum, void** dptr) {
    if (!partialCapable(q)) failUnsupported("partial tables exist for dense aggregations only");
    *dptr = q.dAgg;
    *nMin = q.nMinBlocks * q.denseGroups; *nMax = q.nMaxBlocks * q.denseGroups; *nSum = q.nSumBlocks * q.denseGroups;
}
std::string queryPartialLayoutText(const Query& q) {
    size_t at = q.explainText.find("partial table:");
    if (at == std::string::npos) return "";
    size_t end = q.explainText.find('\n', at);
    std::string text = q.explainText.substr(at, end == std::string::npos ? std::string::npos : end - at);
    // ... and what explain leaves out: the entries behind a coded key's ranks, as their count and a 64-bit digest of their bytes (shards whose
    // dictionaries differ must never merge their tables cell by cell)
    for (auto& k : q.denseKeys)
        if (k.coded) {
            char hex[17];
            snprintf(hex, sizeof hex, "%016llx", (unsigned long long)fnv1a64(std::string(k.dict.begin(), k.dict.end())));
            text += " dictionary " + k.expr->symbol + "=" + std::to_string((long long)k.card) + ":" + hex;
        }
    return text;
}
const char* querySource(const Query& q) { return q.allSource.c_str(); }
// (the line about the register aggregation's form is composed here from the pipelines' state: nothing is kept inside explainText)
const char* queryExplain(const Query& q) {
    const std::string form = rowCellsLine(q);
    if (form.empty()) return q.explainText.c_str();
    q.explainWithForm = q.explainText + form;
    return q.explainWithForm.c_str();
}
void destroyQuery(Query* q) { delete q; }

}  // namespace rsq
