// multi.cpp — one host process, N GPUs: the rsq_multi_* part of include/resql_hip.h.
//
// The reference's execute() fans one compiled function out to config.numThreads worker threads that pull morsels from a
// shared iterator, and joins them (reference src/JitContextFlounder.h:459-487); its aggregation state is one hash table
// all workers reach.  Across GPUs the morsels are row-range shards resident in each GPU's HBM, every GPU runs the same
// compiled pipelines to a partial aggregate table, and the one exchange step is the group-by merge of those tables:
// an RCCL reduce over xGMI to the root GPU — ncclReduce per [min | max | sum] segment, grouped into one launch per GPU —
// issued from this process through communicators made by ncclCommInitAll.  librccl is loaded with dlopen when the first
// multi-GPU handle is created, so that hosts with one GPU (and machines without RCCL) never need it.
//
// A second merge path gathers the partial tables on the root GPU and reduces them with the engine's own merge kernel (no RCCL,
// shard_exchange.h mergeDenseOnRoot): chosen with rsq_multi_config.merge = RSQ_MERGE_PEER_COPY, and the only one possible when a
// device ordinal is listed twice — which is how a box with ONE GPU exercises N-shard execution end to end (tests).
//
// Plans that do not end in a dense partial table (joins with many groups, hash aggregation, plain materialisation) run
// whole on every shard in parallel host threads; the shards must then be disjoint in the group key (the caller shards the
// probe-side table on a key boundary and replicates the build sides), and the merge is a host-side ordered
// merge of the (LIMIT-ed) result rows.
//
// Whatever passes between shards here - events, gathers, the dense merge, peer access, the shards' host threads - is shard_exchange.h's.
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstring>
#include <set>

#include "engine_internal.h"
#include "shard_exchange.h"

using namespace rsq;

namespace {

struct RcclApi {
    void* handle = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*Reduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};

RcclApi& rccl() {
    static RcclApi api;
    if (api.handle) return api;
    // a process that already has an RCCL (PyTorch brings its own) keeps using that one: same SONAME, same handle
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void* h = nullptr;
    for (const char* n : names) { h = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (h) break; }
    if (!h) throw Error(RSQ_ERR_DEVICE, std::string("cannot load librccl: ") + dlerror());
    auto sym = [&](const char* n) { void* p = dlsym(h, n); if (!p) throw Error(RSQ_ERR_DEVICE, std::string("librccl lacks ") + n); return p; };
    api.CommInitAll = (decltype(api.CommInitAll))sym("ncclCommInitAll");
    api.CommDestroy = (decltype(api.CommDestroy))sym("ncclCommDestroy");
    api.Reduce = (decltype(api.Reduce))sym("ncclReduce");
    api.GroupStart = (decltype(api.GroupStart))sym("ncclGroupStart");
    api.GroupEnd = (decltype(api.GroupEnd))sym("ncclGroupEnd");
    api.GetErrorString = (decltype(api.GetErrorString))sym("ncclGetErrorString");
    api.handle = h;
    return api;
}

#define RSQ_NCCL(call)                                                                                          \
    do {                                                                                                        \
        ncclResult_t _r = (call);                                                                               \
        if (_r != ncclSuccess) throw Error(RSQ_ERR_DEVICE, std::string(#call) + ": " + rccl().GetErrorString(_r)); \
    } while (0)

thread_local std::string g_multiCreateError;

}  // namespace

struct rsq_multi {
    std::vector<Context*> ctxs;
    std::vector<int> devices;
    bool sharedDevice = false;          // a device ordinal is listed more than once (tests on one GPU)
    int merge = RSQ_MERGE_RCCL;
    std::vector<ncclComm_t> comms;      // RCCL mode, one per device
    std::string lastError;
    ~rsq_multi() {
        for (ncclComm_t c : comms) if (c) (void)rccl().CommDestroy(c);
        for (Context* c : ctxs) delete c;
    }
};

// a nested-loops join (see "Nested-loops joins across GPUs" below): its pair space split by the outer side's rows
struct NljSplit {
    bool gathered = false;              // the inner side is sharded: every shard's part is all-gathered into every shard (else replicated)
    std::vector<std::unique_ptr<Table>> outerSlices;      // a replicated outer table: shard i's slice of its copy (views, no rows of their own)
    std::vector<ShardEvent> innerDone;  // shard i's inner part is materialised (the gather's copies wait for it)
    std::vector<ShardEvent> gather0, gather1;             // around the gather's copies on shard i's stream
    int64_t gatherBytes = -1;           // moved between shards by the last gather (-1: none has run)
};

struct rsq_multi_query {
    rsq_multi* m = nullptr;
    std::vector<Query*> qs;             // one compiled query per device, same plan
    bool dense = false;
    bool async = false;                 // dense and every pipeline can be enqueued without the host in between (no join builds)
    bool orderedFast = false;           // not dense: shards provably disjoint in a group key + ORDER BY ... LIMIT: merge of the shards' ordered rows
    std::string mergeText;              // which merge this query takes, and why (composeMergeText)
    std::string mergeBase, derivedText; // ... its parts: the merge of the plan's kind, the derived tables' splits
    int64_t* gathered = nullptr;        // peer-copy mode: [n][words] on the root device
    std::vector<ShardEvent> ready;      // peer-copy mode: shard i's partial table is complete (none for the root)
    rsq_report report{};
    std::vector<double> shardKernelMs;
    ShardEvent evMerge0, evMerge1;      // on the root's stream, around the group-by merge of the last execution
    double collectiveMs = 0;
    bool nlj = false;
    NljSplit split;
    // derived aggregations (engine_derived_multi.cpp): built on every shard in front of the parent's pipelines
    bool derived = false;
    double derivedMs = 0;               // the last execution's exchanges (part of the collective time)
    ~rsq_multi_query() {
        if (gathered) { (void)hipSetDevice(m->ctxs[0]->device); m->ctxs[0]->free(gathered); }
        for (Query* q : qs) destroyQuery(q);
    }
};

namespace {

template <typename F>
int guardedM(rsq_multi* m, F&& f) {
    try { f(); return RSQ_OK; }
    catch (const Error& e) { if (m) m->lastError = e.what(); else g_multiCreateError = e.what(); return e.status; }
    catch (const std::bad_alloc&) { if (m) m->lastError = "out of host memory"; return RSQ_ERR_NOMEM; }
    catch (const std::exception& e) { if (m) m->lastError = e.what(); else g_multiCreateError = e.what(); return RSQ_ERR_INVALID; }
}

// mergeText: how the shards run in front of the merge (a nested-loops split with the last gather's bytes, the derived tables' splits),
// then the merge of the plan's kind
void composeMergeText(rsq_multi_query& mq) {
    const int n = (int)mq.m->ctxs.size();
    const int64_t bytes = mq.split.gatherBytes;
    std::string s;
    if (mq.nlj)
        s = "nested-loops: outer rows over " + std::to_string(n) + (n == 1 ? " shard" : " shards") + ", inner side " +
            (!mq.split.gathered ? "replicated" : bytes < 0 ? "gathered (peer copies)" : "gathered (peer copies, " + std::to_string((long long)bytes) + " bytes)") + "; ";
    if (mq.derived) s += "derived tables: " + mq.derivedText + "; ";
    mq.mergeText = s + mq.mergeBase;
}

// the group-by merge of one step, enqueued behind every shard's kernels; returns after enqueueing.  An event pair on the root's stream
// brackets it: rsq_multi_query_collective_ms (from the root's last kernel to the merged table, i.e. including the wait for the slowest
// shard).  A single shard without a communicator has no such events and nothing to merge.
void enqueueMerge(rsq_multi_query& mq) {
    rsq_multi& m = *mq.m;
    const int n = (int)m.ctxs.size();
    if (!mq.evMerge0.get()) return;
    mq.evMerge0.record(m.ctxs[0]->stream);
    if (m.merge == RSQ_MERGE_RCCL) {
        // one reduce per non-empty segment to the root (device 0, in place), all of them for all GPUs in ONE group:
        // RCCL launches a single kernel per GPU for the group.  Integer min / max / sum: bit-exact in any order.
        RcclApi& R = rccl();
        int64_t cnt[3];
        std::vector<void*> part((size_t)n);
        for (int i = 0; i < n; i++) queryDenseLayout(*mq.qs[(size_t)i], &cnt[0], &cnt[1], &cnt[2], &part[(size_t)i]);      // (one layout: the compile checked it)
        const int64_t off[3] = {0, cnt[0], cnt[0] + cnt[1]};
        const ncclRedOp_t op[3] = {ncclMin, ncclMax, ncclSum};
        RSQ_NCCL(R.GroupStart());
        for (int i = 0; i < n; i++)
            for (int s = 0; s < 3; s++)
                if (cnt[s] > 0)
                    RSQ_NCCL(R.Reduce((int64_t*)part[(size_t)i] + off[s], (int64_t*)part[(size_t)i] + off[s], (size_t)cnt[s], ncclInt64, op[s], 0,
                                      m.comms[(size_t)i], m.ctxs[(size_t)i]->stream));
        RSQ_NCCL(R.GroupEnd());
    } else {
        // peer copies: every shard's table, complete behind an event on its stream, to the root's gather buffer and through the merge kernel
        for (int i = 1; i < n; i++) mq.ready[(size_t)i].record(m.ctxs[(size_t)i]->stream);
        mergeDenseOnRoot(mq.qs, mq.ready, mq.gathered, "internal: shards planned from the same statistics disagree on the aggregation strategy");
    }
    mq.evMerge1.record(m.ctxs[0]->stream);
}

// ---- Nested-loops joins across GPUs ---------------------------------------------------------------------------------------------
// The pair space is split by the OUTER side's rows: every shard pairs its outer rows with the WHOLE inner side, in the reference's inner
// order.  Outer rows are numbered over the whole table (row0) and inner positions over the whole inner side, so a shard's pair ordinals
// (outer row x inner rows + inner position, codegen.cpp consumeNestedLoops) and first-row trackers are the one-context ones, and the
// dense or the general merge gives the one-context bytes.
//   outer side (the table the join's pipeline scans): sharded - each shard scans its own rows; replicated - each shard scans the slice
//              rsq_multi_shard_rows of its copy, through a view with its own identity (key indexes and the plan memo key on uid, row0, rows);
//   inner side (the left subtree, a query of its own): every table replicated - computed on every shard; exactly one table sharded, and
//              it is the source of the inner side's materialising pipeline - each shard computes its part, and the parts are all-gathered
//              in shard order with peer copies.  Everything else (a sharded build side, two sharded inner tables, a sharded table under a
//              nested inner side) is refused.

// the child an operator's pipeline continues through (codegen.cpp Walker::produce: a hash join's probe side and a nested-loops join's
// outer side continue the pipeline, every other operator its one child), and the scan the pipeline starts at
int pipelineChild(const rsq_op& o) { return o.tag == RSQ_OP_HASHJOIN || o.tag == RSQ_OP_NESTEDLOOPSJOIN ? o.child[1] : o.child[0]; }
int pipelineScan(const rsq_plan_desc& p, int op) {
    for (int steps = 0; op >= 0 && op < p.n_ops && steps <= p.n_ops; steps++, op = pipelineChild(p.ops[op]))
        if (p.ops[op].tag == RSQ_OP_SCAN) return op;
    failInvalid("malformed plan: an operator chain ends without a scan");
}
void subtreeOps(const rsq_plan_desc& p, int op, std::vector<int>& out) {
    if (op < 0 || op >= p.n_ops) failInvalid("malformed plan: operator index out of range");
    if (std::find(out.begin(), out.end(), op) != out.end()) return;
    out.push_back(op);
    for (int k = 0; k < 2; k++) if (p.ops[op].child[k] >= 0) subtreeOps(p, p.ops[op].child[k], out);
}

// Decides how a nested-loops plan is split (the rules above).  `sharded[t]`: table t's instances differ between the shards.  Returns the
// plan operator of the outer side's scan; `gatheredTable` is the sharded inner table (-1: the inner side is replicated).
int planNestedLoopsSplit(rsq_multi& m, const rsq_plan_desc& p, rsq_table* const* tables, int nTables, const std::vector<bool>& sharded,
                         int* gatheredTable) {
    const int n = (int)m.ctxs.size();
    auto tab = [&](int i, int t) { return reinterpret_cast<const Table*>(tables[(size_t)i * (size_t)nTables + (size_t)t]); };
    auto tableOf = [&](int scan) {
        const int t = p.ops[scan].table;
        if (t < 0 || t >= nTables) failInvalid("malformed plan: a scan names no table");
        return t;
    };
    std::vector<int> all;
    subtreeOps(p, p.root, all);
    // the top-level join: not inside another join's inner side (those belong to the inner query)
    std::vector<int> inInner;
    for (int o : all)
        if (p.ops[o].tag == RSQ_OP_NESTEDLOOPSJOIN) subtreeOps(p, p.ops[o].child[0], inInner);
    int nlj = -1;
    for (int o : all)
        if (p.ops[o].tag == RSQ_OP_NESTEDLOOPSJOIN && std::find(inInner.begin(), inInner.end(), o) == inInner.end()) {
            if (nlj >= 0) failUnsupported("across GPUs a plan holds one nested-loops join (and joins inside its inner side)");
            nlj = o;
        }
    // ... on the plan's last pipeline: its outer rows are split, so it must not fill a join table every shard needs whole
    bool onLast = false;
    for (int op = p.root, steps = 0; op >= 0 && op < p.n_ops && steps <= p.n_ops && p.ops[op].tag != RSQ_OP_SCAN; steps++, op = pipelineChild(p.ops[op]))
        if (op == nlj) onLast = true;
    if (!onLast) failUnsupported("a nested-loops join that feeds a join's build side is not split across GPUs");
    const int outerScan = pipelineScan(p, p.ops[nlj].child[1]);
    const int innerScan = pipelineScan(p, p.ops[nlj].child[0]);
    std::vector<int> inner;
    subtreeOps(p, p.ops[nlj].child[0], inner);
    std::vector<int> shardedInner;
    for (int o : all) {
        if (p.ops[o].tag != RSQ_OP_SCAN || o == outerScan || !sharded[(size_t)tableOf(o)]) continue;
        const std::string name = tab(0, tableOf(o))->name;
        if (std::find(inner.begin(), inner.end(), o) == inner.end())
            failUnsupported("table " + name + " is sharded (its shards differ) but is a build side of the nested-loops plan: across GPUs only the "
                            "nested-loops join's outer table and one table of its inner side may be sharded - replicate " + name);
        shardedInner.push_back(o);
    }
    if (shardedInner.size() > 1)
        failUnsupported("the inner side of the nested-loops join reads two sharded tables (" + tab(0, tableOf(shardedInner[0]))->name + ", " +
                        tab(0, tableOf(shardedInner[1]))->name + "): at most one may be sharded - replicate the others");
    if (!shardedInner.empty() && shardedInner[0] != innerScan)
        failUnsupported("table " + tab(0, tableOf(shardedInner[0]))->name + " is sharded but is not the source of the nested-loops join's inner side "
                        "(a build side, or under a nested inner side): replicate it");
    const int gathered = shardedInner.empty() ? -1 : shardedInner[0];
    if (gathered >= 0) {
        // the parts go together in shard order: that is the inner side's order only if the shards hold increasing row ranges
        const int t = tableOf(gathered);
        for (int op = p.ops[nlj].child[0]; op != gathered; op = pipelineChild(p.ops[op]))
            if (p.ops[op].tag == RSQ_OP_ORDERBY || p.ops[op].tag == RSQ_OP_AGGREGATION)
                failUnsupported("table " + tab(0, t)->name + " is sharded, and the nested-loops join's inner side over it is sorted or aggregated: replicate it");
        for (int i = 1; i < n; i++)
            if (tab(i, t)->row0 < tab(i - 1, t)->row0 + tab(i - 1, t)->nRows)
                failUnsupported("table " + tab(0, t)->name + " is the sharded inner side of a nested-loops join, and its shards must hold increasing row "
                                "ranges (shard " + std::to_string(i) + " starts at row " + std::to_string((long long)tab(i, t)->row0) + ", before the end of shard " +
                                std::to_string(i - 1) + "'s rows): set each shard's first row (rsq_table_set_first_row)");
        *gatheredTable = t;
    } else *gatheredTable = -1;
    return outerScan;
}

// rows [start, start + rows) of a table, as a table of its own: offset column pointers, the first row numbered over the whole table, the
// parent's statistics and row count (it plans as the whole table, like a shard), a fresh identity; the parent keeps the memory
std::unique_ptr<Table> sliceOf(const Table& t, int64_t start, int64_t rows) {
    std::unique_ptr<Table> v(new Table());
    v->ctx = t.ctx; v->name = t.name; v->nRows = rows; v->row0 = t.row0 + start; v->nRowsTotal = t.totalRows();
    v->cols = t.cols;
    for (TableColumn& c : v->cols) {
        c.owned = false;
        c.nw = 0; c.nbase = 0; c.nptr = nullptr; c.nbytes = 0;      // (a borrowed view reads the wide column)
        c.dictN = 0; c.dict.clear(); c.dictPtr = nullptr; c.codePtr = nullptr; c.codeBytes = 0;
        if (c.dptr) c.dptr = (char*)c.dptr + (size_t)start * (size_t)columnWidth(c.type);
    }
    return v;
}

// one execution of a nested-loops plan: every shard's inner part (shard threads), the pair budget of the whole statement, the
// all-gather of the parts (or each shard binds its own, replicated, inner side), then every shard's outer pipelines
void executeNestedLoops(rsq_multi_query& mq) {
    rsq_multi& m = *mq.m;
    NljSplit& sp = mq.split;
    const int n = (int)m.ctxs.size();
    std::vector<NljState*> nl((size_t)n);
    int64_t outer = 0;
    for (int i = 0; i < n; i++) { nl[(size_t)i] = &topNestedLoops(*mq.qs[(size_t)i]); outer += nl[(size_t)i]->outerSrc->nRows; }
    // (a shard whose outer slice is empty still makes its inner part for the others)
    std::vector<int64_t> rows((size_t)n, 0);
    onShardThreads(n, [&](int i) {
        RSQ_HIP(hipSetDevice(m.ctxs[(size_t)i]->device));
        runNestedLoopsInner(*nl[(size_t)i], outer > 0);
        rows[(size_t)i] = nl[(size_t)i]->nInner;
        sp.innerDone[(size_t)i].record(m.ctxs[(size_t)i]->stream);
    });
    int64_t inner = 0;
    for (int i = 0; i < n; i++) {
        if (!sp.gathered && rows[(size_t)i] != rows[0])
            throw Error(RSQ_ERR_RUNTIME, "internal: replicated inner sides of a nested-loops join differ between shards (" + std::to_string((long long)rows[0]) +
                                         " and " + std::to_string((long long)rows[(size_t)i]) + " rows)");
        inner = sp.gathered ? inner + rows[(size_t)i] : rows[0];
    }
    try {
        for (int i = 0; i < n; i++) { RSQ_HIP(hipSetDevice(m.ctxs[(size_t)i]->device)); bindNestedLoops(*mq.qs[(size_t)i], *nl[(size_t)i], outer, inner); }
    } catch (const Error&) {
        // refused before any outer pipeline: the report holds the inner sides' work
        mq.report = rsq_report{};
        for (int i = 0; i < n; i++) { mq.report.num_kernels += (int32_t)nl[(size_t)i]->sub.kernels; mq.report.bytes_read += nl[(size_t)i]->sub.bytes; }
        throw;
    }
    // the bound columns of shard j, column by column: the parts of all shards back to back (gathered, each shard's part behind its
    // innerDone, waited for in front of the first column), or its own inner side
    sp.gatherBytes = 0;
    for (int j = 0; j < n; j++) {
        Context& dst = *m.ctxs[(size_t)j];
        const NljState& to = *nl[(size_t)j];
        if (sp.gathered) sp.gather0[(size_t)j].record(dst.stream);
        for (size_t k = 0; k < to.innerSchema.size(); k++) {
            const size_t w = (size_t)columnWidth(to.innerSchema[k].type);
            std::vector<GatherPart> parts;
            for (int i = 0; i < n; i++)
                if ((sp.gathered || i == j) && rows[(size_t)i] > 0)
                    parts.push_back({m.ctxs[(size_t)i], nl[(size_t)i]->sub.query->dMatCols[(size_t)nl[(size_t)i]->innerCol[k]], (size_t)rows[(size_t)i] * w,
                                     k == 0 && i != j ? sp.innerDone[(size_t)i].get() : nullptr});
            if (!parts.empty()) sp.gatherBytes += gatherParts(dst, to.sub.dCols[k], parts);
        }
        if (sp.gathered) sp.gather1[(size_t)j].record(dst.stream);
    }
    if (sp.gathered) composeMergeText(mq);
    onShardThreads(n, [&](int i) { executeQuery(*mq.qs[(size_t)i], mq.dense); });
}

// device time of the last gather: the slowest shard's copies (0 without a gather)
double gatherMs(const rsq_multi_query& mq) {
    double ms = 0;
    for (size_t i = 0; mq.split.gathered && i < mq.split.gather0.size(); i++) ms = std::max(ms, mq.split.gather1[i].msSince(mq.split.gather0[i]));
    return ms;
}

}  // namespace

extern "C" {

int rsq_multi_create(const rsq_multi_config* hostCfg, rsq_multi** out) {
    if (!out || !hostCfg) return RSQ_ERR_INVALID;
    *out = nullptr;
    return guardedM(nullptr, [&] {
        // the host's struct, struct_size bytes of it (every later field reads as 0), like rsq_config (api.cpp readConfig)
        rsq_multi_config mc{};
        const uint32_t have = hostCfg->struct_size;
        if (have < offsetof(rsq_multi_config, merge) || have > 4096)
            failInvalid("rsq_multi_config.struct_size is " + std::to_string(have) + ": set it to sizeof(rsq_multi_config) (" + std::to_string(sizeof(rsq_multi_config)) + " in this library)");
        memcpy(&mc, hostCfg, std::min<size_t>(have, sizeof mc));
        const rsq_multi_config* cfg = &mc;
        if (cfg->n_devices < 1 || !cfg->devices) failInvalid("rsq_multi_create needs at least one device");
        std::unique_ptr<rsq_multi> m(new rsq_multi());
        std::set<int> distinct;
        for (int i = 0; i < cfg->n_devices; i++) {
            if (cfg->devices[i] < 0) failInvalid("rsq_multi_create needs device ordinals (a compile-only context has no shards to run)");
            m->devices.push_back(cfg->devices[i]);
            distinct.insert(cfg->devices[i]);
        }
        m->sharedDevice = (int)distinct.size() != cfg->n_devices;
        m->merge = cfg->merge == RSQ_MERGE_AUTO ? (m->sharedDevice ? RSQ_MERGE_PEER_COPY : RSQ_MERGE_RCCL) : cfg->merge;
        if (m->merge != RSQ_MERGE_RCCL && m->merge != RSQ_MERGE_PEER_COPY) failInvalid("unknown merge mode");
        if (m->merge == RSQ_MERGE_RCCL && m->sharedDevice)
            failInvalid("an RCCL communicator cannot hold the same device twice: use RSQ_MERGE_PEER_COPY for shards that share a GPU");
        for (int i = 0; i < cfg->n_devices; i++) {
            rsq_config c = readConfig(cfg->base, true);
            c.device = cfg->devices[i];
            m->ctxs.push_back(new Context(c));
        }
        if (m->merge == RSQ_MERGE_PEER_COPY && !m->sharedDevice) enablePeerAccess(m->devices, true);      // (the root gathers the partial tables)
        if (m->merge == RSQ_MERGE_RCCL && (cfg->n_devices > 1 || cfg->merge == RSQ_MERGE_RCCL)) {
            m->comms.assign((size_t)cfg->n_devices, nullptr);
            RSQ_NCCL(rccl().CommInitAll(m->comms.data(), cfg->n_devices, m->devices.data()));
        }
        *out = m.release();
    });
}

void rsq_multi_destroy(rsq_multi* m) { delete m; }

const char* rsq_multi_last_error(const rsq_multi* m) { return m ? m->lastError.c_str() : g_multiCreateError.c_str(); }

int32_t rsq_multi_devices(const rsq_multi* m) { return m ? (int32_t)m->ctxs.size() : 0; }

rsq_ctx* rsq_multi_ctx(rsq_multi* m, int32_t shard) {
    if (!m || shard < 0 || shard >= (int32_t)m->ctxs.size()) return nullptr;
    return reinterpret_cast<rsq_ctx*>(m->ctxs[(size_t)shard]);
}

const char* rsq_multi_merge_name(const rsq_multi* m) {
    if (!m) return "";
    if (m->ctxs.size() == 1) return "single GPU (no exchange)";
    return m->merge == RSQ_MERGE_RCCL ? "RCCL reduce to the root GPU, one grouped launch (min | max | sum segments)"
                                      : "peer copies to the root GPU + merge kernel";
}

void rsq_multi_shard_rows(int64_t n_total, int32_t n_shards, int32_t shard, int64_t* row0, int64_t* n_rows) {
    // equal shards on 128-row tile boundaries (the scan's vector loads want 16-byte aligned column offsets); the last
    // shard takes the remainder — resql_amd/dist.py shard_rows, same numbers
    const int64_t tile = 128;
    const int64_t per = n_shards > 0 ? (n_total / (tile * n_shards)) * tile : 0;
    if (row0) *row0 = (int64_t)shard * per;
    if (n_rows) *n_rows = shard < n_shards - 1 ? per : n_total - per * (n_shards - 1);
}

int rsq_multi_table_generate(rsq_multi* m, int32_t kind, int64_t n_rows_total, double scale_factor, int64_t param, uint64_t seed,
                             rsq_table** out_tables) {
    if (!m || !out_tables || n_rows_total < 0) return RSQ_ERR_INVALID;
    const int n = (int)m->ctxs.size();
    for (int i = 0; i < n; i++) out_tables[i] = nullptr;
    return guardedM(m, [&] {
        for (int i = 0; i < n; i++) {
            int64_t r0, nr;
            rsq_multi_shard_rows(n_rows_total, n, i, &r0, &nr);
            std::unique_ptr<Table> t(new Table());
            generateTable(*m->ctxs[(size_t)i], *t, kind, r0, nr, scale_factor, param, seed);
            out_tables[i] = reinterpret_cast<rsq_table*>(t.release());
        }
    });
}

// Row-range shards whose boundaries fall where `key_column` changes: no value of the clustering key spans two shards, so a
// plan grouped by it (TPC-H Q3: l_orderkey) keeps every group on one GPU.  Every tile boundary of
// rsq_multi_shard_rows is moved forward to the first row whose key differs from the row before it; the rows around a boundary
// are generated (the generator is a function of seed and row number) on the root GPU and read back, a window at a time.
int rsq_multi_table_generate_on_key(rsq_multi* m, int32_t kind, int64_t n_rows_total, double scale_factor, int64_t param, uint64_t seed,
                                    const char* key_column, rsq_table** out_tables) {
    if (!m || !out_tables || n_rows_total < 0 || !key_column) return RSQ_ERR_INVALID;
    const int n = (int)m->ctxs.size();
    for (int i = 0; i < n; i++) out_tables[i] = nullptr;
    return guardedM(m, [&] {
        Context& root = *m->ctxs[0];
        auto snap = [&](int64_t b) -> int64_t {
            if (b <= 0 || b >= n_rows_total) return std::max<int64_t>(0, std::min(b, n_rows_total));
            const int64_t window = 4096;
            int64_t prevKey = 0; bool havePrev = false;
            for (int64_t at = b - 1; at < n_rows_total; at += window) {
                const int64_t cnt = std::min(window, n_rows_total - at);
                Table t;
                generateTable(root, t, kind, at, cnt, scale_factor, param, seed);
                const int c = t.findCol(key_column);
                if (c < 0 || !t.cols[(size_t)c].dptr) failInvalid(std::string("table has no generated column ") + key_column);
                const Type& ty = t.cols[(size_t)c].type;
                if (ty.isString() || (columnWidth(ty) != 4 && columnWidth(ty) != 8)) failUnsupported("the shard key must be an INT / DATE / BIGINT / DECIMAL column");
                std::vector<int64_t> keys((size_t)cnt);
                if (columnWidth(ty) == 4) {
                    std::vector<int32_t> k4((size_t)cnt);
                    RSQ_HIP(hipMemcpy(k4.data(), t.cols[(size_t)c].dptr, (size_t)cnt * 4, hipMemcpyDeviceToHost));
                    for (int64_t j = 0; j < cnt; j++) keys[(size_t)j] = k4[(size_t)j];
                } else RSQ_HIP(hipMemcpy(keys.data(), t.cols[(size_t)c].dptr, (size_t)cnt * 8, hipMemcpyDeviceToHost));
                for (int64_t j = 0; j < cnt; j++) {
                    if (havePrev && keys[(size_t)j] != prevKey) return at + j;
                    prevKey = keys[(size_t)j]; havePrev = true;
                }
            }
            return n_rows_total;
        };
        std::vector<int64_t> bound((size_t)n + 1, n_rows_total);
        bound[0] = 0;
        for (int i = 1; i < n; i++) {
            int64_t r0, nr;
            rsq_multi_shard_rows(n_rows_total, n, i, &r0, &nr);
            bound[(size_t)i] = std::max(bound[(size_t)i - 1], snap(r0));
        }
        for (int i = 0; i < n; i++) {
            std::unique_ptr<Table> t(new Table());
            generateTable(*m->ctxs[(size_t)i], *t, kind, bound[(size_t)i], bound[(size_t)i + 1] - bound[(size_t)i], scale_factor, param, seed);
            out_tables[i] = reinterpret_cast<rsq_table*>(t.release());
        }
    });
}

int rsq_multi_query_compile(rsq_multi* m, const rsq_plan_desc* plan, rsq_table* const* tables, int32_t n_tables, rsq_multi_query** out) {
    if (!m || !plan || !out || n_tables < 0 || (n_tables > 0 && !tables)) return RSQ_ERR_INVALID;
    *out = nullptr;
    return guardedM(m, [&] {
        const int n = (int)m->ctxs.size();
        std::unique_ptr<rsq_multi_query> mq(new rsq_multi_query());
        mq->m = m;
        for (int i = 0; i < plan->n_ops; i++)
            if (plan->ops && plan->ops[i].tag == RSQ_OP_NESTEDLOOPSJOIN) {
                if (!(m->ctxs[0]->cfg.engine_flags & RSQ_ENGINE_NESTED_LOOPS))
                    failUnsupported("a nested-loops join is not executed across GPUs (rsq_multi_*): run it on one context");
                mq->nlj = true;
            }
        std::vector<bool> sharded((size_t)n_tables, false);     // the table's instances differ between the shards
        for (int i = 0; i < n; i++)
            for (int t = 0; t < n_tables; t++) {
                const Table* tb = reinterpret_cast<const Table*>(tables[(size_t)i * (size_t)n_tables + (size_t)t]);
                if (!tb) failInvalid("null table");
                if (tb->ctx != m->ctxs[(size_t)i]) failInvalid("table " + tb->name + " of shard " + std::to_string(i) + " does not live on that shard's context");
            }
        // The reference has ONE relation and ONE hash table all workers reach (aggregation.h:240-295, JitContextFlounder.h:459-487): any
        // data works.  Here every shard plans from column statistics, so the shards of a table first receive the statistics of the WHOLE
        // table (union of the byte-value sets, min / max over the shards, summed row count): all of them then derive the same dense
        // group layout whatever their own rows hold, or all of them the hash aggregation where the union is not dense.  A table whose
        // instances are the same rows on every shard (a replicated build side: equal row range and statistics) is left as it is.
        // (two passes: every table's blobs are made and checked first, and only then is any table changed - a schema that differs on one
        // shard must not leave some tables unified and others not)
        if (n > 1) {
            auto tab = [&](int i, int t) { return reinterpret_cast<Table*>(tables[(size_t)i * (size_t)n_tables + (size_t)t]); };
            std::vector<std::vector<char>> allBlobs((size_t)n_tables);
            std::vector<size_t> blobBytes((size_t)n_tables, 0);
            for (int t = 0; t < n_tables; t++) {
                const size_t bb = tableStatsBytes(*tab(0, t));
                std::vector<char>& blobs = allBlobs[(size_t)t];
                blobs.resize((size_t)n * bb);
                bool replicated = true;
                for (int i = 0; i < n; i++) {
                    if (tableStatsBytes(*tab(i, t)) != bb) failInvalid("table " + tab(i, t)->name + " has another schema on shard " + std::to_string(i));
                    exportTableStats(*tab(i, t), blobs.data() + (size_t)i * bb, bb);
                    if (memcmp(blobs.data(), blobs.data() + (size_t)i * bb, bb) != 0) replicated = false;
                }
                blobBytes[(size_t)t] = replicated ? 0 : bb;
                sharded[(size_t)t] = !replicated;
            }
            for (int t = 0; t < n_tables; t++)
                if (blobBytes[(size_t)t])
                    for (int i = 0; i < n; i++) unifyShardStats(*tab(i, t), allBlobs[(size_t)t].data(), n, blobBytes[(size_t)t]);
            // ... and with RSQ_ENGINE_DICT_MULTI one dictionary per coded column (engine.h unifyShardDictionaries): the shards of a table receive
            // the union of their dictionaries, the copies of a replicated table are compared.  Nothing moves where the shards hold it already.
            if ((m->ctxs[0]->cfg.engine_flags & RSQ_ENGINE_DICT_MULTI) && sw::dictScansEnabled())
                for (int t = 0; t < n_tables; t++) {
                    std::vector<Table*> inst;
                    for (int i = 0; i < n; i++) inst.push_back(tab(i, t));
                    unifyShardDictionaries(inst, !sharded[(size_t)t]);
                }
        }
        // (more than one shard: every compile below keeps string group keys on the hash form - Context::shardCompile)
        struct ShardCompile {
            rsq_multi* m; bool on;
            ShardCompile(rsq_multi* m_, bool on_) : m(m_), on(on_) { for (Context* c : m->ctxs) c->shardCompile = on; }
            ~ShardCompile() { for (Context* c : m->ctxs) c->shardCompile = false; }
        } shardCompile(m, n > 1);
        if (!mq->nlj) {
            for (int i = 0; i < n; i++) mq->qs.push_back(compileQuery(*m->ctxs[(size_t)i], *plan, tables + (size_t)i * (size_t)n_tables, n_tables));
        } else {
            int gatheredTable = -1;
            const int outerScan = planNestedLoopsSplit(*m, *plan, tables, n_tables, sharded, &gatheredTable);
            const int outerTable = plan->ops[outerScan].table;
            // a replicated outer table: the outer scan reads shard i's slice of it, a table appended to the shard's array
            const bool sliced = n > 1 && !sharded[(size_t)outerTable];
            std::vector<rsq_op> ops(plan->ops, plan->ops + plan->n_ops);
            rsq_plan_desc p = *plan;
            if (sliced) { ops[(size_t)outerScan].table = n_tables; p.ops = ops.data(); }
            const int nt = n_tables + (sliced ? 1 : 0);
            for (int i = 0; i < n; i++) {
                std::vector<rsq_table*> ts(tables + (size_t)i * (size_t)n_tables, tables + (size_t)(i + 1) * (size_t)n_tables);
                const Table* outer = reinterpret_cast<const Table*>(ts[(size_t)outerTable]);
                if (sliced) {
                    int64_t r0, nr;
                    rsq_multi_shard_rows(outer->nRows, n, i, &r0, &nr);
                    mq->split.outerSlices.push_back(sliceOf(*outer, r0, nr));
                    outer = mq->split.outerSlices.back().get();
                    ts.push_back(reinterpret_cast<rsq_table*>(mq->split.outerSlices.back().get()));
                }
                Query* q = compileQuery(*m->ctxs[(size_t)i], p, ts.data(), nt);
                mq->qs.push_back(q);
                NljState& top = topNestedLoops(*q);
                if (top.outerSrc != outer)
                    throw Error(RSQ_ERR_RUNTIME, "internal: the nested-loops join's outer pipeline does not scan table " + outer->name);
                // (executeQuery runs the outer side only; the gathered table is seen whole by every shard: it never proves shards disjoint in a group key)
                top.sub.external = true;
                if (gatheredTable >= 0) q->gatheredTables.push_back(reinterpret_cast<const Table*>(ts[(size_t)gatheredTable]));
                const Context& c = *m->ctxs[(size_t)i];
                mq->split.innerDone.emplace_back(c, false); mq->split.gather0.emplace_back(c, true); mq->split.gather1.emplace_back(c, true);
            }
            mq->split.gathered = gatheredTable >= 0;
            if (mq->split.gathered) enablePeerAccess(m->devices, false);
        }
        // derived aggregations: across the shards with RSQ_ENGINE_DERIVED_MULTI (never inside a nested-loops plan), else on one context only
        if (!mq->qs.empty() && queryHasDerived(*mq->qs[0])) {
            if (!(m->ctxs[0]->cfg.engine_flags & RSQ_ENGINE_DERIVED_MULTI) || mq->nlj) refuseDerived(*mq->qs[0], "a multi-GPU compile (rsq_multi_query_compile)");
            mq->derived = true;
            mq->derivedText = planDerivedAcrossShards(mq->qs, tables, n_tables, sharded);
            enablePeerAccess(m->devices, false);
        }
        mq->dense = queryIsDense(*mq->qs[0]);
        if (mq->dense) {
            // (with unified statistics every shard derives the same layout; anything else is a defect of this library, not of the data)
            const std::string l0 = queryPartialLayoutText(*mq->qs[0]);
            for (int i = 1; i < n; i++)
                if (!queryIsDense(*mq->qs[(size_t)i]) || queryPartialLayoutText(*mq->qs[(size_t)i]) != l0)
                    throw Error(RSQ_ERR_RUNTIME, "internal: shards planned from the same statistics disagree on the partial aggregate table layout: shard 0 has \"" + l0 +
                                                 "\", shard " + std::to_string(i) + " has \"" + queryPartialLayoutText(*mq->qs[(size_t)i]) + "\"");
            Context& root = *m->ctxs[0];
            if (n > 1 && m->merge == RSQ_MERGE_PEER_COPY) {
                int64_t nMin, nMax, nSum; void* p;
                queryDenseLayout(*mq->qs[0], &nMin, &nMax, &nSum, &p);
                mq->gathered = (int64_t*)root.alloc((size_t)n * (size_t)(nMin + nMax + nSum) * 8);
                mq->ready.emplace_back();
                for (int i = 1; i < n; i++) mq->ready.emplace_back(*m->ctxs[(size_t)i], false);
            }
            if (n > 1 || !m->comms.empty()) { mq->evMerge0 = ShardEvent(root, true); mq->evMerge1 = ShardEvent(root, true); }      // (enqueueMerge)
            // (a nested-loops plan runs on host threads: the host stands between its inner and its outer sides)
            mq->async = !mq->nlj && !mq->derived;
            for (Query* q : mq->qs) mq->async = mq->async && queryAsyncCapable(*q);
            mq->mergeBase = std::string("dense partial tables: ") + rsq_multi_merge_name(m) +
                            (mq->async ? "" : mq->nlj ? " (nested-loops join: the shards run on host threads)" : mq->derived ? " (derived tables: the shards run on host threads)"
                                                                                                                  : " (join builds: the shards run on host threads)");
        } else {
            for (int i = 1; i < n; i++) if (queryIsDense(*mq->qs[(size_t)i])) throw Error(RSQ_ERR_RUNTIME, "internal: shards planned from the same statistics disagree on the aggregation strategy");
            // Groups may straddle shard boundaries (the reference has ONE hash table all workers reach, aggregation.h:240-295):
            // the general merge reads every shard's group rows back and re-aggregates them by key before the root's tail runs.
            // Only when the column statistics PROVE that no group lives in two shards (the caller sharded on a boundary of a
            // group key) and the plan ends in ORDER BY ... LIMIT k is the short way taken: every shard's own top k, merged by the
            // sort keys.  RSQ_MULTI_GENERAL_MERGE=1 forces the general merge (tests).
            std::string why;
            const bool disjoint = n > 1 && shardGroupsDisjoint(mq->qs, why);
            const bool forceGeneral = sw::flag<sw::RSQ_MULTI_GENERAL_MERGE>();
            mq->orderedFast = disjoint && queryOrderedWithLimit(*mq->qs[0]) && !forceGeneral;
            if (n == 1) mq->mergeBase = "single shard";
            else if (mq->orderedFast) mq->mergeBase = "ordered merge of the shards' LIMIT-ed rows (" + why + ")";
            else mq->mergeBase = "general merge: all shards' group rows re-aggregated by key on the host, then one tail (" +
                                 (forceGeneral ? std::string("forced") : disjoint ? std::string("no ORDER BY ... LIMIT to shorten") : why) + ")";
            if (n > 1 && !mq->orderedFast) for (Query* q : mq->qs) setHoldTail(*q, true);
        }
        composeMergeText(*mq);
        mq->shardKernelMs.assign((size_t)n, 0.0);
        *out = mq.release();
    });
}

int rsq_multi_query_execute(rsq_multi_query* mq) {
    if (!mq) return RSQ_ERR_INVALID;
    rsq_multi* m = mq->m;
    return guardedM(m, [&] {
        const int n = (int)m->ctxs.size();
        const double t0 = nowMs();
        // 1. the shards, up to their partial tables (dense) or their own results
        mq->derivedMs = 0;
        if (mq->derived) {
            // the derived tables on every shard, innermost first (their sub-queries, exchanges and writers), then the parent as below
            DerivedMultiRun run;
            runDerivedAcrossShards(mq->qs, run);
            mq->derivedMs = run.exchangeMs;
            mq->derivedText = run.text;
            composeMergeText(*mq);
        }
        if (mq->nlj) executeNestedLoops(*mq);      // inner parts, the budget, the gather, the outer sides
        else if (mq->dense && mq->async)
            // fan out: enqueue every shard's pipelines (no host synchronisation); the merge goes behind them, then ONE synchronising
            // read-back on the root
            for (int i = 0; i < n; i++) executeQuery(*mq->qs[(size_t)i], true, true);
        else
            // on host threads: join builds in front of a dense aggregation (TPC-H Q14-like) need the host's help, as does any other plan
            onShardThreads(n, [&](int i) { executeQuery(*mq->qs[(size_t)i], mq->dense); });
        // 2. the merge of the plan's kind
        if (mq->dense) {
            enqueueMerge(*mq);
            finalizeQuery(*mq->qs[0]);
            if (mq->async) for (int i = 1; i < n; i++) settleAsync(*mq->qs[(size_t)i]);
        } else {
            const double t1 = nowMs();
            if (n > 1) { if (mq->orderedFast) mergeShardResults(*mq->qs[0], mq->qs); else runTailMerged(*mq->qs[0], mq->qs); }
            mq->report.finalize_time_ms = nowMs() - t1;
        }
        // 3. the report: the slowest shard's kernel time (the shards run concurrently), bytes of all shards
        rsq_report r0; queryReport(*mq->qs[0], &r0);
        rsq_report rep = r0;
        rep.bytes_read = 0; rep.num_kernels = 0; rep.kernel_time_ms = 0;
        for (int i = 0; i < n; i++) {
            rsq_report r; queryReport(*mq->qs[(size_t)i], &r);
            rep.bytes_read += r.bytes_read; rep.num_kernels += r.num_kernels;
            rep.kernel_time_ms = std::max(rep.kernel_time_ms, r.kernel_time_ms);
            rep.compilation_time_ms = std::max(rep.compilation_time_ms, r.compilation_time_ms);
            mq->shardKernelMs[(size_t)i] = r.kernel_time_ms;
        }
        if (!mq->dense && n > 1) rep.finalize_time_ms = r0.finalize_time_ms + mq->report.finalize_time_ms;
        mq->collectiveMs = (mq->dense ? mq->evMerge1.msSince(mq->evMerge0) : 0) + (mq->nlj ? gatherMs(*mq) : 0) + mq->derivedMs;
        rep.execution_time_ms = nowMs() - t0;
        rep.hbm_gbps = rep.kernel_time_ms > 0 ? (double)rep.bytes_read / (rep.kernel_time_ms * 1e-3) / 1e9 : 0;
        mq->report = rep;
    });
}

int rsq_multi_query_result(rsq_multi_query* mq, rsq_result_view* out) {
    if (!mq || !out) return RSQ_ERR_INVALID;
    return guardedM(mq->m, [&] { queryResult(*mq->qs[0], out); });
}

int rsq_multi_query_report(const rsq_multi_query* mq, rsq_report* out, double* shard_kernel_ms) {
    if (!mq || !out) return RSQ_ERR_INVALID;
    *out = mq->report;
    if (shard_kernel_ms) for (size_t i = 0; i < mq->shardKernelMs.size(); i++) shard_kernel_ms[i] = mq->shardKernelMs[i];
    return RSQ_OK;
}

double rsq_multi_query_collective_ms(const rsq_multi_query* mq) { return mq ? mq->collectiveMs : 0; }

const char* rsq_multi_query_merge_name(const rsq_multi_query* mq) { return mq ? mq->mergeText.c_str() : ""; }

const char* rsq_multi_query_explain(const rsq_multi_query* mq, int32_t shard) {
    if (!mq || shard < 0 || shard >= (int32_t)mq->qs.size()) return nullptr;
    return queryExplain(*mq->qs[(size_t)shard]);
}

void rsq_multi_query_destroy(rsq_multi_query* mq) { delete mq; }

}  // extern "C"
