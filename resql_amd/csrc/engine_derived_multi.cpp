// engine_derived_multi.cpp - derived aggregations across GPUs (rsq_multi_* with RSQ_ENGINE_DERIVED_MULTI; multi.cpp drives it).
//
// Every shard compiles the whole plan, so every shard has its own sub-query per derived table (engine.cpp compileDerived).  Each
// derived table is split by the tables its sub-query reads ("sharded": a table whose instances differ between the shards):
//   local   every table is replicated (a derived table below counts as replicated): each shard computes the whole table itself;
//   merged  exactly one table is sharded, and it is the source of the sub-query's aggregating pipeline: each shard runs its sub-query up
//           to its group rows (tail held back), and the groups are merged across shards into the table one context gives over the whole
//           tables - the reference has ONE hash table all workers reach (aggregation.h:240-343, JitContextFlounder.h:459-487);
//   anything else is refused, naming the table.
// Merged, hash / join-entry groups: on the DEVICE path (where one context's sub-query would take its device tail) the shards' group rows
// are gathered to the root in shard order (shard_exchange.h gatherParts), merged by key in one device hash table (devtail.hip k_gm_*),
// and go through the device tail's emission order; the root writes its columns and copies them (or each shard's slice) to the other
// shards.  On the HOST path the root merges them with runTailMerged and every shard uploads the tuples and writes its own columns.  A
// dense sub-query merges its partial tables on the root (shard_exchange.h mergeDenseOnRoot) and finalises there; its tuples then travel
// the same two ways.  The events between the shards' streams and the shards' host threads are that layer's too.
// Where the table lands: the source of the plan's last pipeline is scanned slice by slice (rsq_multi_shard_rows of its rows, the slice's
// first row numbered over the whole table, bound at launch); any other place (a build side, an earlier pipeline's source) holds it whole.
#include <algorithm>
#include <cstring>
#include <map>

#include "engine_internal.h"
#include "shard_exchange.h"

namespace rsq {

namespace {

enum { LOCAL = 1, MERGED = 2 };

void scansOf(OpNode* o, std::vector<OpNode*>& out) {
    if (!o) return;
    if (o->tag == RSQ_OP_SCAN) { out.push_back(o); return; }
    for (int k = 0; k < 2; k++) scansOf(o->child[k], out);
}

const Table* aggregatingSource(const Query& s) {
    for (const Pipeline& p : s.pipelines) if (p.sink == SinkKind::AGGREGATE) return p.src;
    return nullptr;
}

struct Planner {
    std::map<const Table*, int> index;      // shard 0's tables -> position in the caller's array
    const std::vector<bool>* sharded = nullptr;
    bool isSharded(const Table* t) const {
        if (t->derived) return false;       // (local or merged: the same rows on every shard)
        auto it = index.find(t);
        return it != index.end() && (*sharded)[(size_t)it->second];
    }

    // the derived tables of `qs` (one query per shard), innermost first
    void classify(const std::vector<Query*>& qs, const std::string& prefix, std::string& text) {
        for (size_t k = 0; k < qs[0]->derived.size(); k++) {
            std::vector<Query*> subs;
            for (Query* q : qs) { subs.push_back(q->derived[k].sub.query.get()); q->derived[k].sub.external = true; }
            DerivedState& d0 = qs[0]->derived[k];
            const std::string name = prefix + d0.table->name;
            classify(subs, name + "/", text);
            Query& s = *d0.sub.query;
            std::vector<OpNode*> scans;
            scansOf(s.root, scans);
            std::vector<const Table*> shardedScans;
            for (OpNode* o : scans) if (isSharded(o->table)) shardedScans.push_back(o->table);
            int mode = LOCAL;
            if (shardedScans.size() > 1)
                failUnsupported("the derived aggregation " + name + " reads two sharded tables (" + shardedScans[0]->name + ", " + shardedScans[1]->name +
                                "): across GPUs at most one table of a derived aggregation may be sharded - replicate " + shardedScans[1]->name);
            if (!shardedScans.empty()) {
                const Table* t = shardedScans[0];
                if (aggregatingSource(s) != t)
                    failUnsupported("table " + t->name + " is sharded but is not the source of the aggregating pipeline of the derived aggregation " + name +
                                    " (a build side): across GPUs replicate " + t->name);
                if (queryIsDense(s) && !s.derived.empty())
                    failUnsupported("table " + t->name + " is sharded under the derived aggregation " + name + ", whose dense groups also read a derived table: replicate " + t->name);
                mode = MERGED;
            }
            for (Query* q : qs) { q->derived[k].multi = mode; q->derived[k].sliceShards = 0; q->derived[k].sliceAt = 0; }
            if (mode == MERGED) text += (text.empty() ? "" : "; ") + name + " merged over " + std::to_string(qs.size()) + " shards";
        }
    }
};

// the columns of shard j's table d are shard 0's (rows [r0, r0 + rows)), by peer copies behind `ready` on the root's stream
void copyColumns(Context& root, DerivedState& from, Context& dst, DerivedState& to, int64_t r0, int64_t rows, hipEvent_t ready, int64_t* moved) {
    Table& t = *to.table;
    const int64_t n = from.table->nRows;
    to.sub.ensureColumns(dst, t.cols, std::max<int64_t>(n, 1), std::max<int64_t>(n + n / 8, 64));      // (engine.cpp writeDerivedFrom's rule)
    RSQ_HIP(hipSetDevice(dst.device));
    RSQ_HIP(hipStreamWaitEvent(dst.stream, ready, 0));
    for (size_t c = 0; c < t.cols.size(); c++) {
        const size_t w = (size_t)columnWidth(t.cols[c].type);
        t.cols[c].dptr = to.sub.dCols[c];
        if (rows <= 0) continue;
        copyDeviceAsync((char*)to.sub.dCols[c] + (size_t)r0 * w, dst.device, (const char*)from.sub.dCols[c] + (size_t)r0 * w, root.device, (size_t)rows * w, dst.stream);
        *moved += (int64_t)((size_t)rows * w);
    }
    t.nRows = n; t.row0 = 0; t.nRowsTotal = -1;
}

// shard i scans its slice of the whole table: offset columns, its first row numbered over the whole table, the whole table's row count
void applySlice(DerivedState& d) {
    if (d.sliceShards <= 0) return;
    Table& t = *d.table;
    const int64_t n = t.nRows;
    int64_t r0 = 0, rows = 0;
    rsq_multi_shard_rows(n, d.sliceShards, d.sliceAt, &r0, &rows);
    for (size_t c = 0; c < t.cols.size(); c++) t.cols[c].dptr = (char*)d.sub.dCols[c] + (size_t)r0 * (size_t)columnWidth(t.cols[c].type);
    t.row0 = r0; t.nRows = rows; t.nRowsTotal = n;
}

void* mergeBuffer(Context& root, DerivedState& d, size_t bytes) {
    if ((int64_t)bytes > d.mergeCapacity || !d.dMerge) {
        if (d.dMerge) root.free(d.dMerge);
        d.dMerge = nullptr; d.mergeCapacity = 0;
        d.dMerge = root.alloc(bytes + bytes / 8);
        d.mergeCapacity = (int64_t)(bytes + bytes / 8);
    }
    return d.dMerge;
}

struct Runner {
    DerivedMultiRun* out = nullptr;

    void run(const std::vector<Query*>& qs, const std::string& prefix) {
        const int n = (int)qs.size();
        for (size_t k = 0; k < qs[0]->derived.size(); k++) {
            std::vector<Query*> subs;
            for (Query* q : qs) subs.push_back(q->derived[k].sub.query.get());
            run(subs, prefix + qs[0]->derived[k].table->name + "/");      // (the tables below it first)
            const std::string name = prefix + qs[0]->derived[k].table->name;
            if (qs[0]->derived[k].multi != LOCAL && n > 1) { merged(qs, k, name); continue; }
            onShardThreads(n, [&](int i) {
                Query& q = *qs[(size_t)i];
                buildDerived(q, q.derived[k]);
                applySlice(q.derived[k]);
            });
            traceLine("[rsq trace] %s: %lld rows, local on %d shards\n", name.c_str(), (long long)qs[0]->derived[k].table->totalRows(), n);
            describe(name, "local", qs[0]->derived[k], -1);
        }
    }

    void describe(const std::string& name, const std::string& how, const DerivedState& d, int64_t bytes) {
        out->text += (out->text.empty() ? "" : "; ") + name + " " + how + (bytes >= 0 ? " (" + std::to_string((long long)bytes) + " bytes)" : "") +
                     (d.sliceShards > 0 ? ", sliced" : ", whole");
    }

    void merged(const std::vector<Query*>& qs, size_t k, const std::string& name) {
        const int n = (int)qs.size();
        Query& q0 = *qs[0];
        DerivedState& d0 = q0.derived[k];
        Query& s0 = *d0.sub.query;
        Context& root = q0.ctx;
        const bool dense = queryIsDense(s0);
        // every shard's sub-query up to its group rows (hash) or its partial table (dense)
        std::vector<ShardEvent> done((size_t)n);
        onShardThreads(n, [&](int i) {
            SubQuery& sub = qs[(size_t)i]->derived[k].sub;
            Query& s = *sub.query;
            RSQ_HIP(hipSetDevice(s.ctx.device));
            if (!dense) { setHoldTail(s, true); s.holdTailOnDevice = true; }
            runSubQuery(sub, dense);
            done[(size_t)i] = ShardEvent(s.ctx, false);
            done[(size_t)i].record(s.ctx.stream);
        });
        const double t0 = nowMs();
        int64_t moved = 0;
        const std::string path = dense ? exchangeDense(qs, k, done, moved) : exchangeRows(qs, k, done, moved);
        // the root's columns, then every other shard's: copies of the root's (tuples on the root's device) or its own writer over the uploaded tuples
        const bool devTuples = s0.resultInPinned && s0.resultDev != nullptr;
        RSQ_HIP(hipSetDevice(root.device));
        writeDerivedFrom(q0, d0, s0, true);
        ShardEvent written(root, false);
        written.record(root.stream);
        const int64_t rows = d0.table->nRows;
        for (int j = 1; j < n; j++) {
            Query& q = *qs[(size_t)j];
            DerivedState& d = q.derived[k];
            if (devTuples) {
                int64_t r0 = 0, nr = rows;
                if (d.sliceShards > 0) rsq_multi_shard_rows(rows, d.sliceShards, d.sliceAt, &r0, &nr);
                copyColumns(root, d0, q.ctx, d, r0, nr, written.get(), &moved);
            } else {
                RSQ_HIP(hipSetDevice(q.ctx.device));
                writeDerivedFrom(q, d, s0, false);
            }
        }
        for (int i = 0; i < n; i++) applySlice(qs[(size_t)i]->derived[k]);
        for (int i = 0; i < n; i++) { RSQ_HIP(hipSetDevice(qs[(size_t)i]->ctx.device)); RSQ_HIP(hipStreamSynchronize(qs[(size_t)i]->ctx.stream)); }
        const double ms = nowMs() - t0;
        out->exchangeMs += ms;
        out->exchangeBytes += moved;
        traceLine("[rsq trace] %s: %lld rows merged %s over %d shards (%lld bytes moved, %.3f ms)\n", name.c_str(), (long long)rows, path.c_str(), n, (long long)moved, ms);
        describe(name, "merged " + path + " over " + std::to_string(n) + " shards", d0, moved);
    }

    // the shared dense merge on the root (gather buffer: mergeBuffer), then the root's tail
    std::string exchangeDense(const std::vector<Query*>& qs, size_t k, const std::vector<ShardEvent>& done, int64_t& moved) {
        std::vector<Query*> subs;
        for (Query* q : qs) subs.push_back(q->derived[k].sub.query.get());
        Query& s0 = *subs[0];
        int64_t nMin, nMax, nSum; void* p0;
        queryDenseLayout(s0, &nMin, &nMax, &nSum, &p0);
        int64_t* gathered = (int64_t*)mergeBuffer(s0.ctx, qs[0]->derived[k], qs.size() * (size_t)(nMin + nMax + nSum) * 8);
        moved += mergeDenseOnRoot(subs, done, gathered, "internal: shards disagree on the partial table of a derived aggregation");
        const uint64_t before = s0.report.num_kernels;
        finalizeQuery(s0);
        qs[0]->derived[k].sub.kernels += 1 + (s0.report.num_kernels >= before ? s0.report.num_kernels - before : 0);      // (the merge and the tail's launches)
        return s0.resultInPinned && s0.resultDev ? "on the device (dense partial tables)" : "on the host (dense partial tables, merge kernel on the device)";
    }

    // group rows: gathered and merged on the root's device (device path), or merged by the host (host path)
    std::string exchangeRows(const std::vector<Query*>& qs, size_t k, const std::vector<ShardEvent>& done, int64_t& moved) {
        const int n = (int)qs.size();
        DerivedState& d0 = qs[0]->derived[k];
        Query& s0 = *d0.sub.query;
        Context& root = s0.ctx;
        std::vector<Query*> subs;
        int64_t total = 0;
        for (Query* q : qs) {
            Query& s = *q->derived[k].sub.query;
            if (s.groupRowWords != s0.groupRowWords || s.aggMode != s0.aggMode) throw Error(RSQ_ERR_RUNTIME, "internal: shards disagree on the group rows of a derived aggregation");
            subs.push_back(&s);
            total += s.nGroupRows;
        }
        if (!s0.agg) failUnsupported("a derived table without an aggregation");
        bool device = deviceTailTakes(total) && s0.dGroupRows;
        if (device && s0.rowTail < 0) s0.rowTail = planRowsDeviceTail(s0, s0.rtKeys, s0.rtCols, s0.rtTupleSize, s0.rtLimitRows, s0.rtSorts) ? 1 : 0;
        device = device && s0.rowTail == 1 && !s0.rtSorts && s0.accums.size() <= 32;
        if (!device) {
            for (Query* s : subs) fetchHeldGroupRows(*s);
            for (int i = 1; i < n; i++) moved += subs[(size_t)i]->nGroupRows * subs[(size_t)i]->groupRowWords * 8;
            runTailMerged(s0, subs);
            return "on the host";
        }
        const int stride = s0.groupRowWords;
        const HashTable& ht = *s0.hashTables[(size_t)s0.aggTable];
        GroupMergeSpec spec{};
        spec.stride = stride; spec.nTab = (int32_t)(ht.keys.size() + ht.payload.size()); spec.nAcc = (int32_t)s0.accums.size();
        spec.keys = s0.rtKeys;
        for (size_t w = 0; w < s0.accums.size(); w++) { spec.accWord[w] = 1 + spec.nTab + s0.accumSlot[w]; spec.accKind[w] = s0.accums[w].merge; }
        auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
        const size_t rowBytes = (size_t)total * (size_t)stride * 8;
        char* buf = (char*)mergeBuffer(root, d0, up(rowBytes) * 2 + up(groupMergeTempBytes(total)) + 256);
        int64_t* gathered = (int64_t*)buf;
        int64_t* mergedRows = (int64_t*)(buf + up(rowBytes));
        void* temp = buf + up(rowBytes) * 2;
        uint64_t* dCount = (uint64_t*)(buf + up(rowBytes) * 2 + up(groupMergeTempBytes(total)));
        std::vector<GatherPart> parts;
        for (int i = 0; i < n; i++) parts.push_back({&subs[(size_t)i]->ctx, subs[(size_t)i]->dGroupRows, (size_t)subs[(size_t)i]->nGroupRows * (size_t)stride * 8, done[(size_t)i].get()});
        moved += gatherParts(root, gathered, parts);
        mergeGroupRows(root, gathered, total, spec, temp, mergedRows, dCount);
        uint64_t groups = 0;
        uint32_t err = 0;
        RSQ_HIP(hipMemcpyAsync(&groups, dCount, 8, hipMemcpyDeviceToHost, root.stream));
        RSQ_HIP(hipMemcpyAsync(&err, root.dErr, 4, hipMemcpyDeviceToHost, root.stream));
        waitForStream(root);
        if (err) { root.errWordClean = false; checkDeviceError(err); }
        if (groups > (uint64_t)total) throw Error(RSQ_ERR_RUNTIME, "internal: the merge across shards made more groups than it was given rows");
        d0.sub.kernels += 5;
        d0.sub.bytes += (uint64_t)rowBytes;
        s0.resultInPinned = false; s0.resultDev = nullptr;
        const uint64_t before = s0.report.num_kernels;
        runRowsDeviceTail(s0, (int64_t)groups, mergedRows);
        d0.sub.kernels += s0.report.num_kernels - before;      // (the device tail counts its launches in the sub-query's report)
        return "on the device";
    }
};

}  // namespace

std::string planDerivedAcrossShards(const std::vector<Query*>& qs, rsq_table* const* tables, int nTables, const std::vector<bool>& sharded) {
    Planner P;
    P.sharded = &sharded;
    for (int t = 0; t < nTables; t++) P.index[reinterpret_cast<const Table*>(tables[t])] = t;
    std::string text;
    P.classify(qs, "", text);      // (it marks every derived table, at every level, as built by runDerivedAcrossShards)
    // the parent's tables: a sharded one must be the source of the last pipeline (the caller's shard, as every rsq_multi_* plan)
    Query& q0 = *qs[0];
    const Table* last = q0.pipelines.empty() ? nullptr : q0.pipelines.back().src;
    std::vector<OpNode*> scans;
    scansOf(q0.root, scans);
    for (OpNode* o : scans)
        if (P.isSharded(o->table) && o->table != last)
            failUnsupported("table " + o->table->name + " is sharded but is a build side (or the source of an earlier pipeline) of a plan with derived aggregations: "
                            "across GPUs only the source of the last pipeline and one table of a derived aggregation may be sharded - replicate " + o->table->name);
    // a derived table the last pipeline scans: every shard scans its slice (else every row would be counted once per shard)
    if (last && last->derived && qs.size() > 1)
        for (size_t k = 0; k < q0.derived.size(); k++)
            if (q0.derived[k].table.get() == last)
                for (size_t i = 0; i < qs.size(); i++) { qs[i]->derived[k].sliceShards = (int)qs.size(); qs[i]->derived[k].sliceAt = (int)i; }
    std::string where;
    for (size_t k = 0; k < q0.derived.size(); k++)
        where += (where.empty() ? "" : ", ") + q0.derived[k].table->name + (q0.derived[k].multi == MERGED ? " merged" : " local") +
                 (q0.derived[k].sliceShards > 0 ? " sliced" : " whole");
    return where + (text.empty() ? "" : " (" + text + ")");
}

void runDerivedAcrossShards(const std::vector<Query*>& qs, DerivedMultiRun& out) {
    out = DerivedMultiRun();
    Runner{&out}.run(qs, "");
}

}  // namespace rsq
