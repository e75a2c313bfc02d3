// api.cpp — the extern "C" surface of include/resql_hip.h.  No exception crosses it.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <map>
#include <thread>

#include "engine.h"
#include "sqlfront.h"
#include "hostref.h"
#include "result_pack.h"
#include "order_sort.h"

using namespace rsq;

namespace {
thread_local std::string g_createError;

template <typename F>
int guarded(Context* ctx, F&& f) {
    try { f(); return RSQ_OK; }
    catch (const Error& e) { if (ctx) ctx->lastError = e.what(); else g_createError = e.what(); return e.status; }
    catch (const std::bad_alloc&) { if (ctx) ctx->lastError = "out of host memory"; return RSQ_ERR_NOMEM; }
    catch (const std::exception& e) { if (ctx) ctx->lastError = e.what(); else g_createError = e.what(); return RSQ_ERR_INVALID; }
}

Context* C(rsq_ctx* c) { return reinterpret_cast<Context*>(c); }
Table* T(rsq_table* t) { return reinterpret_cast<Table*>(t); }
Query* Q(rsq_query* q) { return reinterpret_cast<Query*>(q); }

struct QueryHandle { Context* ctx; Query* q; };

Table* makeTable(Context& ctx, const rsq_table_desc& d, bool adopt, double* statsMs = nullptr) {
    std::unique_ptr<Table> t(new Table());
    t->ctx = &ctx;
    t->name = std::string(d.name, strnlen(d.name, RSQ_SYMBOL_MAX));
    t->nRows = d.n_rows;
    if (d.n_rows < 0 || d.n_cols < 0) failInvalid("negative table size");
    for (int i = 0; i < d.n_cols; i++) {
        const rsq_column& c = d.cols[i];
        TableColumn tc;
        tc.name = std::string(c.name, strnlen(c.name, RSQ_SYMBOL_MAX));
        tc.type = Type::fromC(c.type);
        size_t bytes = (size_t)d.n_rows * (size_t)columnWidth(tc.type);
        if (c.data) {
            if (adopt) { tc.dptr = const_cast<void*>(c.data); tc.owned = false; }
            else if (ctx.device >= 0) {
                tc.dptr = ctx.allocRaw(bytes); tc.owned = true;
                if (bytes) RSQ_HIP(hipMemcpy(tc.dptr, c.data, bytes, hipMemcpyHostToDevice));
            } else {   // compile-only context: keep a host copy for the statistics
                tc.dptr = malloc(bytes ? bytes : 1); tc.owned = true;
                if (!tc.dptr) throw std::bad_alloc();
                memcpy(tc.dptr, c.data, bytes);
            }
        }
        t->cols.push_back(tc);
    }
    const auto t0 = std::chrono::steady_clock::now();
    computeColumnStats(ctx, *t);
    if (statsMs) *statsMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return t.release();
}
}  // namespace

// rsq_config as the host's header declared it: struct_size bytes are the host's, everything behind them reads as 0
namespace rsq {
rsq_config readConfig(const rsq_config* cfg, bool multiBase) {
    rsq_config c{};
    c.struct_size = (uint32_t)sizeof(rsq_config);
    if (!cfg) return c;
    const uint32_t have = cfg->struct_size;
    if (have < offsetof(rsq_config, kernel_cache_dir) || have > 4096)
        failInvalid("rsq_config.struct_size is " + std::to_string(have) + ": set it to sizeof(rsq_config) (" + std::to_string(sizeof(rsq_config)) + " in this library)");
    memcpy(&c, cfg, std::min<size_t>(have, sizeof c));
    c.struct_size = (uint32_t)sizeof(rsq_config);
    if (c.emission_order != RSQ_EMIT_REFERENCE && c.emission_order != RSQ_EMIT_ANY) failInvalid("rsq_config.emission_order must be RSQ_EMIT_REFERENCE (0) or RSQ_EMIT_ANY (1)");
    if (c.compat_flags & ~(uint32_t)RSQ_COMPAT_JIT_INT16_CAST) failInvalid("rsq_config.compat_flags has bits this library does not know");
    if (c.engine_flags & ~(uint32_t)(RSQ_ENGINE_DRIVER_ALLOC | RSQ_ENGINE_NO_PLAN_MEMO | RSQ_ENGINE_NESTED_LOOPS | RSQ_ENGINE_DERIVED_MULTI | RSQ_ENGINE_DICT_MULTI)) failInvalid("rsq_config.engine_flags has bits this library does not know");
    if ((c.engine_flags & RSQ_ENGINE_DERIVED_MULTI) && !multiBase)
        failInvalid("rsq_config.engine_flags has RSQ_ENGINE_DERIVED_MULTI, a setting of multi-GPU handles (rsq_multi_config.base) only");
    if ((c.engine_flags & RSQ_ENGINE_DICT_MULTI) && !multiBase)
        failInvalid("rsq_config.engine_flags has RSQ_ENGINE_DICT_MULTI, a setting of multi-GPU handles (rsq_multi_config.base) only");
    if (c.nested_loops_max_pairs < 0) failInvalid("rsq_config.nested_loops_max_pairs is negative (0: the default of 2^36 pairs)");
    if (c.nested_loops_max_pairs == 0) c.nested_loops_max_pairs = (int64_t)1 << 36;
    if (c.nested_loops_inner_slices < 0 || c.nested_loops_inner_slices > 4096)
        failInvalid("rsq_config.nested_loops_inner_slices is " + std::to_string(c.nested_loops_inner_slices) + " (0: chosen per execution, 1: never split, 2..4096: that many)");
    if (c.tbl_ingest != 0 && c.tbl_ingest != 1) failInvalid("rsq_config.tbl_ingest is " + std::to_string(c.tbl_ingest) + " (0: BULK INSERT parses on the host, 1: on the device)");
    return c;
}
}  // namespace rsq

// ---- shard statistics -------------------------------------------------------------------------------------------------------
// One blob per table: [magic | columns | row0 | rows] then per column [valid | ascending | min | max | number of byte values | 256 byte
// values].  Fixed size for a schema, plain little-endian words: what one all-gather between the rank processes moves.
namespace rsq {
namespace {
const uint64_t STATS_MAGIC = 0x3174617473717372ull;      // "rsqstat1"
struct StatsHead { uint64_t magic; int64_t nCols, row0, nRows; };
struct StatsCol { int32_t valid, ascending; int64_t min, max; int32_t nBytes, strict; uint8_t bytes[256]; };
}  // namespace
size_t tableStatsBytes(const Table& t) { return sizeof(StatsHead) + t.cols.size() * sizeof(StatsCol); }
void exportTableStats(const Table& t, void* buf, size_t bytes) {
    if (bytes < tableStatsBytes(t)) failInvalid("statistics buffer too small");
    StatsHead h{STATS_MAGIC, (int64_t)t.cols.size(), t.row0, t.nRows};
    memcpy(buf, &h, sizeof h);
    for (size_t i = 0; i < t.cols.size(); i++) {
        const ColumnStats& st = t.shardStats(i);
        StatsCol c{};
        c.valid = st.valid; c.ascending = st.ascending; c.strict = st.strictlyAscending; c.min = st.min; c.max = st.max; c.nBytes = (int32_t)st.distinctBytes.size();
        for (size_t k = 0; k < st.distinctBytes.size() && k < 256; k++) c.bytes[k] = st.distinctBytes[k];
        memcpy((char*)buf + sizeof h + i * sizeof c, &c, sizeof c);
    }
}
void unifyShardStats(Table& t, const void* blobs, int nShards, size_t blobBytes) {
    if (!blobs || nShards < 1 || blobBytes < tableStatsBytes(t)) failInvalid("shard statistics: " + std::to_string(nShards) + " blob(s) of " + std::to_string(blobBytes) + " bytes do not describe table " + t.name);
    if (t.ownStats.empty()) for (auto& c : t.cols) t.ownStats.push_back(c.stats);
    int64_t total = 0;
    bool mine = false;
    std::vector<ColumnStats> u(t.cols.size());
    std::vector<bool> unknown(t.cols.size(), false), any(t.cols.size(), false);
    for (int s = 0; s < nShards; s++) {
        const char* b = (const char*)blobs + (size_t)s * blobBytes;
        StatsHead h; memcpy(&h, b, sizeof h);
        if (h.magic != STATS_MAGIC || h.nCols != (int64_t)t.cols.size() || h.nRows < 0) failInvalid("shard statistics: blob " + std::to_string(s) + " is not a statistics blob of table " + t.name);
        if (h.row0 == t.row0 && h.nRows == t.nRows) mine = true;
        total += h.nRows;
        if (h.nRows == 0) continue;                      // an empty shard says nothing about the values
        for (size_t i = 0; i < t.cols.size(); i++) {
            StatsCol c; memcpy(&c, b + sizeof h + i * sizeof c, sizeof c);
            if (!c.valid) { unknown[i] = true; continue; }
            if (c.nBytes < 0 || c.nBytes > 256) failInvalid("shard statistics: malformed byte-value set");
            if (c.min > c.max) failInvalid("shard statistics: blob " + std::to_string(s) + " has min > max in column " + t.cols[i].name);
            ColumnStats& o = u[i];
            if (!any[i]) { o.min = c.min; o.max = c.max; any[i] = true; }
            else { o.min = std::min(o.min, c.min); o.max = std::max(o.max, c.max); }
            for (int k = 0; k < c.nBytes; k++) o.distinctBytes.push_back(c.bytes[k]);
        }
    }
    if (!mine) failInvalid("shard statistics: none of the blobs is this shard's own (rows " + std::to_string(t.row0) + " + " + std::to_string(t.nRows) + " of " + t.name + ")");
    for (size_t i = 0; i < t.cols.size(); i++) {
        ColumnStats& o = u[i];
        // this shard's OWN statistics are folded in whatever the blobs said about it: device code trusts the union without a range check
        // for engine-owned columns (codegen_join.cpp checkKey), so a stale or foreign blob must never narrow it below what the rows here hold
        const ColumnStats& own = t.ownStats[i];
        if (own.valid && t.nRows > 0) {
            if (!any[i]) { o.min = own.min; o.max = own.max; any[i] = true; }
            else { o.min = std::min(o.min, own.min); o.max = std::max(o.max, own.max); }
            o.distinctBytes.insert(o.distinctBytes.end(), own.distinctBytes.begin(), own.distinctBytes.end());
        }
        std::sort(o.distinctBytes.begin(), o.distinctBytes.end());
        o.distinctBytes.erase(std::unique(o.distinctBytes.begin(), o.distinctBytes.end()), o.distinctBytes.end());
        o.valid = any[i] && !unknown[i];
        o.ascending = t.ownStats[i].ascending;           // (properties of this shard's own rows: they shape kernels, never a layout)
        o.strictlyAscending = t.ownStats[i].strictlyAscending;
        t.cols[i].stats = o;
    }
    t.nRowsTotal = total;
    t.bumpVersion();
}
}  // namespace rsq

// helpers of the device primitives exposed for tests (rsq_prim_*, below)
namespace {
// device buffers of one call: given back when it ends, also by an exception, once the stream has drained
struct PrimBuffers {
    Context& c;
    std::vector<void*> held;
    explicit PrimBuffers(Context& ctx) : c(ctx) {}
    ~PrimBuffers() { (void)hipStreamSynchronize(c.stream); for (void* p : held) c.free(p); }
    template <typename E> E* take(size_t n) { void* p = c.alloc(std::max<size_t>(n * sizeof(E), 16)); held.push_back(p); return (E*)p; }
};
void primSync(Context& c) { RSQ_HIP(hipStreamSynchronize(c.stream)); c.streamDrained(); }
uint32_t primErrWord(Context& c) {
    uint32_t e = 0;
    RSQ_HIP(hipMemcpyAsync(&e, c.dErr, 4, hipMemcpyDeviceToHost, c.stream));
    primSync(c);
    return e;
}
// the bits the call raised, and the error word as it was before the call
void primNotes(Context& c, uint32_t before, uint32_t* notes) {
    const uint32_t after = primErrWord(c), raised = after & ~before;
    if (raised) {
        const uint32_t keep = after & ~raised;
        RSQ_HIP(hipMemcpyAsync(c.dErr, &keep, 4, hipMemcpyHostToDevice, c.stream));
        primSync(c);
    }
    *notes = raised;
}
Context& primContext(rsq_ctx* ctx) {
    Context& c = *C(ctx);
    if (c.device < 0) failUnsupported("this context has no device (compile-only)");
    RSQ_HIP(hipSetDevice(c.device));
    return c;
}
const int64_t kPrimMaxRankBlocks = (int64_t)1171 * RSQ_RANK_CHUNK_BLOCKS;      // a key domain of 2^28 bits (k_rank_blocks_chained)
const int64_t kPrimMaxItems = (int64_t)1 << 31;      // pairs, values, rows of one call: the kernels' tile and row indices are 32 bits
const int32_t kPrimMaxStride = 4096;                 // words of a group row (a merge)

// A report handed out: the caller's struct_size bytes of it, struct_size kept (a host built against an older header receives the
// fields it knows).  False: struct_size is not one a header of this library can have given.
template <typename R>
bool copyReportOut(const R& report, R* out) {
    if (out->struct_size < 8 || out->struct_size > 4096) return false;
    R r = report;
    r.struct_size = out->struct_size;
    memcpy(out, &r, std::min<size_t>(out->struct_size, sizeof r));
    return true;
}

// rsq_query_<what>_report: the last execution's, of one of the materialisation's device tails (engine_mattail.cpp)
template <typename R>
int queryReportOut(const rsq_query* q, R* out, const char* type) {
    if (!q || !out) return RSQ_ERR_INVALID;
    const QueryHandle* h = reinterpret_cast<const QueryHandle*>(q);
    return guarded(h->ctx, [&] {
        R r{};
        queryReport(*h->q, &r);
        if (!copyReportOut(r, out)) failInvalid(std::string(type) + ".struct_size is " + std::to_string(out->struct_size) + ": set it to sizeof(" + type + ")");
    });
}
}  // namespace

extern "C" {

int64_t rsq_table_stats_bytes(const rsq_table* t) { return t ? (int64_t)tableStatsBytes(*reinterpret_cast<const Table*>(t)) : -1; }
int rsq_table_stats_export(const rsq_table* t, void* buf, int64_t bytes) {
    if (!t || !buf || bytes < 0) return RSQ_ERR_INVALID;
    const Table* tb = reinterpret_cast<const Table*>(t);
    return guarded(tb->ctx, [&] { exportTableStats(*tb, buf, (size_t)bytes); });
}
int rsq_table_unify_shard_stats(rsq_table* t, const void* blobs, int32_t n_shards, int64_t blob_bytes) {
    if (!t || !blobs || blob_bytes < 0) return RSQ_ERR_INVALID;
    return guarded(T(t)->ctx, [&] { unifyShardStats(*T(t), blobs, n_shards, (size_t)blob_bytes); });
}
int rsq_table_unify_shard_dictionaries(rsq_table* const* shards, int32_t n_shards) {
    if (!shards || n_shards < 1) return RSQ_ERR_INVALID;
    for (int32_t i = 0; i < n_shards; i++) if (!shards[i] || !T(shards[i])->ctx) return RSQ_ERR_INVALID;
    // (the message goes to the first shard's context)
    return guarded(T(shards[0])->ctx, [&] {
        std::vector<Table*> ts;
        for (int32_t i = 0; i < n_shards; i++) ts.push_back(T(shards[i]));
        unifyShardDictionaries(ts);
    });
}
int rsq_table_time_dictionary_pass(rsq_table* t, const char* column, int32_t which, double* ms) {
    if (!t || !column || !ms || !T(t)->ctx) return RSQ_ERR_INVALID;
    return guarded(T(t)->ctx, [&] {
        const int ci = T(t)->findCol(column);
        if (ci < 0) failInvalid(std::string("no such column: ") + column);
        *ms = timeDictPass(*T(t)->ctx, *T(t), ci, which);
    });
}
int64_t rsq_table_total_rows(const rsq_table* t) { return t ? reinterpret_cast<const Table*>(t)->totalRows() : -1; }

int rsq_ctx_create(const rsq_config* cfg, rsq_ctx** out) {
    if (!out) return RSQ_ERR_INVALID;
    *out = nullptr;
    return guarded(nullptr, [&] { *out = reinterpret_cast<rsq_ctx*>(new Context(readConfig(cfg))); });
}

void rsq_ctx_destroy(rsq_ctx* ctx) { delete C(ctx); }

const char* rsq_last_error(const rsq_ctx* ctx) {
    if (!ctx) return g_createError.c_str();
    return reinterpret_cast<const Context*>(ctx)->lastError.c_str();
}

int rsq_ctx_memory_stats(const rsq_ctx* ctx, rsq_memory_stats* out) {
    if (!ctx || !out) return RSQ_ERR_INVALID;
    const Context& c = *reinterpret_cast<const Context*>(ctx);
    const uint32_t have = out->struct_size;
    if (have < offsetof(rsq_memory_stats, device_used_bytes) || have > 4096) return RSQ_ERR_INVALID;
    rsq_memory_stats m{};
    m.struct_size = (uint32_t)sizeof m;
    if (c.devArena) { m.device_slab_bytes = c.devArena->slabBytes(); m.device_used_bytes = c.devArena->usedBytes(); m.device_slab_allocs = c.devArena->nSlabAllocs; m.arena_requests += c.devArena->nAllocs; m.driver_ms += c.devArena->slabAllocMs; }
    for (const Arena* a : {c.pinArena.get(), c.pinNcArena.get()})
        if (a) { m.pinned_slab_bytes += a->slabBytes(); m.pinned_used_bytes += a->usedBytes(); m.pinned_slab_allocs += a->nSlabAllocs; m.arena_requests += a->nAllocs; m.driver_ms += a->slabAllocMs; }
    m.raw_driver_calls = c.allocStats.rawCalls;
    m.driver_ms += c.allocStats.rawMs;
    m.plan_memo_entries = c.planMemo.size();
    m.plan_memo_hits = c.planMemoHits;
    m.key_index_entries = c.keyIndexes.size();
    for (auto& kv : c.keyIndexes) m.key_index_bytes += (uint64_t)kv.second.bmBlocks * 32;
    m.column_image_bytes = c.columnImageBytes;
    memcpy(out, &m, std::min<size_t>(have, sizeof m));
    out->struct_size = have;
    return RSQ_OK;
}

int rsq_table_create(rsq_ctx* ctx, const rsq_table_desc* desc, rsq_table** out) {
    if (!ctx || !desc || !out) return RSQ_ERR_INVALID;
    return guarded(C(ctx), [&] { *out = reinterpret_cast<rsq_table*>(makeTable(*C(ctx), *desc, false)); });
}

int rsq_table_create_device(rsq_ctx* ctx, const rsq_table_desc* desc, rsq_table** out) {
    if (!ctx || !desc || !out) return RSQ_ERR_INVALID;
    return guarded(C(ctx), [&] {
        if (C(ctx)->device < 0) throw Error(RSQ_ERR_DEVICE, "rsq_table_create_device needs a device context");
        *out = reinterpret_cast<rsq_table*>(makeTable(*C(ctx), *desc, true));
    });
}

int rsq_table_from_rowstore(rsq_ctx* ctx, const rsq_table_desc* schema, const uint8_t* const* blocks,
                            const size_t* content_size, int32_t n_blocks, rsq_table** out) {
    return rsq_table_from_rowstore_ex(ctx, schema, blocks, content_size, n_blocks, nullptr, nullptr, out);
}

int rsq_table_from_rowstore_ex(rsq_ctx* ctx, const rsq_table_desc* schema, const uint8_t* const* blocks, const size_t* content_size,
                               int32_t n_blocks, const rsq_rowstore_options* options, rsq_rowstore_report* report, rsq_table** out) {
    if (!ctx || !schema || !out || n_blocks < 0) return RSQ_ERR_INVALID;
    if (schema->n_cols <= 0 || (n_blocks > 0 && (!blocks || !content_size))) return RSQ_ERR_INVALID;
    return guarded(C(ctx), [&] {
        Context& cx = *C(ctx);
        rsq_rowstore_options opt{};
        if (options) {
            if (options->struct_size < 8 || options->struct_size > 4096) failInvalid("rsq_rowstore_options.struct_size is " + std::to_string(options->struct_size) + ": set it to sizeof(rsq_rowstore_options)");
            memcpy(&opt, options, std::min<size_t>(options->struct_size, sizeof opt));
        }
        if (report && (report->struct_size < 8 || report->struct_size > 4096)) failInvalid("rsq_rowstore_report.struct_size is " + std::to_string(report->struct_size) + ": set it to sizeof(rsq_rowstore_report)");
        if (opt.mode < 0 || opt.mode > 2) failInvalid("rsq_rowstore_options.mode must be 0 (the context's rowstore_bridge setting), 1 (host) or 2 (device)");
        if (opt.chunk_bytes < 0 || opt.chunk_bytes > ((int64_t)1 << 30)) failInvalid("rsq_rowstore_options.chunk_bytes is " + std::to_string(opt.chunk_bytes) + " (0: 64 MiB; at most 1 GiB)");
        const bool device = opt.mode == 2 || (opt.mode == 0 && cx.rowstoreBridge == 1);
        std::vector<Type> types;
        for (int i = 0; i < schema->n_cols; i++) types.push_back(Type::fromC(schema->cols[i].type));
        rsq_rowstore_report rep{};
        const auto started = std::chrono::steady_clock::now();
        auto ms = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
        // (a type no column holds raises here, on either path and in front of every allocation, what it always raised)
        const RowstoreLayout layout = rowstoreLayout(types);
        int64_t n = rowstoreRows(content_size, n_blocks, layout.tupleSize);
        std::unique_ptr<Table> t;
        if (device) t = rowstoreToDevice(cx, *schema, types, layout, blocks, content_size, n_blocks, n, opt.chunk_bytes, rep);
        if (t) {
            const auto t0 = std::chrono::steady_clock::now();
            computeColumnStats(cx, *t);
            rep.stats_ms = ms(t0);
        }
        if (!t) {
            // the host path: packed ReSQL tuples (strings by value, schema.h:76-106 offsets) transposed into columns by one host thread
            // (rowstore.cpp), then uploaded - all of it, also where the device path gave up (its reason stays in the report)
            const int32_t why = rep.fallback_reason;
            rep = rsq_rowstore_report{};
            rep.fallback_reason = why;
            std::vector<std::vector<uint8_t>> cols;
            auto t0 = std::chrono::steady_clock::now();
            transposeRowstoreHost(types, blocks, content_size, n_blocks, cols, n);
            rep.transpose_ms = ms(t0);
            std::vector<rsq_column> cd((size_t)schema->n_cols);
            for (int i = 0; i < schema->n_cols; i++) { cd[(size_t)i] = schema->cols[i]; cd[(size_t)i].data = cols[(size_t)i].data(); }
            rsq_table_desc d = *schema; d.n_rows = n; d.cols = cd.data();
            t0 = std::chrono::steady_clock::now();
            t.reset(makeTable(cx, d, false, &rep.stats_ms));
            rep.copy_ms = ms(t0) - rep.stats_ms;
        }
        rep.rows = n; rep.tuple_bytes = n * (int64_t)layout.tupleSize;
        rep.total_ms = ms(started);
        if (report) {
            const uint32_t have = report->struct_size;
            rep.struct_size = have;
            memcpy(report, &rep, std::min<size_t>(have, sizeof rep));
        }
        *out = reinterpret_cast<rsq_table*>(t.release());
    });
}

int rsq_ctx_set_rowstore_bridge(rsq_ctx* ctx, int32_t where) {
    if (!ctx) return RSQ_ERR_INVALID;
    return guarded(C(ctx), [&] {
        if (where != 0 && where != 1) failInvalid("rowstore_bridge is " + std::to_string(where) + " (0: row stores are transposed on the host, 1: on the device)");
        C(ctx)->rowstoreBridge = where;
    });
}

int rsq_table_load_tbl(rsq_ctx* ctx, const rsq_table_desc* schema, const char* path, char field_terminator,
                       int32_t n_threads, rsq_table** out) {
    return rsq_table_load_tbl_ex(ctx, schema, path, field_terminator, n_threads, nullptr, nullptr, out);
}

int rsq_table_load_tbl_ex(rsq_ctx* ctx, const rsq_table_desc* schema, const char* path, char field_terminator, int32_t n_threads,
                          const rsq_tbl_load_options* options, rsq_tbl_load_report* report, rsq_table** out) {
    if (!ctx || !schema || !path || !out || schema->n_cols < 0) return RSQ_ERR_INVALID;
    return guarded(C(ctx), [&] {
        Context& cx = *C(ctx);
        rsq_tbl_load_options opt{};
        if (options) {
            if (options->struct_size < 8 || options->struct_size > 4096) failInvalid("rsq_tbl_load_options.struct_size is " + std::to_string(options->struct_size) + ": set it to sizeof(rsq_tbl_load_options)");
            memcpy(&opt, options, std::min<size_t>(options->struct_size, sizeof opt));
        }
        if (report && (report->struct_size < 8 || report->struct_size > 4096)) failInvalid("rsq_tbl_load_report.struct_size is " + std::to_string(report->struct_size) + ": set it to sizeof(rsq_tbl_load_report)");
        if (opt.mode < 0 || opt.mode > 2) failInvalid("rsq_tbl_load_options.mode must be 0 (the context's tbl_ingest), 1 (host) or 2 (device)");
        if (opt.chunk_bytes < 0 || (opt.chunk_bytes > 0 && opt.chunk_bytes < 64)) failInvalid("rsq_tbl_load_options.chunk_bytes is " + std::to_string(opt.chunk_bytes) + " (0: 64 MiB; at least 64)");
        if (opt.max_device_text_bytes < 0) failInvalid("rsq_tbl_load_options.max_device_text_bytes is negative (0: what is free on the device minus 1 GiB)");
        const bool device = opt.mode == 2 || (opt.mode == 0 && cx.cfg.tbl_ingest == 1);
        std::vector<Type> types;
        for (int i = 0; i < schema->n_cols; i++) types.push_back(Type::fromC(schema->cols[i].type));
        rsq_tbl_load_report rep{};
        const auto started = std::chrono::steady_clock::now();
        auto ms = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
        std::unique_ptr<Table> t;
        if (device) t = loadTblDevice(cx, *schema, types, path, field_terminator, opt.chunk_bytes, opt.max_device_text_bytes, rep);
        if (t) {
            const auto t0 = std::chrono::steady_clock::now();
            computeColumnStats(cx, *t);
            rep.stats_ms = ms(t0);
        } else {
            // the host path: all of it, also after a device load that gave up (its reason stays in the report)
            const int32_t why = rep.fallback_reason;
            rep = rsq_tbl_load_report{};
            rep.fallback_reason = why;
            std::vector<std::vector<uint8_t>> cols;
            int64_t n = 0;
            int threads = n_threads > 0 ? n_threads : (int)std::max(1u, std::thread::hardware_concurrency());
            auto t0 = std::chrono::steady_clock::now();
            parseTblFile(path, types, field_terminator, threads, cols, n);
            rep.read_ms = ms(t0);
            static const uint8_t kEmpty[16] = {0};       // an empty file still gives columns WITH data (of zero rows)
            std::vector<rsq_column> cd((size_t)schema->n_cols);
            for (int i = 0; i < schema->n_cols; i++) {
                cd[(size_t)i] = schema->cols[i];
                cd[(size_t)i].data = cols[(size_t)i].empty() ? (const void*)kEmpty : (const void*)cols[(size_t)i].data();
            }
            rsq_table_desc d = *schema; d.n_rows = n; d.cols = cd.data();
            t0 = std::chrono::steady_clock::now();
            t.reset(makeTable(cx, d, false, &rep.stats_ms));
            rep.copy_ms = ms(t0) - rep.stats_ms;
            rep.rows = n;
            FILE* f = fopen(path, "rb");          // (the size alone: parseTblFile has read the file)
            if (f) { if (fseek(f, 0, SEEK_END) == 0) rep.text_bytes = (int64_t)ftell(f); fclose(f); }
        }
        rep.total_ms = ms(started);
        if (report) {
            const uint32_t have = report->struct_size;
            rep.struct_size = have;
            memcpy(report, &rep, std::min<size_t>(have, sizeof rep));
        }
        *out = reinterpret_cast<rsq_table*>(t.release());
    });
}

int rsq_table_generate(rsq_ctx* ctx, int32_t kind, int64_t row0, int64_t n_rows, double scale_factor,
                       int64_t param, uint64_t seed, rsq_table** out) {
    if (!ctx || !out || n_rows < 0) return RSQ_ERR_INVALID;
    return guarded(C(ctx), [&] {
        std::unique_ptr<Table> t(new Table());
        generateTable(*C(ctx), *t, kind, row0, n_rows, scale_factor, param, seed);
        *out = reinterpret_cast<rsq_table*>(t.release());
    });
}

int64_t rsq_table_rows(const rsq_table* t) { return t ? reinterpret_cast<const Table*>(t)->nRows : -1; }
int rsq_table_set_first_row(rsq_table* t, int64_t row0) {
    if (!t || row0 < 0) return RSQ_ERR_INVALID;
    reinterpret_cast<Table*>(t)->row0 = row0;
    reinterpret_cast<Table*>(t)->bumpVersion();
    return RSQ_OK;
}

int rsq_table_refresh_stats(rsq_table* t) {
    if (!t) return RSQ_ERR_INVALID;
    Table& tab = *reinterpret_cast<Table*>(t);
    if (!tab.ctx) return RSQ_ERR_INVALID;
    return guarded(tab.ctx, [&] {
        if (!tab.ownStats.empty()) failInvalid("rsq_table_refresh_stats: the table plans with unified shard statistics; refresh the shards and unify again");
        computeColumnStats(*tab.ctx, tab);
        tab.bumpVersion();          // (the context's plan memo: what queries learnt over the old content does not describe the new)
    });
}

int rsq_table_read_column(rsq_ctx* ctx, const rsq_table* t, const char* name, void* host_dst, size_t bytes) {
    if (!ctx || !t || !name || !host_dst) return RSQ_ERR_INVALID;
    return guarded(C(ctx), [&] {
        const Table* tb = reinterpret_cast<const Table*>(t);
        int ci = tb->findCol(name);
        if (ci < 0 || !tb->cols[(size_t)ci].dptr) failInvalid(std::string("no such column: ") + name);
        size_t have = (size_t)tb->nRows * (size_t)columnWidth(tb->cols[(size_t)ci].type);
        if (bytes > have) failInvalid("read beyond the column");
        if (C(ctx)->device >= 0) RSQ_HIP(hipMemcpy(host_dst, tb->cols[(size_t)ci].dptr, bytes, hipMemcpyDeviceToHost));
        else memcpy(host_dst, tb->cols[(size_t)ci].dptr, bytes);
    });
}

int rsq_table_read_image(rsq_ctx* ctx, const rsq_table* t, const char* name, int32_t which, void* host_dst, size_t bytes, int64_t info[4]) {
    if (!ctx || !t || !name || !info || which < 0 || which > 2 || (bytes && !host_dst)) return RSQ_ERR_INVALID;
    return guarded(C(ctx), [&] {
        const Table* tb = reinterpret_cast<const Table*>(t);
        if (tb->ctx != C(ctx)) failInvalid("the table belongs to another context");
        int ci = tb->findCol(name);
        if (ci < 0) failInvalid(std::string("no such column: ") + name);
        const TableColumn& c = tb->cols[(size_t)ci];
        info[0] = c.nw; info[1] = c.nw ? c.nbase : 0; info[2] = c.dictN; info[3] = tb->nRows;
        if (!bytes) return;
        const bool device = C(ctx)->device >= 0;
        if (!device && which != 1) failUnsupported("a compile-only context keeps no narrow image and no dictionary codes");
        const size_t have = which == 0 ? (size_t)tb->nRows * (size_t)c.nw
                          : which == 1 ? (size_t)c.dictN * (size_t)columnWidth(c.type)
                                       : (c.dictN ? (size_t)tb->nRows : 0);
        if (bytes > have) failInvalid("read beyond the image");
        if (!device) { memcpy(host_dst, c.dict.data(), bytes); return; }
        const void* src = which == 0 ? c.nptr : which == 1 ? c.dictPtr : c.codePtr;
        if (!src) failInvalid("the column has no such image");
        RSQ_HIP(hipStreamSynchronize(C(ctx)->stream));
        RSQ_HIP(hipMemcpy(host_dst, src, bytes, hipMemcpyDeviceToHost));
    });
}

void rsq_table_destroy(rsq_table* t) { delete T(t); }

int rsq_query_compile(rsq_ctx* ctx, const rsq_plan_desc* plan, rsq_table* const* tables, int32_t n_tables, rsq_query** out) {
    if (!ctx || !plan || !out || n_tables < 0) return RSQ_ERR_INVALID;
    *out = nullptr;
    return guarded(C(ctx), [&] {
        std::unique_ptr<QueryHandle> h(new QueryHandle{C(ctx), nullptr});
        h->q = compileQuery(*C(ctx), *plan, tables, n_tables);
        *out = reinterpret_cast<rsq_query*>(h.release());
    });
}

#define QH(q) reinterpret_cast<QueryHandle*>(q)

int rsq_query_execute(rsq_query* q) {
    if (!q) return RSQ_ERR_INVALID;
    return guarded(QH(q)->ctx, [&] { executeQuery(*QH(q)->q, false); });
}

int rsq_query_await_kernels(rsq_query* q) {
    if (!q) return RSQ_ERR_INVALID;
    return guarded(QH(q)->ctx, [&] { awaitKernels(*QH(q)->q); });
}

int rsq_query_execute_partial(rsq_query* q, void** dev_ptr, int64_t* n_min_words, int64_t* n_max_words, int64_t* n_sum_words) {
    if (!q || !dev_ptr || !n_min_words || !n_max_words || !n_sum_words) return RSQ_ERR_INVALID;
    return guarded(QH(q)->ctx, [&] {
        executeQuery(*QH(q)->q, true);
        partialBuffer(*QH(q)->q, dev_ptr, n_min_words, n_max_words, n_sum_words);
    });
}

int rsq_query_execute_partial_async(rsq_query* q) {
    if (!q) return RSQ_ERR_INVALID;
    return guarded(QH(q)->ctx, [&] { executeQuery(*QH(q)->q, true, true); });
}

int rsq_ctx_set_stream(rsq_ctx* ctx, void* hip_stream, int32_t use_callers_stream) {
    if (!ctx) return RSQ_ERR_INVALID;
    return guarded(C(ctx), [&] { C(ctx)->setStream((hipStream_t)hip_stream, use_callers_stream != 0); });
}

int rsq_query_partial_layout(const rsq_query* q, int64_t* n_min_words, int64_t* n_max_words, int64_t* n_sum_words) {
    if (!q || !n_min_words || !n_max_words || !n_sum_words) return RSQ_ERR_INVALID;
    const QueryHandle* h = reinterpret_cast<const QueryHandle*>(q);
    return guarded(h->ctx, [&] { void* p = nullptr; partialBuffer(*h->q, &p, n_min_words, n_max_words, n_sum_words); });
}

int rsq_query_bind_partial(rsq_query* q, void* dev_ptr, size_t bytes) {
    if (!q) return RSQ_ERR_INVALID;
    return guarded(QH(q)->ctx, [&] { bindPartial(*QH(q)->q, dev_ptr, bytes); });
}

int rsq_query_merge_gathered(rsq_query* q, const void* gathered_dev, int32_t n_ranks) {
    if (!q) return RSQ_ERR_INVALID;
    return guarded(QH(q)->ctx, [&] { mergeGathered(*QH(q)->q, gathered_dev, n_ranks); });
}

int rsq_query_finalize_host(rsq_query* q, const int64_t* words, int64_t n_words) {
    if (!q || !words || n_words < 0) return RSQ_ERR_INVALID;
    return guarded(QH(q)->ctx, [&] { finalizeQueryHost(*QH(q)->q, words, (size_t)n_words); });
}

int rsq_query_finalize(rsq_query* q) {
    if (!q) return RSQ_ERR_INVALID;
    return guarded(QH(q)->ctx, [&] { finalizeQuery(*QH(q)->q); });
}

int rsq_query_result(rsq_query* q, rsq_result_view* out) {
    if (!q || !out) return RSQ_ERR_INVALID;
    return guarded(QH(q)->ctx, [&] { queryResult(*QH(q)->q, out); });
}

int rsq_query_report(const rsq_query* q, rsq_report* out) {
    if (!q || !out) return RSQ_ERR_INVALID;
    const QueryHandle* h = reinterpret_cast<const QueryHandle*>(q);
    return guarded(h->ctx, [&] { queryReport(*h->q, out); });
}

int rsq_query_kernel_time_stats(rsq_query* q, double* sum_ms, uint64_t* executions, int32_t reset) {
    if (!q) return RSQ_ERR_INVALID;
    return guarded(QH(q)->ctx, [&] { queryKernelTimeStats(*QH(q)->q, sum_ms, executions, reset != 0); });
}

int rsq_query_nested_loops_slices(const rsq_query* q, int32_t* out) {
    if (!q || !out) return RSQ_ERR_INVALID;
    const QueryHandle* h = reinterpret_cast<const QueryHandle*>(q);
    return guarded(h->ctx, [&] {
        *out = queryNestedLoopsSlices(*h->q);
    });
}

// slices of a nested-loops pair loop's inner range (resql_hip.h)
int32_t rsq_nested_loops_slices(int64_t base_workgroups, int64_t max_workgroups, int64_t inner_rows, int32_t configured) {
    const int64_t cap = std::max<int64_t>(1, max_workgroups), base = std::max<int64_t>(1, base_workgroups);
    if (configured == 1) return 1;
    if (configured >= 2) return (int32_t)std::min<int64_t>(configured, cap);
    const int64_t byRows = inner_rows <= 0 ? 1 : (inner_rows + RSQ_NLJ_MIN_SLICE_ROWS - 1) / RSQ_NLJ_MIN_SLICE_ROWS;
    return (int32_t)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(cap / base, byRows), INT32_MAX));
}

const char* rsq_query_source(const rsq_query* q) { return q ? querySource(*reinterpret_cast<const QueryHandle*>(q)->q) : ""; }
const char* rsq_query_explain(const rsq_query* q) { return q ? queryExplain(*reinterpret_cast<const QueryHandle*>(q)->q) : ""; }

void rsq_query_destroy(rsq_query* q) {
    if (!q) return;
    destroyQuery(QH(q)->q);
    delete QH(q);
}

char* rsq_serialize_expr(rsq_ctx* ctx, const rsq_plan_desc* plan, int32_t expr, int32_t derive,
                         rsq_table* const* tables, int32_t n_tables) {
    if (!ctx || !plan) return nullptr;
    char* res = nullptr;
    guarded(C(ctx), [&] {
        ExprPool pool;
        for (int i = 0; i < n_tables; i++)
            for (auto& c : T(tables[i])->cols) pool.identTypes[c.name] = c.type;
        std::vector<Expr*> v = pool.build(*plan);
        if (expr < 0 || expr >= (int)v.size()) failInvalid("bad expression index");
        if (derive) pool.derive(v[(size_t)expr]);
        res = strdup(serializeExpr(v[(size_t)expr]).c_str());
    });
    return res;
}

char* rsq_result_serialize(const rsq_result_view* view) {
    if (!view) return nullptr;
    try { return strdup(serializeResultView(*view).c_str()); } catch (...) { return nullptr; }
}

void rsq_free(void* p) { free(p); }

namespace {
// options and report of rsq_query_result_text / _write as the host's header declared them
void readTextOptions(const rsq_result_text_options* options, const rsq_result_text_report* report, rsq_result_text_options& opt) {
    opt = rsq_result_text_options{};
    if (options) {
        if (options->struct_size < 8 || options->struct_size > 4096) failInvalid("rsq_result_text_options.struct_size is " + std::to_string(options->struct_size) + ": set it to sizeof(rsq_result_text_options)");
        memcpy(&opt, options, std::min<size_t>(options->struct_size, sizeof opt));
    }
    if (report && (report->struct_size < 8 || report->struct_size > 4096)) failInvalid("rsq_result_text_report.struct_size is " + std::to_string(report->struct_size) + ": set it to sizeof(rsq_result_text_report)");
    if (opt.mode < 0 || opt.mode > 2) failInvalid("rsq_result_text_options.mode must be 0 (the context's result_text setting), 1 (host) or 2 (device)");
    if (opt.chunk_rows < 0) failInvalid("rsq_result_text_options.chunk_rows is negative (0: chosen)");
    if (opt.max_device_bytes < 0) failInvalid("rsq_result_text_options.max_device_bytes is negative (0: what is free on the device minus 1 GiB)");
}
void handTextReport(rsq_result_text_report rep, rsq_result_text_report* report) {
    if (!report) return;
    const uint32_t have = report->struct_size;
    rep.struct_size = have;
    memcpy(report, &rep, std::min<size_t>(have, sizeof rep));
}
}  // namespace

int rsq_query_result_text(rsq_query* q, const rsq_result_text_options* options, rsq_result_text_report* report, char** text, int64_t* text_bytes) {
    if (!q || !text || !text_bytes) return RSQ_ERR_INVALID;
    *text = nullptr; *text_bytes = 0;
    return guarded(QH(q)->ctx, [&] {
        Context& cx = *QH(q)->ctx;
        rsq_result_text_options opt;
        readTextOptions(options, report, opt);
        rsq_result_view view;
        queryResult(*QH(q)->q, &view);
        TextOut out;
        rsq_result_text_report rep{};
        writeResultText(cx, view, queryResultDeviceTuples(*QH(q)->q), opt.mode == 2 || (opt.mode == 0 && cx.resultText == 1), opt.chunk_rows, opt.max_device_bytes, out, rep);
        handTextReport(rep, report);
        *text_bytes = (int64_t)out.size;
        *text = out.release();
    });
}

int rsq_query_result_write(rsq_query* q, const char* path, const rsq_result_text_options* options, rsq_result_text_report* report) {
    if (!q || !path) return RSQ_ERR_INVALID;
    return guarded(QH(q)->ctx, [&] {
        Context& cx = *QH(q)->ctx;
        rsq_result_text_options opt;
        readTextOptions(options, report, opt);
        rsq_result_view view;
        queryResult(*QH(q)->q, &view);
        TextOut out;
        out.file = fopen(path, "w");
        if (!out.file) failInvalid(std::string("Could not open file ") + path);
        rsq_result_text_report rep{};
        writeResultText(cx, view, queryResultDeviceTuples(*QH(q)->q), opt.mode == 2 || (opt.mode == 0 && cx.resultText == 1), opt.chunk_rows, opt.max_device_bytes, out, rep);
        out.closeFile();
        handTextReport(rep, report);
    });
}

int rsq_ctx_set_row_cells(rsq_ctx* ctx, int32_t mode) {
    if (!ctx) return RSQ_ERR_INVALID;
    return guarded(C(ctx), [&] {
        if (mode < -1 || mode > 1) failInvalid("row_cells is " + std::to_string(mode) + " (-1: chosen by the executions' kernel times, 0: no second form, 1: in every launch that fits it)");
        C(ctx)->rowCellsMode = mode;
    });
}

// a context's setting of 0 or 1; the refusal of any other value says `name` and, in parentheses, what the two `mean`
static int setZeroOrOne(rsq_ctx* ctx, int32_t Context::* member, int32_t where, const char* name, const char* means) {
    if (!ctx) return RSQ_ERR_INVALID;
    return guarded(C(ctx), [&] {
        if (where != 0 && where != 1) failInvalid(std::string(name) + " is " + std::to_string(where) + " (" + means + ")");
        C(ctx)->*member = where;
    });
}

int rsq_ctx_set_result_text(rsq_ctx* ctx, int32_t where) {
    return setZeroOrOne(ctx, &Context::resultText, where, "result_text", "0: results become text on the host, 1: on the device");
}
int rsq_ctx_set_order_limit(rsq_ctx* ctx, int32_t where) {
    return setZeroOrOne(ctx, &Context::orderLimit, where, "order_limit", "0: ORDER BY ... LIMIT over a materialisation sorts every row on the host, 1: decides from candidates selected on the device");
}
int rsq_ctx_set_result_pack(rsq_ctx* ctx, int32_t where) {
    return setZeroOrOne(ctx, &Context::resultPack, where, "result_pack", "0: a materialisation's result tuples are packed on the host, 1: on the device");
}
int rsq_ctx_set_order_sort(rsq_ctx* ctx, int32_t where) {
    return setZeroOrOne(ctx, &Context::orderSort, where, "order_sort", "0: an ORDER BY over a materialisation sorts the tuples on the host, 1: the device orders the rows");
}

int rsq_query_order_limit_report(const rsq_query* q, rsq_order_limit_report* out) { return queryReportOut(q, out, "rsq_order_limit_report"); }
int rsq_query_result_pack_report(const rsq_query* q, rsq_result_pack_report* out) { return queryReportOut(q, out, "rsq_result_pack_report"); }
int rsq_query_order_sort_report(const rsq_query* q, rsq_order_sort_report* out) { return queryReportOut(q, out, "rsq_order_sort_report"); }

int rsq_ref_emission_order_device(rsq_ctx* ctx, const uint64_t* hashes, int64_t n, uint64_t min_size, uint32_t* out) {
    if (!ctx || n < 0 || (n > 0 && (!hashes || !out))) return RSQ_ERR_INVALID;
    return guarded(C(ctx), [&] {
        Context& c = *C(ctx);
        if (c.device < 0) throw Error(RSQ_ERR_DEVICE, "this context has no device (compile-only)");
        if (n == 0) return;
        std::vector<std::pair<uint64_t, uint64_t>> levels;
        if (!replayLevels((uint64_t)n, min_size, levels)) failUnsupported("the device replay does not take tables of this size");
        RSQ_HIP(hipSetDevice(c.device));
        uint64_t* dH = (uint64_t*)c.alloc((size_t)n * 8);
        uint32_t* dO = (uint32_t*)c.alloc((size_t)n * 4);
        void* work = c.alloc(replayDeviceBytes((uint64_t)n, levels.back().first));
        RSQ_HIP(hipMemcpy(dH, hashes, (size_t)n * 8, hipMemcpyHostToDevice));
        replayEmissionOrderDevice(c, dH, (uint64_t)n, levels, work, dO);
        RSQ_HIP(hipStreamSynchronize(c.stream));
        RSQ_HIP(hipMemcpy(out, dO, (size_t)n * 4, hipMemcpyDeviceToHost));
        c.free(dH); c.free(dO); c.free(work);
    });
}

// ---- device primitives exposed for tests ----
int rsq_prim_exclusive_scan(rsq_ctx* ctx, const uint32_t* counts, int64_t n, int32_t form, uint64_t* offsets, uint32_t* notes) {
    if (!ctx || !notes || n < 0 || (n > 0 && (!counts || !offsets)) || (form != 0 && form != 1)) return RSQ_ERR_INVALID;
    *notes = 0;
    return guarded(C(ctx), [&] {
        Context& c = primContext(ctx);
        if (n == 0) return;
        const uint32_t before = primErrWord(c);
        PrimBuffers b(c);
        uint32_t* dCnt = b.take<uint32_t>((size_t)n);
        uint64_t* dOff = b.take<uint64_t>((size_t)n);
        const size_t tempBytes = scanTempBytes(n);
        void* temp = b.take<char>(tempBytes);
        RSQ_HIP(hipMemcpyAsync(dCnt, counts, (size_t)n * 4, hipMemcpyHostToDevice, c.stream));
        if (form == 1) exclusiveScanCountsChained(c, dCnt, dOff, n, temp, tempBytes);
        else exclusiveScanCounts(c, dCnt, dOff, n, temp, tempBytes);
        RSQ_HIP(hipMemcpyAsync(offsets, dOff, (size_t)n * 8, hipMemcpyDeviceToHost, c.stream));
        primSync(c);
        primNotes(c, before, notes);
    });
}

int rsq_prim_rank_index(rsq_ctx* ctx, uint32_t* blocks, int64_t n_blocks, int32_t form, uint32_t* chunk_base, uint32_t* notes) {
    if (!ctx || !notes || !chunk_base || n_blocks < 0 || (n_blocks > 0 && !blocks) || (form != 0 && form != 1)) return RSQ_ERR_INVALID;
    *notes = 0;
    return guarded(C(ctx), [&] {
        Context& c = primContext(ctx);
        if (n_blocks > kPrimMaxRankBlocks) failUnsupported("a key bitmap of more than 2^28 bits");
        if (n_blocks == 0) { chunk_base[0] = 0; return; }
        const uint32_t before = primErrWord(c);
        const size_t nChunks = (size_t)((n_blocks + RSQ_RANK_CHUNK_BLOCKS - 1) / RSQ_RANK_CHUNK_BLOCKS);
        PrimBuffers b(c);
        uint32_t* dBm = b.take<uint32_t>((size_t)n_blocks * 8);
        uint32_t* dTotal = b.take<uint32_t>(nChunks);
        uint32_t* dBase = b.take<uint32_t>(nChunks + 1);
        RSQ_HIP(hipMemcpyAsync(dBm, blocks, (size_t)n_blocks * 32, hipMemcpyHostToDevice, c.stream));
        if (form == 1) {
            RSQ_HIP(hipMemsetAsync(dTotal, 0, nChunks * 4, c.stream));          // the chain words: zero before the launch
            rankTableIndexChained(c, dBm, n_blocks, dTotal, dBase);
        } else rankTableIndex(c, dBm, n_blocks, dTotal, dBase);
        RSQ_HIP(hipMemcpyAsync(blocks, dBm, (size_t)n_blocks * 32, hipMemcpyDeviceToHost, c.stream));
        RSQ_HIP(hipMemcpyAsync(chunk_base, dBase, (nChunks + 1) * 4, hipMemcpyDeviceToHost, c.stream));
        primSync(c);
        primNotes(c, before, notes);
    });
}

int rsq_prim_rank_place(rsq_ctx* ctx, const uint32_t* blocks, int64_t n_blocks, int64_t bm_min, int64_t bm_bits, const int64_t* records,
                        const uint32_t* used, int32_t n_waves, int32_t region, int32_t n_words, int64_t capacity, int64_t* words_out,
                        uint32_t* notes) {
    if (!ctx || !notes || !blocks || !records || !used || !words_out) return RSQ_ERR_INVALID;
    *notes = 0;
    // (the kernels trust these: a block index comes from bm_bits, a record address from used[] and region)
    if (n_blocks < 1 || n_blocks > kPrimMaxRankBlocks || bm_bits < 1 || bm_bits > n_blocks * 224 || n_waves < 1 || n_waves > (1 << 20) || region < 1 ||
        n_words < 1 || n_words > 64 || capacity < 1 || capacity > ((int64_t)1 << 31))
        return RSQ_ERR_INVALID;
    uint64_t nRecords = 0;
    for (int32_t w = 0; w < n_waves; w++) { if (used[w] > (uint32_t)region) return RSQ_ERR_INVALID; nRecords += used[w]; }
    if (nRecords > 0xffffffffull) return RSQ_ERR_INVALID;
    return guarded(C(ctx), [&] {
        Context& c = primContext(ctx);
        const uint32_t before = primErrWord(c);
        const size_t nChunks = (size_t)((n_blocks + RSQ_RANK_CHUNK_BLOCKS - 1) / RSQ_RANK_CHUNK_BLOCKS);
        const size_t recWords = (size_t)n_waves * (size_t)region * (size_t)n_words, outWords = (size_t)capacity * (size_t)n_words;
        PrimBuffers b(c);
        uint32_t* dBm = b.take<uint32_t>((size_t)n_blocks * 8);
        uint32_t* dTotal = b.take<uint32_t>(nChunks);
        uint32_t* dBase = b.take<uint32_t>(nChunks + 1);
        int64_t* dRec = b.take<int64_t>(recWords);
        uint32_t* dUsed = b.take<uint32_t>((size_t)n_waves);
        uint32_t* dCount = b.take<uint32_t>(1);
        int64_t* dWords = b.take<int64_t>(outWords);
        const uint32_t count = (uint32_t)nRecords;
        RSQ_HIP(hipMemcpyAsync(dBm, blocks, (size_t)n_blocks * 32, hipMemcpyHostToDevice, c.stream));
        RSQ_HIP(hipMemcpyAsync(dRec, records, recWords * 8, hipMemcpyHostToDevice, c.stream));
        RSQ_HIP(hipMemcpyAsync(dUsed, used, (size_t)n_waves * 4, hipMemcpyHostToDevice, c.stream));
        RSQ_HIP(hipMemcpyAsync(dCount, &count, 4, hipMemcpyHostToDevice, c.stream));
        RSQ_HIP(hipMemsetAsync(dWords, 0xff, outWords * 8, c.stream));
        rankTableIndex(c, dBm, n_blocks, dTotal, dBase);
        rankTablePlace(c, dRec, dUsed, (uint32_t)n_waves, (uint32_t)region, dCount, n_words, dBm, bm_min, bm_bits, dBase, n_blocks, dWords, capacity);
        RSQ_HIP(hipMemcpyAsync(words_out, dWords, outWords * 8, hipMemcpyDeviceToHost, c.stream));
        primSync(c);
        primNotes(c, before, notes);
    });
}

int rsq_prim_radix_sort_pairs(rsq_ctx* ctx, const uint64_t* keys, const uint32_t* vals, int64_t n, int32_t key_bits, uint64_t* keys_out,
                              uint32_t* vals_out, uint32_t* notes) {
    if (!ctx || !notes || n < 0 || n > kPrimMaxItems || (n > 0 && (!keys || !vals || !keys_out || !vals_out)) || key_bits < 1 || key_bits > 64)
        return RSQ_ERR_INVALID;
    *notes = 0;
    return guarded(C(ctx), [&] {
        Context& c = primContext(ctx);
        if (n == 0) return;
        const uint32_t before = primErrWord(c);
        PrimBuffers b(c);
        uint64_t* dKeys[2] = {b.take<uint64_t>((size_t)n), b.take<uint64_t>((size_t)n)};
        uint32_t* dVals[2] = {b.take<uint32_t>((size_t)n), b.take<uint32_t>((size_t)n)};
        const size_t tempBytes = radixSortTempBytes(n);
        void* temp = b.take<char>(tempBytes);
        RSQ_HIP(hipMemcpyAsync(dKeys[0], keys, (size_t)n * 8, hipMemcpyHostToDevice, c.stream));
        RSQ_HIP(hipMemcpyAsync(dVals[0], vals, (size_t)n * 4, hipMemcpyHostToDevice, c.stream));
        // (n <= 1: nothing runs and the A buffers, the input, are the answer)
        const int in = radixSortPairs(c, dKeys[0], dVals[0], dKeys[1], dVals[1], n, key_bits, temp, tempBytes) ? 1 : 0;
        RSQ_HIP(hipMemcpyAsync(keys_out, dKeys[in], (size_t)n * 8, hipMemcpyDeviceToHost, c.stream));
        RSQ_HIP(hipMemcpyAsync(vals_out, dVals[in], (size_t)n * 4, hipMemcpyDeviceToHost, c.stream));
        primSync(c);
        primNotes(c, before, notes);
    });
}

int rsq_prim_running_min(rsq_ctx* ctx, const int64_t* in, int64_t n, int64_t* out, uint32_t* notes) {
    if (!ctx || !notes || n < 0 || n > kPrimMaxItems || (n > 0 && (!in || !out))) return RSQ_ERR_INVALID;
    *notes = 0;
    return guarded(C(ctx), [&] {
        Context& c = primContext(ctx);
        if (n == 0) return;
        const uint32_t before = primErrWord(c);
        PrimBuffers b(c);
        int64_t* dV = b.take<int64_t>((size_t)n);
        int64_t* dChunkMin = b.take<int64_t>(runningMinTempBytes(n) / 8);
        RSQ_HIP(hipMemcpyAsync(dV, in, (size_t)n * 8, hipMemcpyHostToDevice, c.stream));
        runningMinInPlace(c, dV, n, dChunkMin);
        RSQ_HIP(hipGetLastError());
        RSQ_HIP(hipMemcpyAsync(out, dV, (size_t)n * 8, hipMemcpyDeviceToHost, c.stream));
        primSync(c);
        primNotes(c, before, notes);
    });
}

int rsq_prim_merge_group_rows(rsq_ctx* ctx, const int64_t* rows, int64_t n, int32_t stride, int32_t n_tab, const int32_t* key_word,
                              const int32_t* key_type, const int32_t* key_len, int32_t n_keys, const int32_t* acc_word, const int32_t* acc_kind,
                              int32_t n_acc, int64_t* out_rows, uint64_t* out_count, uint32_t* notes) {
    if (!ctx || !notes || !out_count || n < 0 || (n > 0 && (!rows || !out_rows))) return RSQ_ERR_INVALID;
    *notes = 0;
    // (the kernels trust the spec: a key's words and an accumulator's word are row offsets)
    if (n >= ((int64_t)1 << 31) || stride < 1 || stride > kPrimMaxStride || n_tab < 0 || n_tab > stride - 1 || n_keys < 0 || n_keys > 16 || n_acc < 0 ||
        n_acc > 32 || (n_keys > 0 && (!key_word || !key_type || !key_len)) || (n_acc > 0 && (!acc_word || !acc_kind)))
        return RSQ_ERR_INVALID;
    GroupMergeSpec spec{};
    spec.stride = stride; spec.nTab = n_tab; spec.nAcc = n_acc;
    spec.keys.n = n_keys;
    for (int32_t k = 0; k < n_keys; k++) {
        const int32_t t = key_type[k], len = key_len[k];
        if (t != RSQ_VARCHAR && t != RSQ_CHAR && t != RSQ_BOOL && t != RSQ_INT && t != RSQ_BIGINT && t != RSQ_DECIMAL && t != RSQ_DATE) return RSQ_ERR_INVALID;
        const bool string = t == RSQ_VARCHAR || t == RSQ_CHAR;
        if (len < 0 || (string && len < 1) || (!string && len > 1)) return RSQ_ERR_INVALID;
        const int64_t words = len > 1 ? ((int64_t)len + 7) / 8 : 1;          // (len <= 1: one word, compared by the type's rule)
        if (key_word[k] < 1 || (int64_t)key_word[k] + words - 1 > n_tab) return RSQ_ERR_INVALID;
        spec.keys.k[k] = RowTailKey{key_word[k], t, len, 0};
    }
    for (int32_t w = 0; w < n_acc; w++) {
        if (acc_word[w] < n_tab + 1 || acc_word[w] > stride - 1 || (acc_kind[w] != 0 && acc_kind[w] != 2 && acc_kind[w] != 3)) return RSQ_ERR_INVALID;
        spec.accWord[w] = acc_word[w]; spec.accKind[w] = acc_kind[w];
    }
    return guarded(C(ctx), [&] {
        Context& c = primContext(ctx);
        const uint32_t before = primErrWord(c);
        const size_t words = (size_t)n * (size_t)stride;
        PrimBuffers b(c);
        int64_t* dRows = b.take<int64_t>(words);
        int64_t* dOut = b.take<int64_t>(words);
        void* temp = b.take<char>(groupMergeTempBytes(n));
        uint64_t* dCount = b.take<uint64_t>(1);
        if (words) RSQ_HIP(hipMemcpyAsync(dRows, rows, words * 8, hipMemcpyHostToDevice, c.stream));
        if (words) RSQ_HIP(hipMemsetAsync(dOut, 0xff, words * 8, c.stream));
        mergeGroupRows(c, dRows, n, spec, temp, dOut, dCount);
        if (words) RSQ_HIP(hipMemcpyAsync(out_rows, dOut, words * 8, hipMemcpyDeviceToHost, c.stream));
        RSQ_HIP(hipMemcpyAsync(out_count, dCount, 8, hipMemcpyDeviceToHost, c.stream));
        primSync(c);
        primNotes(c, before, notes);
    });
}

int rsq_prim_topk_select(rsq_ctx* ctx, const int64_t* rows, int64_t n_rows, int64_t rows_upper_bound, int32_t stride, int32_t key_word, int32_t is32,
                         int32_t desc, int64_t want, int32_t form, const uint64_t* image_range, int64_t capacity, int64_t* cand_out,
                         uint32_t* cand_count, uint32_t* notes) {
    if (!ctx || !notes || !cand_out || !cand_count || n_rows < 0 || (n_rows > 0 && !rows)) return RSQ_ERR_INVALID;
    *notes = 0;
    // (the kernels trust these: a row address comes from stride and key_word, a candidate address from capacity; row indices are 32 bits)
    if (n_rows > kPrimMaxItems || rows_upper_bound < 0 || rows_upper_bound > kPrimMaxItems || stride < 1 || stride > 64 || key_word < 0 ||
        key_word >= stride || want < 1 || want > 0xffffffffll || capacity < 1 || capacity > kPrimMaxItems || (form != 0 && form != 1) ||
        (form == 1 && !image_range))
        return RSQ_ERR_INVALID;
    return guarded(C(ctx), [&] {
        Context& c = primContext(ctx);
        const uint32_t before = primErrWord(c);
        const size_t rowWords = (size_t)n_rows * (size_t)stride, candWords = (size_t)capacity * (size_t)stride;
        PrimBuffers b(c);
        int64_t* dRows = b.take<int64_t>(rowWords);
        uint32_t* dN = b.take<uint32_t>(1);
        uint64_t* dImages = b.take<uint64_t>((size_t)std::min<int64_t>(n_rows, rows_upper_bound));      // (the kernels take min(*nRows, bound) rows)
        char* scratch = b.take<char>(topkHistBytes());
        int64_t* dCand = b.take<int64_t>(candWords);
        const uint32_t n32 = (uint32_t)n_rows;
        if (rowWords) RSQ_HIP(hipMemcpyAsync(dRows, rows, rowWords * 8, hipMemcpyHostToDevice, c.stream));
        RSQ_HIP(hipMemcpyAsync(dN, &n32, 4, hipMemcpyHostToDevice, c.stream));
        RSQ_HIP(hipMemsetAsync(dCand, 0xff, candWords * 8, c.stream));
        if (form == 1) {
            prepareTopCandidatesRange(c, scratch);
            RSQ_HIP(hipMemcpyAsync(scratch, image_range, 16, hipMemcpyHostToDevice, c.stream));
            selectTopCandidatesRange(c, dRows, stride, key_word, is32 != 0, desc != 0, dN, (uint32_t)rows_upper_bound, (uint32_t)want, scratch, dCand,
                                     (uint32_t)capacity);
        } else
            selectTopCandidates(c, dRows, stride, key_word, is32 != 0, desc != 0, dN, (uint32_t)rows_upper_bound, (uint32_t)want, dImages, scratch, dCand,
                                (uint32_t)capacity);
        RSQ_HIP(hipMemcpyAsync(cand_out, dCand, candWords * 8, hipMemcpyDeviceToHost, c.stream));
        RSQ_HIP(hipMemcpyAsync(cand_count, scratch + 16, 4, hipMemcpyDeviceToHost, c.stream));
        primSync(c);
        primNotes(c, before, notes);
    });
}

int rsq_prim_column_topk(rsq_ctx* ctx, const void* key, int32_t key_width, int64_t n, int32_t desc, int64_t want, int64_t capacity, const void* payload,
                         int32_t payload_width, uint32_t* positions_out, void* payload_out, uint64_t* cand_count, uint64_t* threshold_image, uint32_t* notes) {
    if (!ctx || !notes || !positions_out || !payload_out || !cand_count || !threshold_image || n < 0 || (n > 0 && (!key || !payload))) return RSQ_ERR_INVALID;
    *notes = 0;
    // (the kernels trust these: a cell's address comes from its width, a candidate's from the capacity; row numbers are 32 bits)
    if ((key_width != 4 && key_width != 8) || n > 0xffffffffll || want < 1 || want > 0xffffffffll || capacity < 1 || capacity >= kPrimMaxItems ||
        payload_width < 1 || payload_width > 4096)
        return RSQ_ERR_INVALID;
    return guarded(C(ctx), [&] {
        Context& c = primContext(ctx);
        const uint32_t before = primErrWord(c);
        struct Held {       // given back however the call ends, once the stream has drained
            Context& c; OrderLimitBuffers b;
            ~Held() { (void)hipStreamSynchronize(c.stream); b.release(c); }
        } held{c, {}};
        PrimBuffers pb(c);
        unsigned char* dKey = pb.take<unsigned char>((size_t)n * (size_t)key_width);
        unsigned char* dPayload = pb.take<unsigned char>((size_t)n * (size_t)payload_width);
        if (n) {
            RSQ_HIP(hipMemcpyAsync(dKey, key, (size_t)n * (size_t)key_width, hipMemcpyHostToDevice, c.stream));
            RSQ_HIP(hipMemcpyAsync(dPayload, payload, (size_t)n * (size_t)payload_width, hipMemcpyHostToDevice, c.stream));
        }
        held.b.ensure(c, n, capacity, {payload_width});
        OrderLimitSelection s;
        orderLimitSelect(c, held.b, dKey, key_width, desc != 0, n, (uint32_t)want, {dPayload}, true, s);
        memcpy(positions_out, s.positions, (size_t)capacity * 4);
        memcpy(payload_out, s.cols[0], (size_t)capacity * (size_t)payload_width);
        *cand_count = s.candidates; *threshold_image = s.threshold;
        primNotes(c, before, notes);
    });
}

int rsq_prim_pack_tuples(rsq_ctx* ctx, const void* const* columns, const rsq_type* types, int32_t n_cols, int64_t n_rows, void* out, int64_t out_bytes) {
    if (!ctx || !columns || !types || !out || n_cols < 1 || n_cols > (int32_t)rpack::MAX_COLUMNS || n_rows < 0 || n_rows >= kPrimMaxItems) return RSQ_ERR_INVALID;
    for (int32_t c = 0; c < n_cols; c++) if (n_rows > 0 && !columns[c]) return RSQ_ERR_INVALID;
    return guarded(C(ctx), [&] {
        Context& c = primContext(ctx);
        std::vector<Type> ty;
        for (int32_t i = 0; i < n_cols; i++) ty.push_back(Type::fromC(types[i]));
        const int64_t ts = packTupleSize(ty);
        if (!rpack::fitsDevice(n_rows, ts, INT64_MAX)) failInvalid("rsq_prim_pack_tuples: " + std::to_string((long long)n_rows) + " tuples of " + std::to_string((long long)ts) + " bytes are more than 2 GiB");
        const size_t bytes = (size_t)n_rows * (size_t)ts, guard = 64;
        if (out_bytes != (int64_t)(bytes + guard)) failInvalid("rsq_prim_pack_tuples: out_bytes is " + std::to_string((long long)out_bytes) + ", the tuples and their guard take " + std::to_string(bytes + guard));
        PrimBuffers pb(c);
        std::vector<const void*> dCols;
        for (int32_t i = 0; i < n_cols; i++) {
            const size_t b = (size_t)n_rows * (size_t)columnWidth(ty[(size_t)i]);
            unsigned char* d = pb.take<unsigned char>(b);
            if (b) RSQ_HIP(hipMemcpyAsync(d, columns[i], b, hipMemcpyHostToDevice, c.stream));
            dCols.push_back(d);
        }
        unsigned char* dOut = pb.take<unsigned char>(bytes + guard);
        RSQ_HIP(hipMemsetAsync(dOut, 0xEE, bytes + guard, c.stream));
        packTuples(c, ty, dCols.data(), n_rows, dOut);
        RSQ_HIP(hipMemcpyAsync(out, dOut, bytes + guard, hipMemcpyDeviceToHost, c.stream));
        primSync(c);
    });
}

int rsq_prim_sort_rows(rsq_ctx* ctx, const void* const* columns, const rsq_type* types, int32_t n_cols, const int32_t* key_columns, const int32_t* descending,
                       int32_t n_keys, int64_t n_rows, int64_t lead, uint32_t* perm_out, int64_t* tied_pairs, int32_t* key_bits, int32_t* words) {
    if (!ctx || !columns || !types || !key_columns || !descending || !tied_pairs || !key_bits || !words || n_cols < 1 || n_cols > (int32_t)rpack::MAX_COLUMNS ||
        n_keys < 1 || n_keys > (int32_t)osort::MAX_KEYS || n_rows < 0 || n_rows >= kPrimMaxItems || lead < 0 || lead > n_rows || (n_rows > 0 && !perm_out))
        return RSQ_ERR_INVALID;
    for (int32_t k = 0; k < n_keys; k++) if (key_columns[k] < 0 || key_columns[k] >= n_cols || (n_rows > 0 && !columns[key_columns[k]])) return RSQ_ERR_INVALID;
    return guarded(C(ctx), [&] {
        Context& c = primContext(ctx);
        std::vector<int> width;
        for (int32_t k = 0; k < n_keys; k++) {
            width.push_back(deviceOrderWidth(Type::fromC(types[key_columns[k]])));
            if (!width.back()) failInvalid("rsq_prim_sort_rows: key " + std::to_string(k) + " is not an INT, DATE, BIGINT or DECIMAL column");
        }
        *tied_pairs = 0; *words = 0;
        for (int k = 0; k < (int)osort::MAX_KEYS; k++) key_bits[k] = 0;
        if (n_rows == 0) return;
        PrimBuffers pb(c);
        std::vector<OrderSortKey> keys;
        for (int32_t k = 0; k < n_keys; k++) {          // (the key columns only: the sort reads no other)
            const size_t b = (size_t)n_rows * (size_t)width[(size_t)k];
            unsigned char* d = pb.take<unsigned char>(b);
            RSQ_HIP(hipMemcpyAsync(d, columns[key_columns[k]], b, hipMemcpyHostToDevice, c.stream));
            keys.push_back(OrderSortKey{d, width[(size_t)k], descending[k] != 0});
        }
        OrderSortBuffers b;
        struct Release { Context& c; OrderSortBuffers& b; ~Release() { (void)hipStreamSynchronize(c.stream); b.release(c); } } release{c, b};
        b.ensure(c, n_rows);
        OrderSortOutcome o;
        orderSortRows(c, b, keys.data(), n_keys, n_rows, lead, o);
        for (int32_t k = 0; k < n_keys; k++) key_bits[k] = o.bits[k];
        *words = o.words;
        if (!o.sorted) {
            for (int64_t i = 0; i < n_rows; i++) perm_out[i] = (uint32_t)i;
            *tied_pairs = o.tiedPairs;
            primSync(c);
            return;
        }
        uint32_t ties = 0;
        RSQ_HIP(hipMemcpyAsync(perm_out, o.dPerm, (size_t)n_rows * 4, hipMemcpyDeviceToHost, c.stream));
        if (lead > 1) RSQ_HIP(hipMemcpyAsync(&ties, o.dTies, 4, hipMemcpyDeviceToHost, c.stream));
        primSync(c);
        *tied_pairs = ties;
    });
}

int rsq_prim_gather_tuples(rsq_ctx* ctx, const void* tuples, int32_t tuple_size, int64_t n_rows, const uint32_t* perm, int64_t n_out, void* out, int64_t out_bytes) {
    if (!ctx || !out || tuple_size < 1 || n_rows < 0 || n_rows >= kPrimMaxItems || n_out < 0 || n_out > n_rows || (n_rows > 0 && !tuples) || (n_out > 0 && !perm)) return RSQ_ERR_INVALID;
    for (int64_t i = 0; i < n_out; i++) if ((int64_t)perm[i] >= n_rows) return RSQ_ERR_INVALID;          // (the kernel trusts the permutation)
    return guarded(C(ctx), [&] {
        Context& c = primContext(ctx);
        if (!rpack::fitsDevice(n_rows, tuple_size, INT64_MAX)) failInvalid("rsq_prim_gather_tuples: " + std::to_string((long long)n_rows) + " tuples of " + std::to_string(tuple_size) + " bytes are more than 2 GiB");
        const size_t inBytes = (size_t)n_rows * (size_t)tuple_size, bytes = (size_t)n_out * (size_t)tuple_size, guard = 64;
        if (out_bytes != (int64_t)(bytes + guard)) failInvalid("rsq_prim_gather_tuples: out_bytes is " + std::to_string((long long)out_bytes) + ", the tuples and their guard take " + std::to_string(bytes + guard));
        PrimBuffers pb(c);
        unsigned char* dIn = pb.take<unsigned char>(inBytes);
        uint32_t* dPerm = pb.take<uint32_t>((size_t)n_out);
        unsigned char* dOut = pb.take<unsigned char>(bytes + guard);
        if (inBytes) RSQ_HIP(hipMemcpyAsync(dIn, tuples, inBytes, hipMemcpyHostToDevice, c.stream));
        if (n_out) RSQ_HIP(hipMemcpyAsync(dPerm, perm, (size_t)n_out * 4, hipMemcpyHostToDevice, c.stream));
        RSQ_HIP(hipMemsetAsync(dOut, 0xEE, bytes + guard, c.stream));
        gatherTuples(c, dIn, dOut, dPerm, tuple_size, n_out);
        RSQ_HIP(hipMemcpyAsync(out, dOut, bytes + guard, hipMemcpyDeviceToHost, c.stream));
        primSync(c);
    });
}

int rsq_ref_emission_order(const uint64_t* hashes, int64_t n, uint64_t min_size, int32_t parallel, uint32_t* out) {
    if (n < 0 || (n > 0 && (!hashes || !out))) return RSQ_ERR_INVALID;
    try {
        if (parallel) {
            std::vector<uint32_t> order; ReplayScratch scratch;
            refEmissionOrderParallel(hashes, (size_t)n, min_size, order, scratch);
            for (int64_t i = 0; i < n; i++) out[i] = order[(size_t)i];
        } else {
            std::vector<size_t> order = refEmissionOrder(std::vector<uint64_t>(hashes, hashes + n), min_size);
            for (int64_t i = 0; i < n; i++) out[i] = (uint32_t)order[(size_t)i];
        }
        return RSQ_OK;
    } catch (const Error& e) { return e.status; }
    catch (const std::exception&) { return RSQ_ERR_RUNTIME; }
}

// ---- SQL front end (sqlfront.cpp) ----
struct rsq_sql_plan { rsq::ExprPool pool; rsq::sql::Statement st; rsq::sql::PlanDesc plan; std::vector<Table*> db; };

int rsq_sql_plan_select(rsq_ctx* ctx, const char* sqlText, rsq_table* const* tables, int32_t n_tables, rsq_sql_plan** out) {
    if (!ctx || !sqlText || !out || n_tables < 0) return RSQ_ERR_INVALID;
    *out = nullptr;
    return guarded(C(ctx), [&] {
        std::unique_ptr<rsq_sql_plan> p(new rsq_sql_plan());
        std::vector<Table*> db;
        for (int i = 0; i < n_tables; i++) { if (!tables[i]) failInvalid("null table"); db.push_back(T(tables[i])); }
        rsq::sql::parse(sqlText, p->pool, p->st);
        if (p->st.kind != rsq::sql::Statement::SELECT) failInvalid("not a select statement");
        rsq::sql::planSelect(p->st, p->pool, db, p->plan, (C(ctx)->cfg.engine_flags & RSQ_ENGINE_NESTED_LOOPS) != 0);
        p->db = db;
        *out = p.release();
    });
}
const rsq_plan_desc* rsq_sql_plan_desc(const rsq_sql_plan* plan) { return plan ? &plan->plan.desc : nullptr; }
void rsq_sql_plan_destroy(rsq_sql_plan* plan) { delete plan; }
char* rsq_sql_plan_text(const rsq_sql_plan* plan) {
    if (!plan) return nullptr;
    try { return strdup(rsq::sql::dumpPlan(plan->plan.desc, plan->db).c_str()); }
    catch (const std::exception& e) { return strdup((std::string("error: ") + e.what()).c_str()); }
    catch (...) { return nullptr; }
}

int rsq_sql_compile(rsq_ctx* ctx, const char* sqlText, rsq_table* const* tables, int32_t n_tables, rsq_query** out) {
    if (!out) return RSQ_ERR_INVALID;
    *out = nullptr;
    rsq_sql_plan* p = nullptr;
    int st = rsq_sql_plan_select(ctx, sqlText, tables, n_tables, &p);
    if (st != RSQ_OK) return st;
    st = rsq_query_compile(ctx, &p->plan.desc, tables, n_tables, out);
    delete p;
    return st;
}

// ---- statement loop (executeStatement, execute.h:508-545) ----
struct rsq_db {
    Context* ctx = nullptr;
    std::map<std::string, std::vector<std::pair<std::string, Type>>> schemas;      // CREATE TABLE
    std::map<std::string, Table*> tables;                                          // name order = the planner's table order
    rsq_query* last = nullptr;
    rsq_report lastReport{};
    rsq_tbl_load_report lastLoad{};          // of the last BULK INSERT
    rsq_result_text_report lastText{};       // of the last SELECT that `tofile` wrote
    rsq_order_limit_report lastOrderLimit{}; // of the last SELECT
    rsq_result_pack_report lastResultPack{}; // of the last SELECT
    rsq_order_sort_report lastOrderSort{};   // of the last SELECT
    // DBConfig / JitConfig as the control variables set them (execute.h:23-27, JitContextFlounder.h:86-109)
    bool showPlan = false, writeResultsToFile = false;
    uint16_t numThreads = 1;
    bool printPerformance = false, printAssembly = false, printFlounder = false, optimizeFlounder = false, emitMachineCode = false;
    std::string message;          // what the reference's printQueryResult would print in front of the relation (execute.h:173-200)
};

}  // extern "C"

namespace {

// rsq_db_<what>_report: the report the statement loop kept (no message: RSQ_ERR_INVALID alone)
template <typename R>
int dbReportOut(const rsq_db* db, R rsq_db::* last, R* out) { return db && out && copyReportOut(db->*last, out) ? RSQ_OK : RSQ_ERR_INVALID; }

// setBoolVar / setIntVar (execute.h:407-451): spaces are removed from the line, the variable name may stand anywhere in it
// (rfind), the line is either the bare name (prints the value) or name=value
bool controlVar(std::string cmd, const std::string& name, std::string& value, bool& bare) {
    cmd.erase(std::remove(cmd.begin(), cmd.end(), ' '), cmd.end());
    if (cmd.rfind(name) == std::string::npos) return false;
    bare = cmd.length() == name.length();
    if (bare) return true;
    if (cmd.at(name.length()) != '=') failInvalid("Expected varname=value");
    value = cmd.substr(name.length() + 1);
    return true;
}
void boolVar(const std::string& line, const char* name, bool& var, bool& done, std::string& out) {
    std::string v; bool bare = false;
    if (!controlVar(line, name, v, bare)) return;
    done = true;
    if (bare) { out += var ? "true\n" : "false\n"; return; }
    if (v == "true") var = true;
    else if (v == "false") var = false;
    else failInvalid("Expected true or false");
}
void intVar(const std::string& line, const char* name, uint16_t& var, bool& done, std::string& out) {
    std::string v; bool bare = false;
    if (!controlVar(line, name, v, bare)) return;
    done = true;
    if (bare) { out += std::to_string(var) + "\n"; return; }
    // std::stoi semantics (leading blanks, sign, digits; trailing characters ignored) without its exceptions: the reference lets
    // std::invalid_argument escape executeStatement (it catches runtime_error and ResqlError only) and dies
    size_t i = 0;
    bool neg = false;
    if (i < v.size() && (v[i] == '+' || v[i] == '-')) neg = v[i++] == '-';
    if (i >= v.size() || !isdigit((unsigned char)v[i])) failInvalid("Expected an integer value");
    long long x = 0;
    for (; i < v.size() && isdigit((unsigned char)v[i]); i++) { x = x * 10 + (v[i] - '0'); if (x > 0x7fffffffLL) failInvalid("Integer value out of range"); }
    var = (uint16_t)(int)(neg ? -x : x);
}

// printStringTable (dbdata.h:578-626): cells are right-aligned in columns two wider than their longest string
std::string stringTable(const std::vector<std::string>& cells, int nCols, int headerRows, const std::string& subTitle) {
    std::vector<size_t> w((size_t)nCols, 0);
    for (size_t i = 0; i < cells.size(); i++) w[i % (size_t)nCols] = std::max(w[i % (size_t)nCols], cells[i].size() + 2);
    auto rule = [&](const char* l, const char* m, const char* x, const char* r) {
        std::string o = l;
        for (int c = 0; c < nCols; c++) { if (c) o += x; for (size_t k = 0; k < w[(size_t)c]; k++) o += m; }
        return o + r + "\n";
    };
    auto row = [&](size_t at) {
        std::string o;
        for (int c = 0; c < nCols; c++) {
            std::string cell = " " + cells[at + (size_t)c] + " ";
            o += "\xe2\x94\x82" + std::string(w[(size_t)c] > cell.size() ? w[(size_t)c] - cell.size() : 0, ' ') + cell;
        }
        return o + "\xe2\x94\x82\n";
    };
    std::string out = rule("\xe2\x94\x8c", "\xe2\x94\x80", "\xe2\x94\xac", "\xe2\x94\x90");
    size_t at = 0;
    for (int h = 0; h < headerRows; h++, at += (size_t)nCols) out += row(at);
    out += rule("\xe2\x94\x9c", "\xe2\x94\x80", "\xe2\x94\xbc", "\xe2\x94\xa4");
    for (; at < cells.size(); at += (size_t)nCols) out += row(at);
    out += rule("\xe2\x94\x94", "\xe2\x94\x80", "\xe2\x94\xb4", "\xe2\x94\x98");
    if (!subTitle.empty()) {
        size_t width = (size_t)nCols;
        for (size_t x : w) width += x;
        out += std::string(width > subTitle.size() ? width - subTitle.size() : 0, ' ') + subTitle + "\n";
    }
    return out;
}

// processControl (execute.h:454-474): every variable is tried in the reference's order; "tables" must be the whole line
bool processControl(rsq_db& db, const std::string& line, std::string& out) {
    bool done = false;
    boolVar(line, "showplan", db.showPlan, done, out);
    boolVar(line, "tofile", db.writeResultsToFile, done, out);
    intVar(line, "threads", db.numThreads, done, out);
    boolVar(line, "showperf", db.printPerformance, done, out);
    boolVar(line, "showasm", db.printAssembly, done, out);
    boolVar(line, "showfln", db.printFlounder, done, out);
    boolVar(line, "optimize", db.optimizeFlounder, done, out);
    boolVar(line, "emitmc", db.emitMachineCode, done, out);
    if (line == "tables") {          // showTables (execute.h:390-404); std::map order = by name
        std::vector<std::string> cells = {"Table name", "Number of attributes", "Number of tuples"};
        for (auto& t : db.tables) { cells.push_back(t.first); cells.push_back(std::to_string(t.second->cols.size())); cells.push_back(std::to_string(t.second->nRows)); }
        out += stringTable(cells, 3, 1, std::to_string(db.tables.size()) + " tables");
        done = true;
    }
    return done;
}

// showReport (JitContextFlounder.h:132-150) for this engine: the code (HIP source for showasm, the pipeline description for
// showfln), then the performance lines in the reference's format plus the device-side figures
std::string reportText(const rsq_db& db, rsq_query* q, const rsq_report& r) {
    std::string o;
    if (db.printFlounder) { o += rsq_query_explain(q); }
    if (db.printAssembly) { o += rsq_query_source(q); }
    if (db.printPerformance) {
        char b[256];
        snprintf(b, sizeof b, "Launched %llu kernels (%d compiled by hiprtc, %d from the code-object cache). \n", (unsigned long long)r.num_kernels, r.jit_compiles, r.jit_cache_hits);
        o += b;
        snprintf(b, sizeof b, "compile: %.3f ms\n", r.compilation_time_ms); o += b;
        snprintf(b, sizeof b, "execute: %.3f ms\n", r.execution_time_ms); o += b;
        snprintf(b, sizeof b, "device:  %.3f ms, %llu bytes scanned, %.1f GB/s\n", r.kernel_time_ms, (unsigned long long)r.bytes_read, r.hbm_gbps); o += b;
        if (q) o += rowCellsLine(*QH(q)->q);
    }
    return o;
}

// concatenate `more` behind `t` (BULK INSERT appends, execute.h:332-388): new device columns, statistics recomputed
void appendTable(Context& ctx, Table& t, Table& more) {
    if (t.cols.size() != more.cols.size()) failInvalid("append: different schemas");
    for (size_t c = 0; c < t.cols.size(); c++)
        if (t.cols[c].type.tag != more.cols[c].type.tag || columnWidth(t.cols[c].type) != columnWidth(more.cols[c].type)) failInvalid("append: column " + t.cols[c].name + " has another type");
    const int64_t n0 = t.nRows, n1 = more.nRows;
    for (size_t c = 0; c < t.cols.size(); c++) {
        TableColumn& a = t.cols[c]; TableColumn& b = more.cols[c];
        const size_t w = (size_t)columnWidth(a.type);
        if (ctx.device >= 0) {
            char* nu = (char*)ctx.allocRaw((size_t)(n0 + n1) * w);
            if (n0 && a.dptr) RSQ_HIP(hipMemcpy(nu, a.dptr, (size_t)n0 * w, hipMemcpyDeviceToDevice));
            if (n1 && b.dptr) RSQ_HIP(hipMemcpy(nu + (size_t)n0 * w, b.dptr, (size_t)n1 * w, hipMemcpyDeviceToDevice));
            if (a.owned && a.dptr) ctx.freeRaw(a.dptr);
            a.dptr = nu; a.owned = true;
        } else {
            char* nu = (char*)malloc(std::max<size_t>(1, (size_t)(n0 + n1) * w));
            if (!nu) throw std::bad_alloc();
            if (n0 && a.dptr) memcpy(nu, a.dptr, (size_t)n0 * w);
            if (n1 && b.dptr) memcpy(nu + (size_t)n0 * w, b.dptr, (size_t)n1 * w);
            if (a.owned && a.dptr) ::free(a.dptr);
            a.dptr = nu; a.owned = true;
        }
    }
    t.nRows = n0 + n1;
    t.layoutVersion++;
    t.bumpVersion();
    computeColumnStats(ctx, t);
}

}  // namespace

extern "C" {

int rsq_table_append(rsq_table* t, rsq_table* more) {
    if (!t || !more || t == more) return RSQ_ERR_INVALID;
    Table& a = *T(t); Table& b = *T(more);
    if (!a.ctx || a.ctx != b.ctx) return RSQ_ERR_INVALID;
    return guarded(a.ctx, [&] {
        if (!a.ownStats.empty() || a.nRowsTotal >= 0) failInvalid("rsq_table_append: the table is a shard that plans with unified statistics");
        appendTable(*a.ctx, a, b);
        delete &b;
    });
}

int rsq_db_create(rsq_ctx* ctx, rsq_db** out) {
    if (!ctx || !out) return RSQ_ERR_INVALID;
    *out = new rsq_db();
    (*out)->ctx = C(ctx);
    return RSQ_OK;
}

void rsq_db_destroy(rsq_db* db) {
    if (!db) return;
    if (db->last) rsq_query_destroy(db->last);
    for (auto& t : db->tables) delete t.second;
    delete db;
}

int rsq_db_adopt_table(rsq_db* db, rsq_table* table) {
    if (!db || !table) return RSQ_ERR_INVALID;
    return guarded(db->ctx, [&] {
        Table* t = T(table);
        if (db->tables.count(t->name) || db->schemas.count(t->name)) failInvalid("Table " + t->name + " already exists.");
        std::vector<std::pair<std::string, Type>> sch;
        for (auto& c : t->cols) sch.emplace_back(c.name, c.type);
        db->schemas[t->name] = sch;
        db->tables[t->name] = t;
    });
}

int rsq_db_report(const rsq_db* db, rsq_report* out) {
    if (!db || !out) return RSQ_ERR_INVALID;
    *out = db->lastReport;
    return RSQ_OK;
}

int rsq_db_load_report(const rsq_db* db, rsq_tbl_load_report* out) { return dbReportOut(db, &rsq_db::lastLoad, out); }
int rsq_db_result_text_report(const rsq_db* db, rsq_result_text_report* out) { return dbReportOut(db, &rsq_db::lastText, out); }
int rsq_db_order_limit_report(const rsq_db* db, rsq_order_limit_report* out) { return dbReportOut(db, &rsq_db::lastOrderLimit, out); }
int rsq_db_result_pack_report(const rsq_db* db, rsq_result_pack_report* out) { return dbReportOut(db, &rsq_db::lastResultPack, out); }
int rsq_db_order_sort_report(const rsq_db* db, rsq_order_sort_report* out) { return dbReportOut(db, &rsq_db::lastOrderSort, out); }

const char* rsq_db_message(const rsq_db* db) { return db ? db->message.c_str() : ""; }

int rsq_db_execute(rsq_db* db, const char* sqlText, int32_t* kind, rsq_result_view* result) {
    if (!db || !sqlText) return RSQ_ERR_INVALID;
    if (kind) *kind = 0;
    db->message.clear();
    rsq_ctx* cx = reinterpret_cast<rsq_ctx*>(db->ctx);
    int selectStatus = RSQ_OK;
    bool isSelect = false;
    int st = guarded(db->ctx, [&] {
        // control statements first (executeStatement, execute.h:512-516)
        std::string ctl;
        if (processControl(*db, sqlText, ctl)) { db->message = ctl; if (kind) *kind = 4; return; }
        rsq::ExprPool pool;
        rsq::sql::Statement stmt;
        rsq::sql::parse(sqlText, pool, stmt);
        if (kind) *kind = stmt.kind;
        if (stmt.kind == rsq::sql::Statement::CREATE_TABLE) {
            if (db->schemas.count(stmt.tableName)) failInvalid("Table " + stmt.tableName + " already exists.");
            if (stmt.schema.empty()) failInvalid("Create table needs at least one schema element.");
            db->schemas[stmt.tableName] = stmt.schema;
            // an empty relation that can be scanned (db.relations.try_emplace(name, schema), execute.h:279)
            static const uint8_t kEmpty[16] = {0};       // columns WITH data, of zero rows
            std::vector<rsq_column> cols(stmt.schema.size());
            for (size_t i = 0; i < cols.size(); i++) {
                memset(&cols[i], 0, sizeof cols[i]);
                snprintf(cols[i].name, RSQ_SYMBOL_MAX, "%s", stmt.schema[i].first.c_str());
                cols[i].type = stmt.schema[i].second.toC();
                cols[i].data = kEmpty;
            }
            rsq_table_desc d;
            memset(&d, 0, sizeof d);
            snprintf(d.name, RSQ_SYMBOL_MAX, "%s", stmt.tableName.c_str());
            d.n_rows = 0; d.n_cols = (int32_t)cols.size(); d.cols = cols.data();
            db->tables[stmt.tableName] = makeTable(*db->ctx, d, false);
            db->message = "Created table " + stmt.tableName + "\n";
        } else if (stmt.kind == rsq::sql::Statement::BULK_INSERT) {
            auto it = db->schemas.find(stmt.tableName);
            if (it == db->schemas.end()) failInvalid("Table " + stmt.tableName + " does not exist.");
            if (stmt.fieldTerminator.length() > 1) failInvalid("Bulk insert only supports single-character field terminators.");
            if (stmt.fieldTerminator.empty()) failInvalid("empty field terminator");
            auto have = db->tables.find(stmt.tableName);
            std::vector<rsq_column> cols(it->second.size());
            for (size_t i = 0; i < cols.size(); i++) {
                memset(&cols[i], 0, sizeof cols[i]);
                snprintf(cols[i].name, RSQ_SYMBOL_MAX, "%s", it->second[i].first.c_str());
                cols[i].type = it->second[i].second.toC();
            }
            rsq_table_desc d;
            memset(&d, 0, sizeof d);
            snprintf(d.name, RSQ_SYMBOL_MAX, "%s", stmt.tableName.c_str());
            d.n_cols = (int32_t)cols.size(); d.cols = cols.data();
            rsq_table* t = nullptr;
            rsq_tbl_load_report loaded{};
            loaded.struct_size = (uint32_t)sizeof loaded;
            int rc = rsq_table_load_tbl_ex(cx, &d, stmt.fileName.c_str(), stmt.fieldTerminator[0], 0, nullptr, &loaded, &t);
            if (rc != RSQ_OK) throw Error(rc, db->ctx->lastError);
            db->lastLoad = loaded;
            const int64_t inserted = T(t)->nRows;
            if (have != db->tables.end() && have->second->nRows > 0) {
                // the reference appends to the relation (AppendIterator on the existing table, execute.h:348-350)
                std::unique_ptr<Table> more(T(t));
                appendTable(*db->ctx, *have->second, *more);
            } else {
                if (have != db->tables.end()) delete have->second;
                db->tables[stmt.tableName] = T(t);
            }
            db->message = "Inserted " + std::to_string(inserted) + " tuples\n";
        } else isSelect = true;
    });
    if (st != RSQ_OK || !isSelect) return st;
    // SELECT: executeSelect (execute.h:250-260)
    if (db->last) { rsq_query_destroy(db->last); db->last = nullptr; }
    std::vector<rsq_table*> arr;
    for (auto& t : db->tables) arr.push_back(reinterpret_cast<rsq_table*>(t.second));
    std::string planText;
    if (db->showPlan) {            // root->print(plan) before anything else (execute.h:217-220)
        rsq_sql_plan* p = nullptr;
        selectStatus = rsq_sql_plan_select(cx, sqlText, arr.data(), (int32_t)arr.size(), &p);
        if (selectStatus != RSQ_OK) return selectStatus;
        char* txt = rsq_sql_plan_text(p);
        if (txt) { planText = txt; free(txt); }
        rsq_sql_plan_destroy(p);
    }
    selectStatus = rsq_sql_compile(cx, sqlText, arr.data(), (int32_t)arr.size(), &db->last);
    if (selectStatus != RSQ_OK) return selectStatus;
    selectStatus = rsq_query_execute(db->last);
    if (selectStatus != RSQ_OK) return selectStatus;
    rsq_query_report(db->last, &db->lastReport);
    queryReport(*QH(db->last)->q, &db->lastOrderLimit);
    queryReport(*QH(db->last)->q, &db->lastResultPack);
    queryReport(*QH(db->last)->q, &db->lastOrderSort);
    rsq_result_view view;
    selectStatus = rsq_query_result(db->last, &view);
    if (selectStatus != RSQ_OK) return selectStatus;
    if (db->writeResultsToFile) {            // writeRelationToFile(*rel, "qres.tbl") (execute.h:203-210, 243-245)
        selectStatus = guarded(db->ctx, [&] {
            TextOut out;
            out.file = fopen("qres.tbl", "w");
            if (!out.file) failInvalid("Could not open file qres.tbl");
            writeResultText(*db->ctx, view, queryResultDeviceTuples(*QH(db->last)->q), db->ctx->resultText == 1, 0, 0, out, db->lastText);          // (the context's setting at 0: serializeResultView, as ever)
            out.closeFile();
        });
        if (selectStatus != RSQ_OK) return selectStatus;
    }
    // printQueryResult (execute.h:178-183): the plan line, then showReport
    db->message = planText + "\n" + reportText(*db, db->last, db->lastReport);
    if (result) *result = view;
    return RSQ_OK;
}

char* rsq_sql_describe(rsq_ctx* ctx, const char* sqlText, int32_t what) {
    if (!ctx || !sqlText) return nullptr;
    char* res = nullptr;
    guarded(C(ctx), [&] {
        if (what == 0) {
            bool err = false;
            std::string out;
            for (auto& t : rsq::sql::tokenize(sqlText, err)) { out += t.name; out += " "; out += t.text; out += "\n"; }
            if (err) out += "ERROR\n";
            res = strdup(out.c_str());
        } else {
            rsq::ExprPool pool;
            rsq::sql::Statement stmt;
            rsq::sql::parse(sqlText, pool, stmt);
            res = strdup(rsq::sql::dumpStatement(stmt).c_str());
        }
    });
    return res;
}

int rsq_measure_read_bandwidth(rsq_ctx* ctx, size_t bytes, int32_t iters, double* gb_per_s) {
    if (!ctx || !gb_per_s || iters <= 0) return RSQ_ERR_INVALID;
    return guarded(C(ctx), [&] { *gb_per_s = measureReadBandwidth(*C(ctx), bytes, iters); });
}

}  // extern "C"
