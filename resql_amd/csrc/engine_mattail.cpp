// engine_mattail.cpp - the device tails of a materialisation without an aggregation, each opt-in per context: the candidates of an
// ORDER BY ... LIMIT (rsq_ctx_set_order_limit, order_limit.hip), the sort of an ORDER BY (rsq_ctx_set_order_sort, order_sort.hip) and the
// pack of the result's tuples (rsq_ctx_set_result_pack, result_pack.hip).  Their reports, their buffers' lifetime and - in
// runMaterializeDeviceTail - which of them decides an execution.  Called from compileQuery, executeQuery and ~Query.
#include <algorithm>
#include <cstring>

#include "engine_internal.h"
#include "result_pack.h"
#include "order_sort.h"

namespace rsq {

void planMaterializeTails(Query& q) {
    q.orderLimit.report = q.orderLimit.plan = planOrderLimit(q);
    q.orderSort.report = q.orderSort.plan = planOrderSort(q);
    q.resultPack.plan = rsq_result_pack_report{};
    q.resultPack.plan.planned = !q.agg && q.matOp && !q.matSchema.empty() && q.matSchema.size() <= (size_t)rpack::MAX_COLUMNS;
    q.resultPack.report = q.resultPack.plan;
}

// every execution's reports begin as the plan's: the host path, under setting 1 for want of the shape until a tail below says otherwise
// (held tails, partial executions and sub-queries never reach one)
void resetMaterializeReports(Query& q) {
    const Context& ctx = q.ctx;
    q.orderLimit.report = q.orderLimit.plan;
    q.orderLimit.report.fallback_reason = ctx.orderLimit == 1 ? RSQ_ORDER_LIMIT_FALLBACK_SHAPE : RSQ_ORDER_LIMIT_FALLBACK_NONE;
    q.orderSort.report = q.orderSort.plan;
    q.orderSort.report.fallback_reason = ctx.orderSort == 1 ? RSQ_ORDER_SORT_FALLBACK_SHAPE : RSQ_ORDER_SORT_FALLBACK_NONE;
    q.resultPack.report = q.resultPack.plan;
    q.resultPack.report.fallback_reason = ctx.resultPack == 1 ? RSQ_RESULT_PACK_FALLBACK_SHAPE : RSQ_RESULT_PACK_FALLBACK_NONE;
}

void releaseMaterializeTails(Query& q) {
    Context& ctx = q.ctx;
    q.orderLimit.buffers.release(ctx);
    q.orderSort.buffers.release(ctx);
    for (uint8_t* d : {q.orderSort.dScan, q.orderSort.dOut, q.resultPack.dev}) if (d) ctx.free(d);
    for (uint8_t* p : {q.orderSort.pinned, q.resultPack.pinned}) if (p) ctx.freePinned(p);
    for (hipEvent_t e : {q.resultPack.ev0, q.resultPack.ev1}) if (e) ctx.giveEvent(e);
}

void queryReport(const Query& q, rsq_order_limit_report* out) { *out = q.orderLimit.report; }
void queryReport(const Query& q, rsq_result_pack_report* out) { *out = q.resultPack.report; }
void queryReport(const Query& q, rsq_order_sort_report* out) { *out = q.orderSort.report; }

const uint8_t* queryResultDeviceTuples(const Query& q) {
    // (the query-owned buffers only - the pack buffer, the device sort's ordered tuples: the aggregation tails' buffers are arena space
    // another statement may be handed)
    return q.resultInPinned && q.resultDev && (q.resultDev == q.resultPack.dev || q.resultDev == q.orderSort.dOut) ? q.resultDev : nullptr;
}

void resultPackHostRelation(Query& q) {
    rsq_result_pack_report& r = q.resultPack.report;
    if (!r.planned || q.holdTail) return;
    r.tuple_size = schemaTupleSize(q.resultSchema); r.rows = q.resultRows; r.tuple_bytes = r.rows * (int64_t)r.tuple_size;
}

// ---- the steps the pack and the sort share --------------------------------------------------------------------------------------
// do they take this execution at all?  (the columns stand complete in q.dMatCols, whichever tier wrote them, and somebody reads the result)
static bool takesMaterialisation(const Query& q, bool planned) {
    return planned && !q.holdTail && !q.subQuery && q.dMatCols.size() == q.matSchema.size();
}

static std::vector<Type> materialisedTypes(const Query& q) {
    std::vector<Type> types;
    for (auto& a : q.matSchema) types.push_back(a.type);
    return types;
}

// allocMatCols' form for small capacities: the host has the cells when the stream completes
static bool hostMapped(const Query& q) {
    for (void* m : q.hMatMapped) if (m) return true;
    return false;
}

// what the device has free, asked only where a buffer must grow: what the query holds already is not asked for again
static int64_t freeDeviceBytes(bool grows) {
    if (!grows) return INT64_MAX;
    size_t freeNow = 0, total = 0;
    RSQ_HIP(hipMemGetInfo(&freeNow, &total));
    return (int64_t)std::min<size_t>(freeNow, (size_t)INT64_MAX);
}

// a buffer of the context's arenas kept between executions: at least `want` bytes (`atLeast` where want may be 0)
static void growDevice(Context& ctx, uint8_t*& p, size_t& have, size_t want, size_t atLeast = 0) {
    if (p && have >= want) return;
    if (p) ctx.free(p);
    p = nullptr; have = 0;
    p = (uint8_t*)ctx.alloc(std::max(want, atLeast));
    have = want;
}

static void growPinned(Context& ctx, uint8_t*& p, size_t& have, size_t want) {
    if (p && have >= want) return;
    if (p) ctx.freePinned(p);
    p = nullptr; have = 0;
    p = (uint8_t*)ctx.allocPinned(want);
    have = want;
}

// the error word as it came back with the tuples, after the wait
static void checkErrorWord(Context& ctx, uint32_t err) {
    if (err) { ctx.errWordClean = false; checkDeviceError(err); }
}

// the result relation is `rows` tuples of the materialisation's schema in `pinned`; `dev`: the same tuples in the same order, or null
static void publishDeviceResult(Query& q, int64_t rows, uint8_t* pinned, uint8_t* dev) {
    q.tailNeedsAllGroups = false;
    q.resultSchema = q.matSchema;
    q.resultRows = rows;
    q.resultPinned = pinned;
    q.resultInPinned = true;
    q.resultDev = dev;
}

// ---- the three tails ------------------------------------------------------------------------------------------------------------
// Each: true where its result stands; false: the next one or the host path follows over q.dMatCols - they are untouched - and its report
// says why.

// ORDER BY ... LIMIT k: the device selects the candidates, only they come back, and the tail decides from them (tail.cpp runOrderLimitTail)
static bool orderLimitOnDevice(Query& q) {
    Context& ctx = q.ctx;
    rsq_order_limit_report& r = q.orderLimit.report;
    if (ctx.orderLimit != 1) return false;
    const int64_t n = q.matRows;
    if (!r.planned || q.holdTail || n >= ((int64_t)1 << 32) || q.dMatCols.size() != q.matSchema.size()) return false;
    const int64_t limit = q.root->limit, want = limit + 1;
    const int64_t capacity = std::max<int64_t>(4 * want, 65536);
    r.rows = n; r.want = want; r.capacity = capacity;
    if (4 * limit >= n) { r.fallback_reason = RSQ_ORDER_LIMIT_FALLBACK_FEW_ROWS; return false; }      // (the rule of tail.cpp runTailOn)
    std::vector<int32_t> widths;
    std::vector<const void*> src;
    for (size_t c = 0; c < q.matSchema.size(); c++) { widths.push_back(columnWidth(q.matSchema[c].type)); src.push_back(q.dMatCols[c]); }
    OrderLimitBuffers& b = q.orderLimit.buffers;
    b.ensure(ctx, n, capacity, widths);
    OrderLimitSelection s;
    orderLimitSelect(ctx, b, q.dMatCols[(size_t)r.first_key_column], r.key_is32 ? 4 : 8, r.descending != 0, n, (uint32_t)want, src, false, s);
    q.report.num_kernels += 10;      // six digit histograms, the threshold, the counts, their scan, the gather
    r.candidates = (int64_t)s.candidates; r.select_ms = s.selectMs; r.copy_ms = s.copyMs;
    if (s.candidates > (uint64_t)capacity) { r.fallback_reason = RSQ_ORDER_LIMIT_FALLBACK_OVERFLOW; return false; }
    const double t0 = nowMs();
    const bool decided = runOrderLimitTail(q, s.cols.data(), (size_t)s.candidates);
    r.tail_ms = nowMs() - t0;
    if (!decided) { r.fallback_reason = RSQ_ORDER_LIMIT_FALLBACK_TIES; return false; }
    r.path = 1; r.fallback_reason = RSQ_ORDER_LIMIT_FALLBACK_NONE;
    return true;
}

// ORDER BY directly above the materialisation: the device orders the rows by the whole key list (order_sort.hip orderSortRows), packs all
// rows in scan order, gathers the result's tuples in the order and one copy brings them, with the tie count, into the query's pinned
// buffer.  q.hMatCols is neither filled nor read.  False leaves the result state untouched as well.
static bool orderSortOnDevice(Query& q) {
    Context& ctx = q.ctx;
    auto& st = q.orderSort;
    rsq_order_sort_report& r = st.report;
    if (ctx.orderSort != 1 || !takesMaterialisation(q, r.planned)) return false;
    const std::vector<Type> types = materialisedTypes(q);
    const int64_t n = q.matRows, ts = packTupleSize(types);
    const bool hasLimit = q.root->hasLimit;
    const int64_t lead = hasLimit ? std::min<int64_t>(n, q.root->limit + 1) : n;          // (runOrderLimitTail's rule: ties behind row k + 1 do not matter)
    const int64_t outRows = hasLimit ? std::min<int64_t>(n, q.root->limit) : n;
    r.rows = n; r.lead = std::max<int64_t>(lead, 0); r.out_rows = std::max<int64_t>(outRows, 0); r.tuple_size = (int32_t)ts;
    if (n <= 0 || hostMapped(q)) { r.fallback_reason = RSQ_ORDER_SORT_FALLBACK_SMALL; return false; }
    const size_t scanBytes = n < ((int64_t)1 << 32) ? (size_t)n * (size_t)ts : 0, outBytes = (size_t)outRows * (size_t)ts;
    const int64_t freeBytes = freeDeviceBytes(st.buffers.rows < n || st.scanBytes < scanBytes || st.outBytes < outBytes);
    if (!osort::fitsDevice(n, outRows, ts, n < ((int64_t)1 << 32) ? (int64_t)radixSortTempBytes(n) : 0, freeBytes)) { r.fallback_reason = RSQ_ORDER_SORT_FALLBACK_DOES_NOT_FIT; return false; }
    st.buffers.ensure(ctx, n);
    std::vector<OrderSortKey> keys;
    for (size_t k = 0; k < st.keyCols.size(); k++) {
        const size_t c = (size_t)st.keyCols[k];
        keys.push_back(OrderSortKey{q.dMatCols[c], columnWidth(q.matSchema[c].type), (bool)st.keyDesc[k]});
    }
    OrderSortOutcome o;
    orderSortRows(ctx, st.buffers, keys.data(), (int)keys.size(), n, lead, o);
    q.report.num_kernels += (uint32_t)o.launches;
    for (int k = 0; k < 8; k++) r.key_bits[k] = o.bits[k];
    r.total_bits = o.totalBits; r.words = o.words; r.passes = o.passes;
    float ms = 0;
    if (!o.sorted) {          // no key varies: every leading pair ties
        RSQ_HIP(hipEventSynchronize(st.buffers.ev[1]));
        RSQ_HIP(hipEventElapsedTime(&ms, st.buffers.ev[0], st.buffers.ev[1])); r.range_ms = ms;
        r.tied_pairs = o.tiedPairs; r.fallback_reason = RSQ_ORDER_SORT_FALLBACK_TIES;
        return false;
    }
    // the last execution's tuples go with these buffers' contents where the result state names them; whichever path this execution ends
    // on sets the state anew
    if (q.resultInPinned && q.resultPinned == st.pinned) { q.resultInPinned = false; q.resultDev = nullptr; q.resultRows = 0; }
    growDevice(ctx, st.dScan, st.scanBytes, scanBytes, 16);
    growDevice(ctx, st.dOut, st.outBytes, outBytes, 16);
    growPinned(ctx, st.pinned, st.pinnedBytes, outBytes + 16);
    hipEvent_t* ev = st.buffers.ev;
    packTuples(ctx, types, q.dMatCols.data(), n, st.dScan);
    RSQ_HIP(hipEventRecord(ev[4], ctx.stream));
    gatherTuples(ctx, st.dScan, st.dOut, o.dPerm, (int)ts, outRows);
    RSQ_HIP(hipEventRecord(ev[5], ctx.stream));
    q.report.num_kernels += outRows > 0 ? 2 : 1;
    const double t0 = nowMs();
    // the tuples first, the tie count and the error word behind them in the pinned buffer: one wait
    uint8_t* status = st.pinned + ((outBytes + 7) & ~(size_t)7);
    if (outBytes) RSQ_HIP(hipMemcpyAsync(st.pinned, st.dOut, outBytes, hipMemcpyDeviceToHost, ctx.stream));
    if (lead > 1) RSQ_HIP(hipMemcpyAsync(status, o.dTies, 4, hipMemcpyDeviceToHost, ctx.stream));
    RSQ_HIP(hipMemcpyAsync(status + 4, ctx.dErr, 4, hipMemcpyDeviceToHost, ctx.stream));
    waitForStream(ctx);
    r.copy_ms = nowMs() - t0;
    uint32_t ties = 0, err = 0;
    if (lead > 1) memcpy(&ties, status, 4);
    memcpy(&err, status + 4, 4);
    checkErrorWord(ctx, err);
    RSQ_HIP(hipEventElapsedTime(&ms, ev[0], ev[1])); r.range_ms = ms;
    RSQ_HIP(hipEventElapsedTime(&ms, ev[2], ev[3])); r.sort_ms = ms;
    RSQ_HIP(hipEventElapsedTime(&ms, ev[3], ev[4])); r.pack_ms = ms;
    RSQ_HIP(hipEventElapsedTime(&ms, ev[4], ev[5])); r.gather_ms = ms;
    r.tied_pairs = ties;
    if (ties) { r.fallback_reason = RSQ_ORDER_SORT_FALLBACK_TIES; return false; }
    publishDeviceResult(q, outRows, st.pinned, st.dOut);
    r.path = 1; r.fallback_reason = RSQ_ORDER_SORT_FALLBACK_NONE;
    return true;
}

// any materialisation: one launch packs all rows into the query's device buffer (result_pack.hip), one copy brings the tuples into its
// pinned buffer, and an ORDER BY above runs over them there.  q.hMatCols is neither filled nor read.
static bool resultPackOnDevice(Query& q) {
    Context& ctx = q.ctx;
    auto& st = q.resultPack;
    rsq_result_pack_report& r = st.report;
    if (ctx.resultPack != 1 || !takesMaterialisation(q, r.planned)) return false;
    const std::vector<Type> types = materialisedTypes(q);
    const int64_t n = q.matRows, ts = packTupleSize(types);
    if (n <= 0 || hostMapped(q)) { r.fallback_reason = RSQ_RESULT_PACK_FALLBACK_SMALL; return false; }
    const size_t bytes = (size_t)n * (size_t)ts;          // (at most rpack::MAX_TUPLE_BYTES where fitsDevice says yes)
    if (!rpack::fitsDevice(n, ts, freeDeviceBytes(st.devBytes < bytes))) { r.fallback_reason = RSQ_RESULT_PACK_FALLBACK_DOES_NOT_FIT; return false; }
    q.resultInPinned = false; q.resultDev = nullptr; q.resultRows = 0;          // the last result's tuples go with their buffers' contents
    growDevice(ctx, st.dev, st.devBytes, bytes);
    growPinned(ctx, st.pinned, st.pinnedBytes, bytes);
    if (!st.ev0) st.ev0 = ctx.takeEvent();
    if (!st.ev1) st.ev1 = ctx.takeEvent();
    RSQ_HIP(hipEventRecord(st.ev0, ctx.stream));
    packTuples(ctx, types, q.dMatCols.data(), n, st.dev);
    RSQ_HIP(hipEventRecord(st.ev1, ctx.stream));
    q.report.num_kernels += 1;
    const double t0 = nowMs();
    RSQ_HIP(hipMemcpyAsync(st.pinned, st.dev, bytes, hipMemcpyDeviceToHost, ctx.stream));
    uint32_t err = 0;
    RSQ_HIP(hipMemcpyAsync(&err, ctx.dErr, 4, hipMemcpyDeviceToHost, ctx.stream));
    waitForStream(ctx);
    r.copy_ms = nowMs() - t0;
    checkErrorWord(ctx, err);
    float ms = 0;
    RSQ_HIP(hipEventElapsedTime(&ms, st.ev0, st.ev1));
    r.kernel_ms = ms;
    int64_t rows = n;
    const double t1 = nowMs();
    const bool sorted = runMaterializeSort(q, st.pinned, rows);
    if (sorted) r.sort_ms = nowMs() - t1;
    publishDeviceResult(q, rows, st.pinned, sorted ? nullptr : st.dev);      // (sorted on the host: the device's tuples are not the result's order)
    r.path = 1; r.fallback_reason = RSQ_RESULT_PACK_FALLBACK_NONE; r.sorted_on_host = sorted ? 1 : 0;
    r.tuple_size = (int32_t)ts; r.rows = rows; r.tuple_bytes = rows * ts;
    return true;
}

// The precedence between the three settings, and what a decision means for the other reports.  order_limit decides first: its candidates
// are the answer, no materialised row is packed or sorted at all, and the other two say ORDER_LIMIT under their setting 1.  Then
// order_sort: it did the packing, so result_pack keeps SHAPE under its setting 1, with the relation's size.  Then result_pack.
bool runMaterializeDeviceTail(Query& q) {
    const Context& ctx = q.ctx;
    if (orderLimitOnDevice(q)) {
        if (ctx.orderSort == 1) q.orderSort.report.fallback_reason = RSQ_ORDER_SORT_FALLBACK_ORDER_LIMIT;
        if (ctx.resultPack == 1) q.resultPack.report.fallback_reason = RSQ_RESULT_PACK_FALLBACK_ORDER_LIMIT;
        resultPackHostRelation(q);
        return true;
    }
    if (orderSortOnDevice(q)) { resultPackHostRelation(q); return true; }
    return resultPackOnDevice(q);
}

}  // namespace rsq
