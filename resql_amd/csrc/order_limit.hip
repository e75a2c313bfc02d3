// order_limit.hip — ORDER BY ... LIMIT k over a materialisation: the rows that decide the answer, selected on the device
// (rsq_ctx_set_order_limit, rsq_prim_column_topk; engine.h orderLimitSelect).
//
// The materialisation's rows lie in struct-of-arrays columns in scan order.  The first sort key's cell becomes an unsigned image in
// which "earlier in the requested order" is "larger" (order_limit.h).  With want = k + 1:
//   threshold   T = the want-th largest image, exactly: an MSB-first radix select in the digit scheme of the aggregation tails'
//               pre-selection (aot_kernels.hip k_topk_hist: five 11-bit digits and one of 9 bits, per-workgroup LDS histograms flushed with
//               one atomic per non-empty bin, every workgroup re-deriving the prefix chosen so far from the earlier histograms), restated
//               with the key read from its column at its own width in every pass - no image array.  Fewer than want rows: T = 0, every
//               row is a candidate.
//   counts      one count per 256-row block of the rows with image >= T (a wave's ballot, one atomic per wave that holds any)
//   offsets     the toolkit's exclusive scan over the counts and a trailing zero: the last offset is the number of candidates, exact
//   gather      a workgroup per 256-row block that holds candidates: row r goes to the block's offset plus its rank in the workgroup (ballot
//               and popcount in the wave, wave totals through LDS) - SCAN ORDER - as its position (u32) and its cell of every column,
//               numbers at their width, any other width (a string column's span) byte by byte.  Rows beyond the capacity are not written.
// The candidates are one deterministic array: a test compares them with numpy, and the host tail meets them in the order the full
// path would have.  256-thread workgroups, grid-stride loops over the blocks, at most eight workgroups per CU.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>

#include "engine.h"
#include "order_limit.h"
#include "scan_device.h"

namespace rsq {
namespace {

enum { OL_PASSES = 6, OL_BINS = 2048, OL_BLOCK = 256 };
__device__ __forceinline__ int ol_shift(int p) { return p < 5 ? 53 - 11 * p : 0; }
__device__ __forceinline__ int ol_bits(int p) { return p < 5 ? 11 : 9; }

struct OlColumns {
    int32_t n, pad;
    int32_t width[ORDER_LIMIT_MAX_COLUMNS];
    const unsigned char* src[ORDER_LIMIT_MAX_COLUMNS];
    unsigned char* dst[ORDER_LIMIT_MAX_COLUMNS];
};

// Replays the digit choices of passes [0, upto) (aot_kernels.hip topk_prefix): the chosen prefix - the top bits of T, right-aligned - and
// in *remOut how many rows with exactly that prefix are still wanted; *allOut: fewer than `want` rows exist.  All 256 threads call it.
__device__ u64 ol_prefix(const unsigned* __restrict__ hists, int upto, unsigned want, unsigned* remOut, int* allOut) {
    __shared__ unsigned s_above[OL_BLOCK];
    __shared__ unsigned s_digit, s_rem;
    __shared__ int s_found;
    const int t = threadIdx.x;
    u64 prefix = 0;
    unsigned rem = want;
    int all = 0;
    for (int p = 0; p < upto && !all; p++) {
        const unsigned* h = hists + (size_t)p * OL_BINS;
        unsigned c[8], local = 0;
#pragma unroll
        for (int b = 0; b < 8; b++) { c[b] = h[t * 8 + b]; local += c[b]; }
        if (t == 0) s_found = 0;
        s_above[t] = local;
        __syncthreads();
        for (int d = 1; d < OL_BLOCK; d <<= 1) {             // inclusive suffix sums over the threads
            const unsigned v = t + d < OL_BLOCK ? s_above[t + d] : 0u;
            __syncthreads();
            s_above[t] += v;
            __syncthreads();
        }
        unsigned running = s_above[t] - local;               // rows in bins above this thread's eight
#pragma unroll
        for (int b = 7; b >= 0; b--) {
            if (running < rem && rem <= running + c[b]) { s_digit = (unsigned)(t * 8 + b); s_rem = rem - running; s_found = 1; }
            running += c[b];
        }
        __syncthreads();
        if (!s_found) all = 1;
        else { prefix = (prefix << ol_bits(p)) | (u64)s_digit; rem = s_rem; }
        __syncthreads();
    }
    *remOut = rem; *allOut = all;
    return prefix;
}

// pass p: histogram of digit p over the rows whose higher digits equal the prefix chosen so far
__global__ void __launch_bounds__(OL_BLOCK) k_ol_hist(const unsigned char* __restrict__ key, int width, int desc, i64 n, unsigned* __restrict__ hists,
                                                     int pass, unsigned want) {
    __shared__ unsigned s_hist[OL_BINS];
    for (int b = threadIdx.x; b < OL_BINS; b += OL_BLOCK) s_hist[b] = 0;
    unsigned rem; int all;
    const u64 prefix = ol_prefix(hists, pass, want, &rem, &all);        // contains the barriers that publish s_hist = 0
    if (all) return;
    const int shift = ol_shift(pass);
    const unsigned mask = (1u << ol_bits(pass)) - 1u;
    const int above = shift + ol_bits(pass);                            // bits above this digit (64 in pass 0: not shifted by)
    __syncthreads();
    for (i64 i = (i64)blockIdx.x * OL_BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * OL_BLOCK) {
        const u64 u = ordlim::image(key + (size_t)i * (size_t)width, width, desc != 0);
        if (pass == 0 || (u >> above) == prefix) atomicAdd(&s_hist[(unsigned)(u >> shift) & mask], 1u);
    }
    __syncthreads();
    unsigned* h = hists + (size_t)pass * OL_BINS;
    for (int b = threadIdx.x; b < OL_BINS; b += OL_BLOCK) { const unsigned c = s_hist[b]; if (c) atomicAdd(&h[b], c); }
}

// one workgroup: T from the six histograms (0 where fewer than `want` rows exist: every image is at or above it)
__global__ void __launch_bounds__(OL_BLOCK) k_ol_threshold(const unsigned* __restrict__ hists, unsigned want, u64* __restrict__ threshold) {
    unsigned rem; int all;
    const u64 T = ol_prefix(hists, OL_PASSES, want, &rem, &all);
    if (threadIdx.x == 0) *threshold = all ? 0ull : T;
}

// counts[b] (zero before the launch) = rows of 256-row block b with image >= T
__global__ void __launch_bounds__(OL_BLOCK) k_ol_count(const unsigned char* __restrict__ key, int width, int desc, i64 n, const u64* __restrict__ threshold,
                                                      unsigned* __restrict__ counts) {
    const u64 T = *threshold;
    const i64 nBlocks = (n + OL_BLOCK - 1) / OL_BLOCK;
    const int lane = threadIdx.x & 63;
    for (i64 b = blockIdx.x; b < nBlocks; b += gridDim.x) {
        const i64 r = b * OL_BLOCK + threadIdx.x;
        const bool take = r < n && ordlim::image(key + (size_t)r * (size_t)width, width, desc != 0) >= T;
        const u64 vote = __ballot(take);
        if (lane == 0 && vote) atomicAdd(&counts[b], (unsigned)__popcll(vote));
    }
}

// offs[b] = candidates in front of block b, offs[nBlocks] = all of them.  Candidate number p < capacity: positions[p] = its row,
// cols.dst[c] + p * width[c] = its cell of column c.
__global__ void __launch_bounds__(OL_BLOCK) k_ol_gather(const unsigned char* __restrict__ key, int width, int desc, i64 n, const u64* __restrict__ threshold,
                                                       const u64* __restrict__ offs, OlColumns cols, unsigned* __restrict__ positions, u64 capacity) {
    __shared__ unsigned s_wave[OL_BLOCK / 64];
    const u64 T = *threshold;
    const i64 nBlocks = (n + OL_BLOCK - 1) / OL_BLOCK;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (i64 b = blockIdx.x; b < nBlocks; b += gridDim.x) {
        const u64 base = offs[b];
        if (offs[b + 1] == base || base >= capacity) continue;          // (the same for every thread of the workgroup)
        const i64 r = b * OL_BLOCK + threadIdx.x;
        const bool take = r < n && ordlim::image(key + (size_t)r * (size_t)width, width, desc != 0) >= T;
        const u64 vote = __ballot(take);
        if (lane == 0) s_wave[wave] = (unsigned)__popcll(vote);
        __syncthreads();
        unsigned before = 0;
        for (int w = 0; w < wave; w++) before += s_wave[w];
        __syncthreads();                                                // (s_wave is written again in the workgroup's next block)
        if (!take) continue;
        const u64 p = base + before + (unsigned)__popcll(vote & ((1ull << lane) - 1ull));
        if (p >= capacity) continue;
        positions[p] = (unsigned)r;
        for (int c = 0; c < cols.n; c++) {
            const int w = cols.width[c];
            const unsigned char* s = cols.src[c] + (size_t)r * (size_t)w;
            unsigned char* d = cols.dst[c] + (size_t)p * (size_t)w;
            if (w == 4) *(unsigned*)d = *(const unsigned*)s;
            else if (w == 8) *(u64*)d = *(const u64*)s;
            else for (int k = 0; k < w; k++) d[k] = s[k];
        }
    }
}

size_t olScratchBytes() { return (size_t)OL_PASSES * OL_BINS * 4 + 16; }
size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }
double msSince(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

}  // namespace

void OrderLimitBuffers::ensure(Context& ctx, int64_t nRows, int64_t cap, const std::vector<int32_t>& w) {
    if (w.size() > (size_t)ORDER_LIMIT_MAX_COLUMNS) throw Error(RSQ_ERR_UNSUPPORTED, "order_limit: more than 32 columns");
    if (!dScratch) dScratch = (uint32_t*)ctx.alloc(olScratchBytes());
    if (!ev0) { ev0 = ctx.takeEvent(); ev1 = ctx.takeEvent(); }
    const int64_t needBlocks = (nRows + OL_BLOCK - 1) / OL_BLOCK;
    if (!dCounts || needBlocks > blocks) {
        if (dCounts) ctx.free(dCounts);
        if (dOffs) ctx.free(dOffs);
        if (dScanTemp) ctx.free(dScanTemp);
        dCounts = nullptr; dOffs = nullptr; dScanTemp = nullptr;
        blocks = needBlocks;
        dCounts = (uint32_t*)ctx.alloc((size_t)(blocks + 1) * 4);
        dOffs = (uint64_t*)ctx.alloc((size_t)(blocks + 1) * 8);
        scanBytes = scanTempBytes(blocks + 1);
        dScanTemp = ctx.alloc(scanBytes);
    }
    if (!dPositions || cap != capacity || w != widths) {
        if (dPositions) ctx.free(dPositions);
        for (void* p : dCols) ctx.free(p);
        dPositions = nullptr; dCols.clear();
        capacity = cap; widths = w;
        dPositions = (uint32_t*)ctx.alloc(std::max<size_t>(16, (size_t)capacity * 4));
        for (int32_t cw : widths) dCols.push_back(ctx.alloc(std::max<size_t>(16, (size_t)capacity * (size_t)cw)));
    }
}

void OrderLimitBuffers::release(Context& ctx) {
    if (dScratch) ctx.free(dScratch);
    if (dCounts) ctx.free(dCounts);
    if (dOffs) ctx.free(dOffs);
    if (dScanTemp) ctx.free(dScanTemp);
    if (dPositions) ctx.free(dPositions);
    for (void* p : dCols) ctx.free(p);
    if (pinned) ctx.freePinned(pinned);
    ctx.giveEvent(ev0); ctx.giveEvent(ev1);
    *this = OrderLimitBuffers();
}

void orderLimitSelect(Context& ctx, OrderLimitBuffers& b, const void* key, int keyWidth, bool desc, int64_t nRows, uint32_t want,
                      const std::vector<const void*>& src, bool everything, OrderLimitSelection& out) {
    if ((keyWidth != 4 && keyWidth != 8) || nRows < 0 || nRows >= ((int64_t)1 << 32) || want < 1 || src.size() != b.widths.size() ||
        src.size() != b.dCols.size() || (nRows + OL_BLOCK - 1) / OL_BLOCK > b.blocks || b.capacity < 1)
        throw Error(RSQ_ERR_RUNTIME, "internal error: order_limit selection outside its buffers");
    const i64 nBlocks = (nRows + OL_BLOCK - 1) / OL_BLOCK;
    unsigned* hists = b.dScratch;
    u64* threshold = (u64*)(b.dScratch + (size_t)OL_PASSES * OL_BINS);
    OlColumns cols{};
    cols.n = (int32_t)src.size();
    for (size_t c = 0; c < src.size(); c++) { cols.width[c] = b.widths[c]; cols.src[c] = (const unsigned char*)src[c]; cols.dst[c] = (unsigned char*)b.dCols[c]; }
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(8 * (int64_t)ctx.numCUs, nBlocks));
    const unsigned char* k = (const unsigned char*)key;
    RSQ_HIP(hipEventRecord(b.ev0, ctx.stream));
    RSQ_HIP(hipMemsetAsync(b.dScratch, 0, olScratchBytes(), ctx.stream));
    RSQ_HIP(hipMemsetAsync(b.dCounts, 0, (size_t)(nBlocks + 1) * 4, ctx.stream));
    if (everything) {
        RSQ_HIP(hipMemsetAsync(b.dPositions, 0xff, (size_t)b.capacity * 4, ctx.stream));
        for (size_t c = 0; c < src.size(); c++) RSQ_HIP(hipMemsetAsync(b.dCols[c], 0xff, (size_t)b.capacity * (size_t)b.widths[c], ctx.stream));
    }
    for (int p = 0; p < OL_PASSES; p++)
        hipLaunchKernelGGL(k_ol_hist, dim3(grid), dim3(OL_BLOCK), 0, ctx.stream, k, keyWidth, desc ? 1 : 0, (i64)nRows, hists, p, (unsigned)want);
    hipLaunchKernelGGL(k_ol_threshold, dim3(1), dim3(OL_BLOCK), 0, ctx.stream, (const unsigned*)hists, (unsigned)want, threshold);
    hipLaunchKernelGGL(k_ol_count, dim3(grid), dim3(OL_BLOCK), 0, ctx.stream, k, keyWidth, desc ? 1 : 0, (i64)nRows, (const u64*)threshold, (unsigned*)b.dCounts);
    exclusiveScanCounts(ctx, b.dCounts, b.dOffs, nBlocks + 1, b.dScanTemp, b.scanBytes);
    hipLaunchKernelGGL(k_ol_gather, dim3(grid), dim3(OL_BLOCK), 0, ctx.stream, k, keyWidth, desc ? 1 : 0, (i64)nRows, (const u64*)threshold, (const u64*)b.dOffs,
                       cols, (unsigned*)b.dPositions, (u64)b.capacity);
    RSQ_HIP(hipGetLastError());
    RSQ_HIP(hipEventRecord(b.ev1, ctx.stream));
    const auto t0 = std::chrono::steady_clock::now();
    // the status words first: how many rows come back decides how much pinned memory they need
    if (!b.pinned) { b.pinnedBytes = (size_t)64 << 10; b.pinned = (uint8_t*)ctx.allocPinned(b.pinnedBytes); }
    RSQ_HIP(hipMemcpyAsync(b.pinned, b.dOffs + nBlocks, 8, hipMemcpyDeviceToHost, ctx.stream));
    RSQ_HIP(hipMemcpyAsync(b.pinned + 8, threshold, 8, hipMemcpyDeviceToHost, ctx.stream));
    RSQ_HIP(hipStreamSynchronize(ctx.stream));
    ctx.streamDrained();
    memcpy(&out.candidates, b.pinned, 8);
    memcpy(&out.threshold, b.pinned + 8, 8);
    const size_t rows = everything ? (size_t)b.capacity : out.candidates <= (uint64_t)b.capacity ? (size_t)out.candidates : 0;
    size_t need = 16 + round16(rows * 4);
    for (int32_t w : b.widths) need += round16(rows * (size_t)w);
    if (need > b.pinnedBytes) {
        ctx.freePinned(b.pinned);
        b.pinned = nullptr; b.pinnedBytes = 0;
        b.pinned = (uint8_t*)ctx.allocPinned(need);
        b.pinnedBytes = need;
    }
    size_t at = 16;
    out.positions = (const uint32_t*)(b.pinned + at);
    if (rows) RSQ_HIP(hipMemcpyAsync(b.pinned + at, b.dPositions, rows * 4, hipMemcpyDeviceToHost, ctx.stream));
    at += round16(rows * 4);
    out.cols.clear();
    for (size_t c = 0; c < b.widths.size(); c++) {
        const size_t bytes = rows * (size_t)b.widths[c];
        out.cols.push_back(b.pinned + at);
        if (bytes) RSQ_HIP(hipMemcpyAsync(b.pinned + at, b.dCols[c], bytes, hipMemcpyDeviceToHost, ctx.stream));
        at += round16(bytes);
    }
    RSQ_HIP(hipStreamSynchronize(ctx.stream));
    ctx.streamDrained();
    out.copyMs = msSince(t0);
    float ms = 0;
    RSQ_HIP(hipEventElapsedTime(&ms, b.ev0, b.ev1));
    out.selectMs = ms;
}

}  // namespace rsq
