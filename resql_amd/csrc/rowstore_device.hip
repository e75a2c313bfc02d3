// rowstore_device.hip — a ReSQL row store transposed into columns on the device (rsq_ctx_set_rowstore_bridge, rsq_table_from_rowstore_ex).
// transposeRowstoreHost (rowstore.cpp) stays the definition of the columns; the rule of a cell is rowstore.h's, which both sides use.
// The tuples travel in chunks of whole tuples, packed back to back, through two pinned buffers into two device buffers; per chunk:
//   k_rowstore_transpose   a workgroup takes R = min(256, RS_TILE_BYTES / tuple size) consecutive tuples: their byte span staged in LDS 16
//                          bytes per lane, every string cleaned behind its first NUL in place (one lane per row), then column by column
//                          the R cells written so that consecutive lanes store consecutive addresses - 1-, 4- and 8-byte cells one per
//                          lane, a string column's R x len bytes as one span, 16 bytes per lane between its ragged ends
//                          a tuple longer than the tile (R = 0): one lane per (row, column), straight from global memory
// A chunk has at most 2^30 bytes, so indices inside it are 32-bit; the chunk's first row in the columns is 64-bit.
#include <algorithm>
#include <chrono>
#include <cstring>

#include "engine.h"
#include "rowstore.h"

namespace rsq {

#define RS_LANES 256
#define RS_TILE_BYTES 49152           /* LDS tile: the span of a workgroup's tuples, as the text kernels' (tbl_device.hip, result_text.hip); three workgroups per CU */
#define RS_TILE_SLACK 32              /* the span starts up to 15 bytes into the tile and is loaded in whole 16-byte groups; word reads end up to 7 bytes behind a cell */
#define RS_MAX_COLS 64
#define RS_MAX_CHUNK_BYTES ((int64_t)1 << 30)

// kind: what the kernel does with a field - RS_BYTES: the first `width` (1, 4 or 8) bytes, one cell per lane; RS_STRING: the NUL rule
enum { RS_BYTES = 0, RS_STRING = 1 };
struct RsCol { int32_t offset, width, kind, pad; unsigned char* ptr; };
struct RsSchema { int32_t nCols, tupleSize, groupRows, pad; RsCol col[RS_MAX_COLS]; };

// four bytes at any byte address of the tile, assembled from the two aligned words that hold them (never a misaligned wide load)
__device__ __forceinline__ unsigned tile_u32(const unsigned char* tile, unsigned a) {
    const unsigned* w = (const unsigned*)(tile + (a & ~3u));
    const unsigned long long both = ((unsigned long long)w[1] << 32) | (unsigned long long)w[0];
    return (unsigned)(both >> (8u * (a & 3u)));
}

// chunk: nRows tuples back to back, the buffer padded to whole 16-byte groups; rowBase: the chunk's first row in the columns
__global__ void __launch_bounds__(RS_LANES) k_rowstore_transpose(const unsigned char* __restrict__ chunk, unsigned nRows, int64_t rowBase, RsSchema sch) {
    __shared__ __attribute__((aligned(16))) unsigned char s_tile[RS_TILE_BYTES + RS_TILE_SLACK];
    __shared__ RsCol s_cols[RS_MAX_COLS];
    const unsigned tid = threadIdx.x, ts = (unsigned)sch.tupleSize, nCols = (unsigned)sch.nCols;
    if (tid < nCols) s_cols[tid] = sch.col[tid];
    if (sch.groupRows == 0) {          // (uniform) one tuple is longer than the tile: a lane per (row, column), straight from global memory
        __syncthreads();
        const unsigned item = blockIdx.x * RS_LANES + tid;
        const unsigned row = item / nCols, c = item - row * nCols;
        if (row >= nRows) return;
        const RsCol col = s_cols[c];
        rowst::cell(col.kind == RS_STRING ? rowst::CAT_STRING : rowst::CAT_NUMERIC, col.width, chunk + (size_t)row * ts + (unsigned)col.offset,
                    col.ptr + (rowBase + row) * (int64_t)col.width);
        return;
    }
    const unsigned R = (unsigned)sch.groupRows;
    const unsigned r0 = blockIdx.x * R;
    const unsigned nr = nRows - r0 < R ? nRows - r0 : R;
    // the tuples' span, from the 16-byte boundary in front of it (r0 * ts is rarely one): tile byte head + r * ts is row r0 + r's first
    const unsigned begin = r0 * ts, tileBegin = begin & ~15u, head = begin - tileBegin;
    const unsigned spanEnd = head + nr * ts;
    for (unsigned o = tid * 16u; o < spanEnd; o += RS_LANES * 16u) *(uint4*)(s_tile + o) = *(const uint4*)(chunk + tileBegin + o);
    __syncthreads();
    // the NUL rule, in place: behind a string's first NUL its cell is zero
    if (tid < nr) {
        for (unsigned c = 0; c < nCols; c++) {
            if (s_cols[c].kind != RS_STRING) continue;
            unsigned char* f = s_tile + head + tid * ts + (unsigned)s_cols[c].offset;
            const int w = s_cols[c].width;
            int k = 0;
            while (k < w && f[k]) k++;
            for (; k < w; k++) f[k] = 0;
        }
    }
    __syncthreads();
    const int64_t row = rowBase + r0;
    for (unsigned c = 0; c < nCols; c++) {
        const RsCol col = s_cols[c];
        if (col.kind == RS_BYTES) {
            if (tid < nr) {
                const unsigned a = head + tid * ts + (unsigned)col.offset;
                if (col.width == 4) ((unsigned*)col.ptr)[row + tid] = tile_u32(s_tile, a);
                else if (col.width == 8) ((uint2*)col.ptr)[row + tid] = make_uint2(tile_u32(s_tile, a), tile_u32(s_tile, a + 4u));
                else col.ptr[row + tid] = s_tile[a];
            }
            continue;
        }
        // a string column: the nr x len bytes its rows occupy are one span of the column.  Span byte j is byte j % len of row j / len.  The
        // span begins and ends at any byte and its neighbours are other workgroups': whole 16-byte groups are stored only where all 16
        // bytes are this workgroup's (as k_text_write does).  q = a + j: the byte's position counted from the 16-byte boundary in front of dst.
        const unsigned len = (unsigned)col.width, span = nr * len;
        if (span == 0) continue;
        unsigned char* dst = col.ptr + row * (int64_t)len;
        const unsigned char* field0 = s_tile + head + (unsigned)col.offset;
        const unsigned a = (unsigned)((uintptr_t)dst & 15u), b = a + span;
        const unsigned fullBegin = (a + 15u) & ~15u, fullEnd = b & ~15u;
        const unsigned headEnd = fullBegin < b ? fullBegin : b;                 // [a, headEnd): the partial group at the head
        const unsigned tailBegin = fullEnd > headEnd ? fullEnd : headEnd;       // [tailBegin, b): ... and at the tail
        for (unsigned q = fullBegin + tid * 16u; q < fullEnd; q += RS_LANES * 16u) {
            const unsigned j = q - a;
            unsigned r = j / len, k = j - r * len;
            const unsigned char* f = field0 + r * ts;
            unsigned w[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                unsigned v = 0;
#pragma unroll
                for (int s = 0; s < 4; s++) {
                    v |= (unsigned)f[k] << (8 * s);
                    if (++k == len) { k = 0; f += ts; }
                }
                w[i] = v;
            }
            *(uint4*)(dst + j) = make_uint4(w[0], w[1], w[2], w[3]);
        }
        if (tid < headEnd - a) { const unsigned j = tid, r = j / len; dst[j] = field0[r * ts + (j - r * len)]; }
        if (tid >= 64u && tid - 64u < b - tailBegin) { const unsigned j = tailBegin - a + (tid - 64u), r = j / len; dst[j] = field0[r * ts + (j - r * len)]; }
    }
}

namespace {

double msSince(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// everything the call holds besides the table: given back however the call ends
struct RowstoreWork {
    Context& ctx;
    void* pin[2] = {nullptr, nullptr};
    void* dev[2] = {nullptr, nullptr};
    hipEvent_t ev[6] = {};          // per buffer b: [b] its copy has arrived, [2 + b] / [4 + b] around its kernel
    explicit RowstoreWork(Context& c) : ctx(c) {}
    ~RowstoreWork() {
        (void)hipStreamSynchronize(ctx.stream);
        for (void* p : pin) ctx.freePinned(p);
        for (hipEvent_t e : ev) ctx.giveEvent(e);
        for (void* p : dev) ctx.free(p);
    }
};

}  // namespace

std::unique_ptr<Table> rowstoreToDevice(Context& ctx, const rsq_table_desc& schema, const std::vector<Type>& types, const RowstoreLayout& layout,
                                        const uint8_t* const* blocks, const size_t* contentSize, int32_t nBlocks, int64_t nRows, int64_t chunkBytes,
                                        rsq_rowstore_report& rep) {
    auto fallback = [&](int why) { rep.fallback_reason = why; return std::unique_ptr<Table>(); };
    if (ctx.device < 0) return fallback(RSQ_ROWSTORE_FALLBACK_NO_DEVICE);
    if (types.size() > RS_MAX_COLS) return fallback(RSQ_ROWSTORE_FALLBACK_COLUMNS);
    const int64_t ts = layout.tupleSize;
    if (ts > RS_MAX_CHUNK_BYTES) failInvalid("rsq_table_from_rowstore: a tuple of " + std::to_string(ts) + " bytes is longer than a chunk of the device path may be (1 GiB)");
    RsSchema sch{};
    sch.nCols = (int32_t)types.size(); sch.tupleSize = (int32_t)ts;
    sch.groupRows = ts <= RS_TILE_BYTES ? (int32_t)std::min<int64_t>(RS_LANES, RS_TILE_BYTES / ts) : 0;
    for (size_t i = 0; i < types.size(); i++) {
        if (layout.width[i] < 0) failInvalid(std::string("rsq_table_from_rowstore: column ") + std::string(schema.cols[i].name, strnlen(schema.cols[i].name, RSQ_SYMBOL_MAX)) + " has a negative length");
        sch.col[i].offset = layout.offset[i]; sch.col[i].width = layout.width[i];
        // (a string of one byte is its first byte: the NUL rule changes nothing, and the cell goes one per lane)
        sch.col[i].kind = layout.category[i] == rowst::CAT_STRING && layout.width[i] != 1 ? RS_STRING : RS_BYTES;
    }
    RSQ_HIP(hipSetDevice(ctx.device));

    // ---- the table: the kernel writes every byte of every cell, so the columns need no memset ----
    std::unique_ptr<Table> t(new Table());
    t->ctx = &ctx;
    t->name = std::string(schema.name, strnlen(schema.name, RSQ_SYMBOL_MAX));
    t->nRows = nRows;
    for (size_t i = 0; i < types.size(); i++) {
        TableColumn tc;
        tc.name = std::string(schema.cols[i].name, strnlen(schema.cols[i].name, RSQ_SYMBOL_MAX));
        tc.type = types[i];
        tc.dptr = ctx.allocRaw((size_t)nRows * (size_t)layout.width[i]); tc.owned = true;
        t->cols.push_back(tc);
        sch.col[i].ptr = (unsigned char*)tc.dptr;
    }
    rep.path = 1;
    if (nRows == 0) return t;

    // ---- chunks of whole tuples: two pinned buffers in turn, filling chunk k + 1 while chunk k is on the link and in its kernel ----
    const int64_t chunkRows = std::min<int64_t>(nRows, std::max<int64_t>(1, (chunkBytes ? chunkBytes : (int64_t)64 << 20) / ts));
    const size_t bufBytes = (((size_t)(chunkRows * ts) + 15) & ~(size_t)15) + 16;          // (the kernel's last 16-byte load stays inside)
    RowstoreWork w(ctx);
    for (auto& e : w.ev) e = ctx.takeEvent();
    for (auto& p : w.pin) p = ctx.allocPinned(bufBytes);
    for (auto& p : w.dev) p = ctx.alloc(bufBytes);
    bool timed[2] = {false, false};
    auto collectKernel = [&](int b) {          // the kernel time of the chunk buffer b held last
        if (!timed[b]) return;
        RSQ_HIP(hipEventSynchronize(w.ev[4 + b]));
        float ms = 0;
        RSQ_HIP(hipEventElapsedTime(&ms, w.ev[2 + b], w.ev[4 + b]));
        rep.kernel_ms += ms;
        timed[b] = false;
    };
    int32_t blk = 0;          // the next tuple to take: tuple `tup` of block `blk`
    size_t tup = 0;
    int k = 0;
    for (int64_t row0 = 0; row0 < nRows; row0 += chunkRows, k++) {
        const int b = k & 1;
        const int64_t n = std::min<int64_t>(chunkRows, nRows - row0);
        if (k >= 2) {
            auto t0 = std::chrono::steady_clock::now();
            RSQ_HIP(hipEventSynchronize(w.ev[b]));
            rep.copy_ms += msSince(t0);
        }
        auto t0 = std::chrono::steady_clock::now();
        unsigned char* dstp = (unsigned char*)w.pin[b];
        for (int64_t left = n; left > 0;) {
            const size_t inBlock = contentSize[blk] / (size_t)ts;
            if (tup >= inBlock) { blk++; tup = 0; continue; }          // (blocks of less than one tuple, and a block's remainder, are passed over)
            const size_t take = (size_t)std::min<int64_t>(left, (int64_t)(inBlock - tup));
            memcpy(dstp, blocks[blk] + tup * (size_t)ts, take * (size_t)ts);
            dstp += take * (size_t)ts; tup += take; left -= (int64_t)take;
        }
        rep.stage_ms += msSince(t0);
        collectKernel(b);
        RSQ_HIP(hipMemcpyAsync(w.dev[b], w.pin[b], (size_t)(n * ts), hipMemcpyHostToDevice, ctx.stream));
        RSQ_HIP(hipEventRecord(w.ev[b], ctx.stream));
        const int64_t groups = sch.groupRows ? (n + sch.groupRows - 1) / sch.groupRows : (n * sch.nCols + RS_LANES - 1) / RS_LANES;
        RSQ_HIP(hipEventRecord(w.ev[2 + b], ctx.stream));
        hipLaunchKernelGGL(k_rowstore_transpose, dim3((unsigned)groups), dim3(RS_LANES), 0, ctx.stream, (const unsigned char*)w.dev[b], (unsigned)n, (int64_t)row0, sch);
        RSQ_HIP(hipGetLastError());
        RSQ_HIP(hipEventRecord(w.ev[4 + b], ctx.stream));
        timed[b] = true;
        rep.chunks++;
    }
    {
        auto t0 = std::chrono::steady_clock::now();
        RSQ_HIP(hipStreamSynchronize(ctx.stream));
        rep.copy_ms += msSince(t0);
    }
    collectKernel(0); collectKernel(1);
    return t;
}

}  // namespace rsq
