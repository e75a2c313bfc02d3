// result_text.hip — a result relation's '.tbl' text written on the device (rsq_ctx_set_result_text, rsq_query_result_text / _write, the
// statement loop's `tofile`).  serializeResultView (engine.cpp) stays the definition of the text; the cells' text is result_text.h's,
// which is checked against it.  The tuples are uploaded in chunks of rows - or, where the materialisation's device tail left them in the
// query's own device buffer (rsq_ctx_set_result_pack), read there, a chunk beginning at any byte offset; per chunk:
//   k_text_lengths   one lane per row, TEXT_GROUP_ROWS per workgroup: rowLen[row] = the row's text length (one terminator per cell, one
//                    newline), groupBytes[workgroup] = the workgroup's total            -> exclusiveScanCounts: every workgroup's first byte
//   k_text_write     the same geometry: the rows' starts from a scan of rowLen inside the workgroup; where the workgroup's span fits the
//                    LDS tile every lane writes its row there and the workgroup copies the tile out 16 bytes per lane, else the lanes
//                    write their rows straight to global memory
// A chunk's text is shorter than 2^32 bytes, so offsets inside it are 32-bit.
#include <algorithm>
#include <chrono>
#include <cstring>

#include "engine.h"
#include "result_text.h"
#include "scan_device.h"

namespace rsq {

#define TEXT_GROUP_ROWS 256           /* rows per workgroup of both kernels */
#define TEXT_TILE_BYTES 49152         /* LDS tile of the write: a span of 256 rows of up to 192 B on average, as k_tbl_parse's; three workgroups per CU */
#define TEXT_MAX_COLS 64
#define TEXT_MAX_ROW_BYTES 65536      /* upper bound of one row's text the device path takes */

struct TextCol { int32_t category, offset, lenOrScale; };
struct TextSchema { int32_t nCols, tupleSize; TextCol col[TEXT_MAX_COLS]; };

__global__ void __launch_bounds__(TEXT_GROUP_ROWS) k_text_lengths(const unsigned char* __restrict__ tuples, i64 nRows, TextSchema sch, unsigned* __restrict__ rowLen,
                                                                  unsigned* __restrict__ groupBytes) {
    __shared__ unsigned s_wave[TEXT_GROUP_ROWS / 64];
    __shared__ TextCol s_cols[TEXT_MAX_COLS];
    if ((int)threadIdx.x < sch.nCols) s_cols[threadIdx.x] = sch.col[threadIdx.x];
    __syncthreads();
    const i64 row = (i64)blockIdx.x * TEXT_GROUP_ROWS + threadIdx.x;
    unsigned len = 0;
    if (row < nRows) {
        const unsigned char* t = tuples + row * (i64)sch.tupleSize;
        for (int c = 0; c < sch.nCols; c++) len += (unsigned)rtxt::cellTextLength(s_cols[c].category, s_cols[c].lenOrScale, t + s_cols[c].offset);
        len += (unsigned)sch.nCols + 1u;
        rowLen[row] = len;
    }
    unsigned total;
    block_scan<TEXT_GROUP_ROWS, unsigned, ScanSum>(len, s_wave, &total);
    if (threadIdx.x == 0) groupBytes[blockIdx.x] = total;
}

// the row's cells, each with its terminator, and the newline: exactly rowLen bytes
__device__ __forceinline__ void write_row(const unsigned char* t, const TextCol* cols, int nCols, unsigned char* out) {
    for (int c = 0; c < nCols; c++) {
        out += rtxt::writeCellText(cols[c].category, cols[c].lenOrScale, t + cols[c].offset, out);
        *out++ = '|';
    }
    *out = '\n';
}

// groupStart[workgroup]: the workgroup's first byte in `text` (the scan of groupBytes).  A span begins and ends at any byte, and the bytes
// on either side of its ends are a neighbouring workgroup's: whole 16-byte groups are stored only where all 16 bytes are this workgroup's.
__global__ void __launch_bounds__(TEXT_GROUP_ROWS) k_text_write(const unsigned char* __restrict__ tuples, i64 nRows, TextSchema sch, const unsigned* __restrict__ rowLen,
                                                                const u64* __restrict__ groupStart, unsigned char* __restrict__ text) {
    __shared__ __attribute__((aligned(16))) unsigned char s_tile[TEXT_TILE_BYTES];
    __shared__ unsigned s_wave[TEXT_GROUP_ROWS / 64];
    __shared__ TextCol s_cols[TEXT_MAX_COLS];
    if ((int)threadIdx.x < sch.nCols) s_cols[threadIdx.x] = sch.col[threadIdx.x];
    const i64 row = (i64)blockIdx.x * TEXT_GROUP_ROWS + threadIdx.x;
    const unsigned len = row < nRows ? rowLen[row] : 0u;
    unsigned span;
    const unsigned start = block_scan<TEXT_GROUP_ROWS, unsigned, ScanSum>(len, s_wave, &span);          // (its barrier also publishes s_cols)
    unsigned char* dst = text + groupStart[blockIdx.x];
    const unsigned char* t = tuples + row * (i64)sch.tupleSize;
    // the tile holds the span at the same position inside a 16-byte group as global memory does: tile byte p is dst[p - a]
    const unsigned a = (unsigned)((uintptr_t)dst & 15u), b = a + span;
    if (b > TEXT_TILE_BYTES) {          // (uniform) a span longer than the tile: straight to global memory
        if (len) write_row(t, s_cols, sch.nCols, dst + start);
        return;
    }
    if (len) write_row(t, s_cols, sch.nCols, s_tile + a + start);
    __syncthreads();
    const unsigned fullBegin = (a + 15u) & ~15u, fullEnd = b & ~15u;
    const unsigned headEnd = fullBegin < b ? fullBegin : b;                 // [a, headEnd): the partial group at the head
    const unsigned tailBegin = fullEnd > headEnd ? fullEnd : headEnd;       // [tailBegin, b): ... and at the tail
    for (unsigned p = fullBegin + threadIdx.x * 16u; p < fullEnd; p += TEXT_GROUP_ROWS * 16u) *(uint4*)(dst + (p - a)) = *(const uint4*)(s_tile + p);
    if (threadIdx.x < headEnd - a) dst[threadIdx.x] = s_tile[a + threadIdx.x];
    if (threadIdx.x >= 64u && threadIdx.x - 64u < b - tailBegin) dst[tailBegin - a + (threadIdx.x - 64u)] = s_tile[tailBegin + (threadIdx.x - 64u)];
}

void TextOut::append(const void* p, size_t n) {
    if (!n) return;
    if (file) {
        if (fwrite(p, 1, n, file) != n) throw Error(RSQ_ERR_RUNTIME, "could not write the result text");
        return;
    }
    if (size + n + 1 > cap) {
        size_t want = std::max<size_t>(cap * 2, size + n + 1);
        char* nb = (char*)realloc(buf, want);
        if (!nb) throw std::bad_alloc();
        buf = nb; cap = want;
    }
    memcpy(buf + size, p, n);
    size += n;
}
void TextOut::closeFile() {
    FILE* f = file;
    file = nullptr;
    if (f && fclose(f) != 0) throw Error(RSQ_ERR_RUNTIME, "could not write the result text");
}
char* TextOut::release() {
    if (!buf) { buf = (char*)malloc(1); if (!buf) throw std::bad_alloc(); cap = 1; }
    buf[size] = '\0';
    char* p = buf;
    buf = nullptr; cap = 0;
    return p;
}

namespace {

double msSince(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// everything the call holds: given back however it ends
struct TextWork {
    Context& ctx;
    void* pin = nullptr;
    hipEvent_t ev[4] = {};
    std::vector<void*> dev;
    explicit TextWork(Context& c) : ctx(c) {}
    void* device(size_t bytes) { void* p = ctx.alloc(bytes); dev.push_back(p); return p; }
    ~TextWork() {
        (void)hipStreamSynchronize(ctx.stream);
        ctx.freePinned(pin);
        for (hipEvent_t e : ev) ctx.giveEvent(e);
        for (void* p : dev) ctx.free(p);
    }
};

// false: the view's schema is outside the device form.  *rowBound: upper bound of one row's text.
bool textSchemaOf(const rsq_result_view& v, TextSchema& sch, int64_t* rowBound) {
    if (v.n_cols < 0 || v.n_cols > TEXT_MAX_COLS || v.tuple_size < 0) return false;
    sch.nCols = v.n_cols; sch.tupleSize = v.tuple_size;
    int64_t bound = (int64_t)v.n_cols + 1;
    for (int c = 0; c < v.n_cols; c++) {
        const Type ty = Type::fromC(v.types[c]);
        TextCol& tc = sch.col[c];
        tc.offset = v.offsets[c]; tc.lenOrScale = 0;
        switch (ty.tag) {
            case RSQ_INT: tc.category = rtxt::CAT_INT; break;
            case RSQ_BIGINT: tc.category = rtxt::CAT_BIGINT; break;
            case RSQ_DATE: tc.category = rtxt::CAT_DATE; break;
            case RSQ_BOOL: tc.category = rtxt::CAT_BOOL; break;
            case RSQ_DECIMAL: if (ty.scale > 18) return false; tc.category = rtxt::CAT_DECIMAL; tc.lenOrScale = ty.scale; break;
            case RSQ_CHAR: if (ty.len < 1) return false; tc.category = rtxt::CAT_CHAR; tc.lenOrScale = ty.len; break;
            case RSQ_VARCHAR: if (ty.len < 0) return false; tc.category = rtxt::CAT_VARCHAR; tc.lenOrScale = ty.len; break;
            default: return false;          // (the host path raises its own error)
        }
        bound += rtxt::maxCellTextLength(tc.category, tc.lenOrScale);
        if (bound > TEXT_MAX_ROW_BYTES) return false;
    }
    *rowBound = bound;
    return true;
}

// device memory of a chunk of `rows` rows: tuples (tupleSize 0: they are on the device already), text (its upper bound, rounded up to whole 16-byte groups), row lengths, the workgroups' totals
// with their trailing slot, their offsets, the scan's temporary
size_t chunkDeviceBytes(int64_t rows, int64_t tupleSize, int64_t rowBound) {
    const int64_t groups = (rows + TEXT_GROUP_ROWS - 1) / TEXT_GROUP_ROWS;
    return (size_t)(rows * tupleSize + 16) + (size_t)(rows * rowBound + 32) + (size_t)rows * 4 + (size_t)(groups + 1) * 12 + 64 + scanTempBytes(groups + 1);
}

bool textOnDevice(Context& ctx, const rsq_result_view& v, const uint8_t* devTuples, int64_t chunkRows, int64_t maxDeviceBytes, TextOut& out, rsq_result_text_report& rep) {
    if (ctx.device < 0) { rep.fallback_reason = RSQ_TEXT_FALLBACK_NO_DEVICE; return false; }
    TextSchema sch{};
    int64_t rowBound = 0;
    if (!textSchemaOf(v, sch, &rowBound)) { rep.fallback_reason = RSQ_TEXT_FALLBACK_SCHEMA; return false; }
    RSQ_HIP(hipSetDevice(ctx.device));
    size_t limit = (size_t)maxDeviceBytes;
    if (maxDeviceBytes == 0) {
        size_t freeBytes = 0, totalBytes = 0;
        RSQ_HIP(hipMemGetInfo(&freeBytes, &totalBytes));
        limit = freeBytes > ((size_t)1 << 30) ? freeBytes - ((size_t)1 << 30) : 0;
    }
    // rows per chunk: the chunk's upper-bound text stays below 2^32 (chosen: at most 64 MiB, which is also the pinned staging), and the
    // chunk fits the budget - halved until it does
    const int64_t nRows = v.n_rows;
    int64_t rows = chunkRows > 0 ? chunkRows : std::max<int64_t>(TEXT_GROUP_ROWS, ((int64_t)64 << 20) / rowBound);
    rows = std::min<int64_t>(rows, (int64_t)0xffffffffll / rowBound);
    rows = std::max<int64_t>(1, std::min<int64_t>(rows, nRows));
    const int64_t uploaded = devTuples ? 0 : v.tuple_size;          // bytes per row the chunk's tuple buffer takes
    while (rows > 1 && chunkDeviceBytes(rows, uploaded, rowBound) > limit) rows /= 2;
    if (chunkDeviceBytes(rows, uploaded, rowBound) > limit) { rep.fallback_reason = RSQ_TEXT_FALLBACK_DOES_NOT_FIT; return false; }
    rep.path = 1; rep.rows = nRows; rep.tuples_from_device = devTuples ? 1 : 0;
    if (nRows == 0) return true;

    TextWork w(ctx);
    const int64_t groupsMax = (rows + TEXT_GROUP_ROWS - 1) / TEXT_GROUP_ROWS;
    unsigned char* dTuples = devTuples ? nullptr : (unsigned char*)w.device((size_t)(rows * v.tuple_size + 16));
    unsigned char* dText = (unsigned char*)w.device((size_t)(rows * rowBound + 32));
    unsigned* dRowLen = (unsigned*)w.device((size_t)rows * 4);
    unsigned* dGroupBytes = (unsigned*)w.device((size_t)(groupsMax + 1) * 4);
    uint64_t* dGroupStart = (uint64_t*)w.device((size_t)(groupsMax + 1) * 8);
    void* dTemp = w.device(scanTempBytes(groupsMax + 1));
    w.pin = ctx.allocPinned((size_t)(rows * rowBound + 32));
    for (auto& e : w.ev) e = ctx.takeEvent();
    for (int64_t r0 = 0; r0 < nRows; r0 += rows) {
        const int64_t n = std::min<int64_t>(rows, nRows - r0);
        const int64_t groups = (n + TEXT_GROUP_ROWS - 1) / TEXT_GROUP_ROWS;
        // the chunk's tuples: uploaded, or where they lie (the kernels address tuples + row x tupleSize per lane; rtxt:: loads cells at any byte address - unaligned 4- and 8-byte loads)
        const unsigned char* chunk = devTuples ? devTuples + (size_t)r0 * (size_t)v.tuple_size : dTuples;
        RSQ_HIP(hipEventRecord(w.ev[0], ctx.stream));
        if (!devTuples && v.tuple_size > 0) RSQ_HIP(hipMemcpyAsync(dTuples, v.tuples + (size_t)r0 * (size_t)v.tuple_size, (size_t)n * (size_t)v.tuple_size, hipMemcpyHostToDevice, ctx.stream));
        RSQ_HIP(hipEventRecord(w.ev[1], ctx.stream));
        RSQ_HIP(hipMemsetAsync(dGroupBytes + groups, 0, 4, ctx.stream));          // (the trailing slot: dGroupStart[groups] = the chunk's bytes)
        hipLaunchKernelGGL(k_text_lengths, dim3((unsigned)groups), dim3(TEXT_GROUP_ROWS), 0, ctx.stream, chunk, (i64)n, sch, dRowLen, dGroupBytes);
        exclusiveScanCounts(ctx, dGroupBytes, dGroupStart, groups + 1, dTemp, scanTempBytes(groups + 1));
        hipLaunchKernelGGL(k_text_write, dim3((unsigned)groups), dim3(TEXT_GROUP_ROWS), 0, ctx.stream, chunk, (i64)n, sch, (const unsigned*)dRowLen,
                           (const u64*)dGroupStart, dText);
        RSQ_HIP(hipGetLastError());
        RSQ_HIP(hipEventRecord(w.ev[2], ctx.stream));
        uint64_t bytes = 0;
        RSQ_HIP(hipMemcpyAsync(&bytes, dGroupStart + groups, 8, hipMemcpyDeviceToHost, ctx.stream));
        RSQ_HIP(hipStreamSynchronize(ctx.stream));
        if (bytes > (uint64_t)(n * rowBound)) throw Error(RSQ_ERR_RUNTIME, "result text: a chunk's text is longer than its bound");
        if (bytes) RSQ_HIP(hipMemcpyAsync(w.pin, dText, (size_t)bytes, hipMemcpyDeviceToHost, ctx.stream));
        RSQ_HIP(hipEventRecord(w.ev[3], ctx.stream));
        RSQ_HIP(hipStreamSynchronize(ctx.stream));
        float ms = 0;
        if (!devTuples) { RSQ_HIP(hipEventElapsedTime(&ms, w.ev[0], w.ev[1])); rep.upload_ms += ms; }
        RSQ_HIP(hipEventElapsedTime(&ms, w.ev[1], w.ev[2])); rep.kernel_ms += ms;
        RSQ_HIP(hipEventElapsedTime(&ms, w.ev[2], w.ev[3])); rep.download_ms += ms;
        const auto t0 = std::chrono::steady_clock::now();
        out.append(w.pin, (size_t)bytes);
        rep.download_ms += msSince(t0);
        rep.text_bytes += (int64_t)bytes;
        rep.chunks++;
    }
    return true;
}

}  // namespace

void writeResultText(Context& ctx, const rsq_result_view& v, const uint8_t* devTuples, bool device, int64_t chunkRows, int64_t maxDeviceBytes, TextOut& out, rsq_result_text_report& rep) {
    const auto started = std::chrono::steady_clock::now();
    rep = rsq_result_text_report{};
    if (!device || !textOnDevice(ctx, v, devTuples, chunkRows, maxDeviceBytes, out, rep)) {
        // the host path: all of it (a device path gives up before it has written anything; its reason stays in the report)
        const std::string text = serializeResultView(v);
        out.append(text.data(), text.size());
        rep.path = 0; rep.rows = v.n_rows; rep.text_bytes = (int64_t)text.size();
    }
    rep.total_ms = msSince(started);
}

}  // namespace rsq
