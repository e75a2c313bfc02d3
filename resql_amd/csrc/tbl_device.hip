// tbl_device.hip — BULK INSERT's '.tbl' text parsed on the device (rsq_config.tbl_ingest = 1, rsq_table_load_tbl_ex).
// The file is streamed into device memory as it is; three kernels turn it into columns:
//   k_tbl_count_lines   '\n' per TBL_BLOCK_BYTES of text            -> exclusiveScanCounts: the row number of every block's first line start
//   k_tbl_line_starts   lineStart[row] for every row                (a newline at p starts row base + rank + 1 at p + 1)
//   k_tbl_parse         one lane per line, TBL_GROUP_LINES per workgroup: the workgroup's text span staged in LDS, every field parsed
//                       by the plain forms of tbl_fields.h and stored into its column cell
// A line with a field outside those forms, with another field count than the table has columns, or with a NUL is ODD: its lane appends
// (row, offset, length) to a list and the host parses it with tblParseLine (tbl.h) - the host path's own line function - which fills
// the row or raises the host path's error.  The device itself never reports an error.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstring>

#include "engine.h"
#include "scan_device.h"
#include "tbl_fields.h"

namespace rsq {

#define TBL_BLOCK_BYTES 4096          /* text per workgroup of the two line passes: 256 lanes x 16 B */
#define TBL_GROUP_LINES 256           /* lines per workgroup of the parse */
#define TBL_TILE_BYTES 49152          /* LDS tile of the parse: a span of 256 lines of up to 192 B on average (TPC-H lineitem: 125 B, customer: 160 B);
                                         three workgroups per CU */
#define TBL_MAX_COLS 64
#define TBL_MAX_ODD 65536

struct TblCol { int32_t category, width; void* ptr; };
struct TblSchema { int32_t nCols, terminator, endsInNewline, pad; TblCol col[TBL_MAX_COLS]; };
struct TblOdd { i64 row, start, len; };

// the '\n' among the 16 bytes at `off` (a multiple of 16 inside the padded buffer), one bit each; bytes at or beyond `size` are masked
__device__ __forceinline__ unsigned newline_mask(const unsigned char* __restrict__ text, i64 off, i64 size) {
    if (off >= size) return 0u;
    const uint4 v = *(const uint4*)(text + off);
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    unsigned m = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
#pragma unroll
        for (int b = 0; b < 4; b++) m |= (((w[k] >> (8 * b)) & 0xffu) == (unsigned)'\n' ? 1u : 0u) << (4 * k + b);
    }
    const i64 left = size - off;
    return left < 16 ? m & ((1u << (int)left) - 1u) : m;
}

__global__ void __launch_bounds__(256) k_tbl_count_lines(const unsigned char* __restrict__ text, i64 size, unsigned* __restrict__ counts) {
    __shared__ unsigned s_wave[4];
    const i64 off = (i64)blockIdx.x * TBL_BLOCK_BYTES + (i64)threadIdx.x * 16;
    unsigned total;
    block_scan<256, unsigned, ScanSum>((unsigned)__popc(newline_mask(text, off, size)), s_wave, &total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// base[block]: newlines in front of the block.  lineStart has nRows + 1 entries: row 0 starts at 0, lineStart[nRows] = size.
__global__ void __launch_bounds__(256) k_tbl_line_starts(const unsigned char* __restrict__ text, i64 size, const u64* __restrict__ base, i64 nRows,
                                                         i64* __restrict__ lineStart) {
    __shared__ unsigned s_wave[4];
    const i64 off = (i64)blockIdx.x * TBL_BLOCK_BYTES + (i64)threadIdx.x * 16;
    unsigned m = newline_mask(text, off, size);
    unsigned total;
    const unsigned rank = block_scan<256, unsigned, ScanSum>((unsigned)__popc(m), s_wave, &total);
    i64 row = (i64)base[blockIdx.x] + rank + 1;
    while (m) {
        const int b = __ffs((int)m) - 1;
        m &= m - 1;
        if (row <= nRows) lineStart[row] = off + b + 1;          // (the file's last '\n' writes lineStart[nRows] = size)
        row++;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { lineStart[0] = 0; lineStart[nRows] = size; }
}

// one line; false: the line is odd.  Cells of fields in front of an odd one may have been written: the host patches every cell of the row.
__device__ __forceinline__ bool parse_line(const unsigned char* line, int len, const TblCol* cols, int nCols, unsigned char terminator, i64 row) {
    int pos = 0, begin, flen, att = 0;
    while (tblf::nextField(line, len, terminator, &pos, &begin, &flen)) {
        if (att >= nCols) return false;
        const TblCol c = cols[att];
        const unsigned char* f = line + begin;
        bool ok;
        switch (c.category) {
            case tblf::CAT_INT: { int32_t v; ok = tblf::plainInt(f, flen, &v); if (ok) ((int32_t*)c.ptr)[row] = v; break; }
            case tblf::CAT_BIGINT: { int64_t v; ok = tblf::plainBigint(f, flen, &v); if (ok) ((int64_t*)c.ptr)[row] = v; break; }
            case tblf::CAT_DECIMAL: { int64_t v; ok = tblf::plainDecimal(f, flen, &v); if (ok) ((int64_t*)c.ptr)[row] = v; break; }
            case tblf::CAT_DATE: { uint32_t v; ok = tblf::plainDate(f, flen, &v); if (ok) ((uint32_t*)c.ptr)[row] = v; break; }
            case tblf::CAT_BOOL: { uint8_t v; ok = tblf::plainBool(f, flen, &v); if (ok) ((uint8_t*)c.ptr)[row] = v; break; }
            default: ok = tblf::plainString(f, flen, (uint8_t*)c.ptr + row * (i64)c.width, c.width); break;
        }
        if (!ok) return false;
        att++;
    }
    return att == nCols;
}

// odd[0] = number of odd lines met, odd[1] = 1 when the list overflowed
__global__ void __launch_bounds__(TBL_GROUP_LINES) k_tbl_parse(const unsigned char* __restrict__ text, const i64* __restrict__ lineStart, i64 nRows, TblSchema sch,
                                                               unsigned* __restrict__ oddCount, TblOdd* __restrict__ oddList) {
    __shared__ __attribute__((aligned(16))) unsigned char s_tile[TBL_TILE_BYTES];
    __shared__ TblCol s_cols[TBL_MAX_COLS];
    const i64 r0 = (i64)blockIdx.x * TBL_GROUP_LINES;
    const i64 r1 = r0 + TBL_GROUP_LINES < nRows ? r0 + TBL_GROUP_LINES : nRows;
    if ((int)threadIdx.x < sch.nCols) s_cols[threadIdx.x] = sch.col[threadIdx.x];
    // the workgroup's span of text, from the 16-byte boundary in front of it: into LDS when it fits the tile
    const i64 spanEnd = lineStart[r1];
    const i64 tileBegin = lineStart[r0] & ~15ll;
    const bool staged = spanEnd - tileBegin <= TBL_TILE_BYTES;
    if (staged)
        for (i64 o = tileBegin + (i64)threadIdx.x * 16; o < spanEnd; o += TBL_GROUP_LINES * 16) *(uint4*)(s_tile + (o - tileBegin)) = *(const uint4*)(text + o);
    __syncthreads();
    const i64 row = r0 + threadIdx.x;
    if (row >= r1) return;
    const i64 start = lineStart[row];
    const i64 len = lineStart[row + 1] - start - ((row + 1 < nRows || sch.endsInNewline) ? 1 : 0);
    bool ok = len <= 0x3fffffffll;
    if (ok) {
        if (staged) ok = parse_line(s_tile + (start - tileBegin), (int)len, s_cols, sch.nCols, (unsigned char)sch.terminator, row);
        else ok = parse_line(text + start, (int)len, s_cols, sch.nCols, (unsigned char)sch.terminator, row);
    }
    if (!ok) {
        const unsigned slot = atomicAdd(&oddCount[0], 1u);
        if (slot < TBL_MAX_ODD) { TblOdd o; o.row = row; o.start = start; o.len = len; oddList[slot] = o; }
        else oddCount[1] = 1u;
    }
}

// the cells of the odd rows of one column, as the host parsed them: cells[i] -> row rows[i]
__global__ void __launch_bounds__(256) k_tbl_patch(const i64* __restrict__ rows, int n, const unsigned char* __restrict__ cells, int width, unsigned char* __restrict__ col) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    unsigned char* dst = col + rows[i] * (i64)width;
    for (int b = 0; b < width; b++) dst[b] = cells[(i64)i * width + b];
}

namespace {

double msSince(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// everything the load holds besides the table: given back however the load ends
struct TblWork {
    Context& ctx;
    int fd = -1;
    void* pin[2] = {nullptr, nullptr};
    hipEvent_t ev[8] = {};
    std::vector<void*> dev;
    explicit TblWork(Context& c) : ctx(c) {}
    void* raw(size_t bytes) { void* p = ctx.allocRaw(bytes); dev.push_back(p); return p; }
    ~TblWork() {
        (void)hipStreamSynchronize(ctx.stream);
        if (fd >= 0) ::close(fd);
        for (void* p : pin) ctx.freePinned(p);
        for (hipEvent_t e : ev) ctx.giveEvent(e);
        for (void* p : dev) ctx.freeRaw(p);
    }
};

int categoryOf(const Type& t) {
    switch (t.tag) {
        case RSQ_INT: return tblf::CAT_INT;
        case RSQ_BIGINT: return tblf::CAT_BIGINT;
        case RSQ_DECIMAL: return tblf::CAT_DECIMAL;
        case RSQ_DATE: return tblf::CAT_DATE;
        case RSQ_BOOL: return tblf::CAT_BOOL;
        default: return tblf::CAT_STRING;          // (columnWidth has refused every other type)
    }
}

}  // namespace

std::unique_ptr<Table> loadTblDevice(Context& ctx, const rsq_table_desc& schema, const std::vector<Type>& types, const std::string& path,
                                     char terminator, int64_t chunkBytes, int64_t maxDeviceBytes, rsq_tbl_load_report& rep) {
    auto fallback = [&](int why) { rep.fallback_reason = why; return std::unique_ptr<Table>(); };
    if (ctx.device < 0) return fallback(RSQ_TBL_FALLBACK_NO_DEVICE);
    if (types.size() > TBL_MAX_COLS) return fallback(RSQ_TBL_FALLBACK_COLUMNS);
    if (terminator == '\n' || terminator == '\0') return fallback(RSQ_TBL_FALLBACK_TERMINATOR);
    TblSchema sch{};
    sch.nCols = (int32_t)types.size(); sch.terminator = (unsigned char)terminator;
    size_t rowBytes = 0;
    for (size_t i = 0; i < types.size(); i++) {
        sch.col[i].width = columnWidth(types[i]); sch.col[i].category = categoryOf(types[i]);
        rowBytes += (size_t)sch.col[i].width;
    }
    RSQ_HIP(hipSetDevice(ctx.device));
    TblWork w(ctx);
    w.fd = ::open(path.c_str(), O_RDONLY);
    struct stat st;
    if (w.fd < 0 || fstat(w.fd, &st) != 0 || !S_ISREG(st.st_mode)) throw Error(RSQ_ERR_INVALID, "Could not open file " + path);
    const int64_t size = (int64_t)st.st_size;
    rep.text_bytes = size;

    // ---- what the load takes on the device while it runs ----
    size_t limit = (size_t)maxDeviceBytes;
    if (maxDeviceBytes == 0) {
        size_t freeBytes = 0, totalBytes = 0;
        RSQ_HIP(hipMemGetInfo(&freeBytes, &totalBytes));
        limit = freeBytes > ((size_t)1 << 30) ? freeBytes - ((size_t)1 << 30) : 0;
    }
    const size_t padded = (((size_t)size + 15) & ~(size_t)15) + 16;
    const int64_t nBlocks = (size + TBL_BLOCK_BYTES - 1) / TBL_BLOCK_BYTES;
    const size_t scanBytes = (size_t)(nBlocks + 1) * 12 + scanTempBytes(nBlocks + 1);
    const size_t oddBytes = 16 + (size_t)TBL_MAX_ODD * sizeof(TblOdd);
    if (padded + scanBytes + oddBytes > limit) return fallback(RSQ_TBL_FALLBACK_DOES_NOT_FIT);

    // ---- the text: two pinned buffers in turn, reading piece k + 1 while piece k is on its way ----
    unsigned char* dText = (unsigned char*)w.raw(padded);
    const size_t chunk = (size_t)std::max<int64_t>(64, std::min<int64_t>(chunkBytes ? chunkBytes : (int64_t)64 << 20, size));
    for (auto& e : w.ev) e = ctx.takeEvent();
    unsigned char lastByte = '\n';
    if (size > 0) {
        for (auto& p : w.pin) p = ctx.allocPinned(chunk);
        int k = 0;
        for (int64_t off = 0; off < size; k++) {
            const int b = k & 1;
            if (k >= 2) { auto t0 = std::chrono::steady_clock::now(); RSQ_HIP(hipEventSynchronize(w.ev[b])); rep.copy_ms += msSince(t0); }
            const size_t want = (size_t)std::min<int64_t>((int64_t)chunk, size - off);
            auto t0 = std::chrono::steady_clock::now();
            for (size_t got = 0; got < want;) {
                const ssize_t r = pread(w.fd, (char*)w.pin[b] + got, want - got, (off_t)(off + (int64_t)got));
                if (r <= 0) throw Error(RSQ_ERR_INVALID, "Could not read file " + path);
                got += (size_t)r;
            }
            rep.read_ms += msSince(t0);
            lastByte = ((const unsigned char*)w.pin[b])[want - 1];
            RSQ_HIP(hipMemcpyAsync(dText + off, w.pin[b], want, hipMemcpyHostToDevice, ctx.stream));
            RSQ_HIP(hipEventRecord(w.ev[b], ctx.stream));
            off += (int64_t)want;
        }
    }
    RSQ_HIP(hipMemsetAsync(dText + size, 0, padded - (size_t)size, ctx.stream));
    {
        auto t0 = std::chrono::steady_clock::now();
        RSQ_HIP(hipStreamSynchronize(ctx.stream));
        rep.copy_ms += msSince(t0);
    }

    // ---- lines ----
    int64_t nRows = 0;
    uint64_t* dBase = nullptr;
    if (size > 0) {
        uint32_t* dCounts = (uint32_t*)w.raw((size_t)(nBlocks + 1) * 4);
        dBase = (uint64_t*)w.raw((size_t)(nBlocks + 1) * 8);
        void* dTemp = w.raw(scanTempBytes(nBlocks + 1));
        RSQ_HIP(hipMemsetAsync(dCounts + nBlocks, 0, 4, ctx.stream));          // (the trailing slot: dBase[nBlocks] = all newlines)
        RSQ_HIP(hipEventRecord(w.ev[2], ctx.stream));
        hipLaunchKernelGGL(k_tbl_count_lines, dim3((unsigned)nBlocks), dim3(256), 0, ctx.stream, (const unsigned char*)dText, (i64)size, (unsigned*)dCounts);
        exclusiveScanCounts(ctx, dCounts, dBase, nBlocks + 1, dTemp, scanTempBytes(nBlocks + 1));
        RSQ_HIP(hipEventRecord(w.ev[3], ctx.stream));
        uint64_t newlines = 0;
        RSQ_HIP(hipMemcpyAsync(&newlines, dBase + nBlocks, 8, hipMemcpyDeviceToHost, ctx.stream));
        RSQ_HIP(hipStreamSynchronize(ctx.stream));
        nRows = (int64_t)newlines + (lastByte != '\n' ? 1 : 0);          // std::getline: a last line without '\n' still counts
    }
    rep.rows = nRows;
    if (padded + scanBytes + oddBytes + (size_t)(nRows + 1) * 8 + (size_t)nRows * rowBytes > limit) return fallback(RSQ_TBL_FALLBACK_DOES_NOT_FIT);

    // ---- the table: columns zero-filled, as the cells of the host path are ----
    std::unique_ptr<Table> t(new Table());
    t->ctx = &ctx;
    t->name = std::string(schema.name, strnlen(schema.name, RSQ_SYMBOL_MAX));
    t->nRows = nRows;
    for (size_t i = 0; i < types.size(); i++) {
        TableColumn tc;
        tc.name = std::string(schema.cols[i].name, strnlen(schema.cols[i].name, RSQ_SYMBOL_MAX));
        tc.type = types[i];
        const size_t bytes = (size_t)nRows * (size_t)sch.col[i].width;
        tc.dptr = ctx.allocRaw(bytes); tc.owned = true;
        t->cols.push_back(tc);
        if (bytes) RSQ_HIP(hipMemsetAsync(tc.dptr, 0, bytes, ctx.stream));
        sch.col[i].ptr = tc.dptr;
    }
    if (nRows == 0) { rep.path = 1; return t; }

    // ---- line starts, parse ----
    i64* dStarts = (i64*)w.raw((size_t)(nRows + 1) * 8);
    unsigned* dOddCount = (unsigned*)w.raw(oddBytes);
    TblOdd* dOddList = (TblOdd*)((char*)dOddCount + 16);
    RSQ_HIP(hipMemsetAsync(dOddCount, 0, 16, ctx.stream));
    sch.endsInNewline = lastByte == '\n' ? 1 : 0;
    RSQ_HIP(hipEventRecord(w.ev[4], ctx.stream));
    hipLaunchKernelGGL(k_tbl_line_starts, dim3((unsigned)nBlocks), dim3(256), 0, ctx.stream, (const unsigned char*)dText, (i64)size, (const u64*)dBase, (i64)nRows, dStarts);
    RSQ_HIP(hipEventRecord(w.ev[5], ctx.stream));
    const int64_t nGroups = (nRows + TBL_GROUP_LINES - 1) / TBL_GROUP_LINES;
    hipLaunchKernelGGL(k_tbl_parse, dim3((unsigned)nGroups), dim3(TBL_GROUP_LINES), 0, ctx.stream, (const unsigned char*)dText, (const i64*)dStarts, (i64)nRows, sch,
                       dOddCount, dOddList);
    RSQ_HIP(hipEventRecord(w.ev[6], ctx.stream));
    RSQ_HIP(hipGetLastError());
    unsigned odd[2] = {0, 0};
    RSQ_HIP(hipMemcpyAsync(odd, dOddCount, 8, hipMemcpyDeviceToHost, ctx.stream));
    RSQ_HIP(hipStreamSynchronize(ctx.stream));
    float ms = 0;
    RSQ_HIP(hipEventElapsedTime(&ms, w.ev[2], w.ev[3])); rep.count_kernel_ms = ms;
    RSQ_HIP(hipEventElapsedTime(&ms, w.ev[4], w.ev[5])); rep.starts_kernel_ms = ms;
    RSQ_HIP(hipEventElapsedTime(&ms, w.ev[5], w.ev[6])); rep.parse_kernel_ms = ms;
    rep.kernel_ms = rep.count_kernel_ms + rep.starts_kernel_ms + rep.parse_kernel_ms;
    if (odd[1] || odd[0] > TBL_MAX_ODD) return fallback(RSQ_TBL_FALLBACK_ODD_LINES);

    // ---- odd lines: the host's line function, in line order (the smallest bad line number wins, as in parseTblFile) ----
    if (odd[0]) {
        auto t0 = std::chrono::steady_clock::now();
        const size_t n = odd[0];
        std::vector<TblOdd> list(n);
        RSQ_HIP(hipMemcpy(list.data(), dOddList, n * sizeof(TblOdd), hipMemcpyDeviceToHost));
        std::sort(list.begin(), list.end(), [](const TblOdd& a, const TblOdd& b) { return a.row < b.row; });
        std::vector<std::vector<uint8_t>> cells(types.size());
        for (size_t c = 0; c < types.size(); c++) cells[c].assign(n * (size_t)sch.col[c].width, 0);
        std::vector<int64_t> rows(n);
        std::vector<uint8_t*> cell(types.size());
        std::vector<char> line;
        std::string what;
        for (size_t k = 0; k < n; k++) {
            rows[k] = list[k].row;
            const size_t len = (size_t)list[k].len;
            line.assign(len + 1, '\0');
            for (size_t got = 0; got < len;) {
                const ssize_t r = pread(w.fd, line.data() + got, len - got, (off_t)(list[k].start + (int64_t)got));
                if (r <= 0) throw Error(RSQ_ERR_INVALID, "Could not read file " + path);
                got += (size_t)r;
            }
            for (size_t c = 0; c < types.size(); c++) cell[c] = cells[c].data() + k * (size_t)sch.col[c].width;
            if (tblParseLine(types, line.data(), len, terminator, cell.data(), what))
                throw Error(RSQ_ERR_INVALID, "Line " + std::to_string(list[k].row) + " in " + path + " " + what);
        }
        size_t widest = 1;
        for (size_t c = 0; c < types.size(); c++) widest = std::max(widest, (size_t)sch.col[c].width);
        i64* dRows = (i64*)w.raw(n * 8);
        unsigned char* dCells = (unsigned char*)w.raw(n * widest);
        RSQ_HIP(hipMemcpyAsync(dRows, rows.data(), n * 8, hipMemcpyHostToDevice, ctx.stream));
        for (size_t c = 0; c < types.size(); c++) {
            if (cells[c].empty()) continue;
            RSQ_HIP(hipMemcpyAsync(dCells, cells[c].data(), cells[c].size(), hipMemcpyHostToDevice, ctx.stream));
            hipLaunchKernelGGL(k_tbl_patch, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx.stream, (const i64*)dRows, (int)n, (const unsigned char*)dCells,
                               sch.col[c].width, (unsigned char*)sch.col[c].ptr);
        }
        RSQ_HIP(hipGetLastError());
        RSQ_HIP(hipStreamSynchronize(ctx.stream));
        rep.lines_patched = (int64_t)n;
        rep.patch_ms = msSince(t0);
    }
    rep.path = 1;
    return t;
}

}  // namespace rsq
