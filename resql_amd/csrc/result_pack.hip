// result_pack.hip — a materialisation's output columns packed into ReSQL tuples on the device (rsq_ctx_set_result_pack, rsq_prim_pack_tuples).
// columnsToTuples (order_limit.h) over a zeroed buffer stays the definition of the tuples; the rule of a field is result_pack.h's, which
// both sides use.  One launch over all rows - the mirror image of k_rowstore_transpose (rowstore_device.hip):
//   k_pack_tuples   a workgroup takes R = min(256, PK_TILE_BYTES / tuple size) consecutive rows and assembles their tuples' byte span in an
//                   LDS tile, at the same position inside a 16-byte group as the span has in global memory: column by column the R cells
//                   read so that consecutive lanes load consecutive addresses - 1-, 4- and 8-byte cells one per lane, a string column's
//                   R x len bytes as one span, 16 bytes per lane between its ragged ends - and written into the tile as bytes or aligned
//                   words; then one lane per row clears every string field behind its first NUL, with the field's terminator and CHAR(1)'s
//                   second byte, so every byte of the span is defined; then the span is stored 16 bytes per lane
//                   a tuple longer than the tile (R = 0): one lane per (row, column), straight through global memory
// A row's byte offset in the output is 64-bit (rows x tuple size passes 2^32); offsets inside the tile are 32-bit.
#include <algorithm>

#include "engine.h"
#include "result_pack.h"

namespace rsq {

#define PK_LANES 256
#define PK_TILE_BYTES 49152           /* LDS tile: the span of a workgroup's tuples, as k_rowstore_transpose's */
#define PK_TILE_SLACK 32              /* the span starts up to 15 bytes into the tile and is stored in whole 16-byte groups */

// kind: PK_BYTES a cell of 1, 4 or 8 bytes, one per lane (fieldSize > width: zeros behind it - CHAR(1)); PK_STRING: the NUL rule over width bytes
enum { PK_BYTES = 0, PK_STRING = 1 };
struct PkCol { int32_t offset, width, fieldSize, kind; const unsigned char* ptr; };
struct PkSchema { int32_t nCols, tupleSize, groupRows, pad; PkCol col[rpack::MAX_COLUMNS]; };
#define PK_COLS_BYTES ((unsigned)(rpack::MAX_COLUMNS * sizeof(PkCol)))          /* a multiple of 16: the tile behind it stays 16-byte aligned */

// `width` (4 or 8) bytes at any byte address of the tile: aligned words where the address allows, bytes where it does not (never a
// misaligned wide store)
__device__ __forceinline__ void tile_store(unsigned char* tile, unsigned a, unsigned lo, unsigned hi, int width) {
    if ((a & 3u) == 0) {
        *(unsigned*)(tile + a) = lo;
        if (width == 8) *(unsigned*)(tile + a + 4u) = hi;
        return;
    }
#pragma unroll
    for (int s = 0; s < 4; s++) tile[a + (unsigned)s] = (unsigned char)(lo >> (8 * s));
    if (width == 8) {
#pragma unroll
        for (int s = 0; s < 4; s++) tile[a + 4u + (unsigned)s] = (unsigned char)(hi >> (8 * s));
    }
}

// tuples: nRows x sch.tupleSize bytes; sch.col[c].ptr: nRows cells of sch.col[c].width bytes.  Dynamic LDS: PK_COLS_BYTES, and where
// sch.groupRows > 0 the tile of groupRows x tupleSize + PK_TILE_SLACK bytes behind it.
__global__ void __launch_bounds__(PK_LANES) k_pack_tuples(unsigned char* __restrict__ tuples, int64_t nRows, PkSchema sch) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];
    PkCol* s_cols = (PkCol*)s_mem;
    unsigned char* s_tile = s_mem + PK_COLS_BYTES;
    const unsigned tid = threadIdx.x, ts = (unsigned)sch.tupleSize, nCols = (unsigned)sch.nCols;
    if (tid < nCols) s_cols[tid] = sch.col[tid];
    __syncthreads();
    if (sch.groupRows == 0) {          // (uniform) one tuple is longer than the tile: a lane per (row, column), straight through global memory
        const int64_t item = (int64_t)blockIdx.x * PK_LANES + tid;
        const int64_t row = item / (int64_t)nCols;
        if (row >= nRows) return;
        const PkCol col = s_cols[(unsigned)(item - row * (int64_t)nCols)];
        rpack::field(col.kind == PK_STRING ? rpack::CAT_STRING : rpack::CAT_NUMERIC, col.width, col.fieldSize, col.ptr + row * (int64_t)col.width,
                     tuples + row * (int64_t)ts + (unsigned)col.offset);
        return;
    }
    const unsigned R = (unsigned)sch.groupRows;
    const int64_t row0 = (int64_t)blockIdx.x * R;
    const unsigned nr = nRows - row0 < (int64_t)R ? (unsigned)(nRows - row0) : R;
    // the tuples' span: tile byte head + r * ts is row row0 + r's first, and tile byte p is dst[p - head]
    unsigned char* dst = tuples + row0 * (int64_t)ts;
    const unsigned head = (unsigned)((uintptr_t)dst & 15u), spanEnd = head + nr * ts;
    for (unsigned c = 0; c < nCols; c++) {
        const PkCol col = s_cols[c];
        if (col.kind == PK_BYTES) {
            if (tid < nr) {
                const unsigned a = head + tid * ts + (unsigned)col.offset;
                if (col.width == 4) tile_store(s_tile, a, ((const unsigned*)col.ptr)[row0 + tid], 0u, 4);
                else if (col.width == 8) { const uint2 v = ((const uint2*)col.ptr)[row0 + tid]; tile_store(s_tile, a, v.x, v.y, 8); }
                else s_tile[a] = col.ptr[row0 + tid];
            }
            continue;
        }
        // a string column: the nr x len bytes of its rows are one span of the column.  Span byte j is byte j % len of row j / len.  The span
        // begins and ends at any byte and nothing outside it may be loaded (the column's allocation may end with it): whole 16-byte groups
        // are loaded only where all 16 bytes are the span's.  q = a + j: the byte's position counted from the 16-byte boundary in front of src.
        const unsigned len = (unsigned)col.width, span = nr * len;
        if (span == 0) continue;
        const unsigned char* src = col.ptr + row0 * (int64_t)len;
        unsigned char* field0 = s_tile + head + (unsigned)col.offset;
        const unsigned a = (unsigned)((uintptr_t)src & 15u), b = a + span;
        const unsigned fullBegin = (a + 15u) & ~15u, fullEnd = b & ~15u;
        const unsigned headEnd = fullBegin < b ? fullBegin : b;                 // [a, headEnd): the partial group at the head
        const unsigned tailBegin = fullEnd > headEnd ? fullEnd : headEnd;       // [tailBegin, b): ... and at the tail
        for (unsigned q = fullBegin + tid * 16u; q < fullEnd; q += PK_LANES * 16u) {
            const unsigned j = q - a;
            const uint4 v = *(const uint4*)(src + j);
            const unsigned w[4] = {v.x, v.y, v.z, v.w};
            unsigned r = j / len, k = j - r * len;
            unsigned char* f = field0 + r * ts;
#pragma unroll
            for (int i = 0; i < 4; i++) {
#pragma unroll
                for (int s = 0; s < 4; s++) {
                    f[k] = (unsigned char)(w[i] >> (8 * s));
                    if (++k == len) { k = 0; f += ts; }
                }
            }
        }
        if (tid < headEnd - a) { const unsigned j = tid, r = j / len; field0[r * ts + (j - r * len)] = src[j]; }
        if (tid >= 64u && tid - 64u < b - tailBegin) { const unsigned j = tailBegin - a + (tid - 64u), r = j / len; field0[r * ts + (j - r * len)] = src[j]; }
    }
    __syncthreads();
    // what no cell covers, in place: a string field behind its first NUL and its terminator, CHAR(1)'s second byte
    if (tid < nr) {
        for (unsigned c = 0; c < nCols; c++) {
            unsigned char* f = s_tile + head + tid * ts + (unsigned)s_cols[c].offset;
            int k = s_cols[c].width;
            if (s_cols[c].kind == PK_STRING) { k = 0; while (k < s_cols[c].width && f[k]) k++; }
            for (; k < s_cols[c].fieldSize; k++) f[k] = 0;
        }
    }
    __syncthreads();
    // the span out: its neighbours on either side are other workgroups', so whole 16-byte groups are stored only where all 16 bytes are
    // this workgroup's (as k_text_write does)
    const unsigned a = head, b = spanEnd;
    const unsigned fullBegin = (a + 15u) & ~15u, fullEnd = b & ~15u;
    const unsigned headEnd = fullBegin < b ? fullBegin : b;
    const unsigned tailBegin = fullEnd > headEnd ? fullEnd : headEnd;
    for (unsigned p = fullBegin + tid * 16u; p < fullEnd; p += PK_LANES * 16u) *(uint4*)(dst + (p - a)) = *(const uint4*)(s_tile + p);
    if (tid < headEnd - a) dst[tid] = s_tile[a + tid];
    if (tid >= 64u && tid - 64u < b - tailBegin) dst[tailBegin - a + (tid - 64u)] = s_tile[tailBegin + (tid - 64u)];
}

int packTupleSize(const std::vector<Type>& types) {
    int64_t ts = 0;
    for (const Type& t : types) ts += sizeInTuple(t, true);
    if (ts > 0x7fffffffll) failInvalid("a tuple of " + std::to_string((long long)ts) + " bytes is longer than a packed relation's may be");
    return (int)ts;
}

void packTuples(Context& ctx, const std::vector<Type>& types, const void* const* dCols, int64_t nRows, uint8_t* dTuples) {
    if (types.empty() || types.size() > (size_t)rpack::MAX_COLUMNS) failInvalid("packTuples: 1 to " + std::to_string((int)rpack::MAX_COLUMNS) + " columns");
    if (nRows < 0 || nRows >= ((int64_t)1 << 32)) failInvalid("packTuples: row numbers are 32 bits");
    PkSchema sch{};
    const int ts = packTupleSize(types);
    sch.nCols = (int32_t)types.size(); sch.tupleSize = ts;
    sch.groupRows = ts <= PK_TILE_BYTES ? (int32_t)std::min<int64_t>(PK_LANES, PK_TILE_BYTES / ts) : 0;
    int off = 0;
    for (size_t c = 0; c < types.size(); c++) {
        PkCol& pc = sch.col[c];
        pc.offset = off; pc.width = columnWidth(types[c]); pc.fieldSize = sizeInTuple(types[c], true);
        pc.kind = types[c].isString() ? PK_STRING : PK_BYTES;
        // (the kernel trusts these: a BYTES cell is loaded at its width, a field ends inside its tuple)
        if (pc.width < 0 || pc.fieldSize < pc.width || (pc.kind == PK_BYTES && pc.width != 1 && pc.width != 4 && pc.width != 8) ||
            (pc.kind == PK_STRING && pc.fieldSize != pc.width + 1))
            failRuntime("internal error: packTuples met a column of " + std::to_string(pc.width) + " bytes in a field of " + std::to_string(pc.fieldSize));
        pc.ptr = (const unsigned char*)dCols[c];
        off += pc.fieldSize;
    }
    if (nRows == 0) return;
    const int64_t groups = sch.groupRows ? (nRows + sch.groupRows - 1) / sch.groupRows : (nRows * sch.nCols + PK_LANES - 1) / PK_LANES;
    if (groups > 0x7fffffffll) failInvalid("packTuples: more workgroups than a launch takes");
    const size_t lds = PK_COLS_BYTES + (sch.groupRows ? (((size_t)sch.groupRows * (size_t)ts + 15) & ~(size_t)15) + PK_TILE_SLACK : 0);
    hipLaunchKernelGGL(k_pack_tuples, dim3((unsigned)groups), dim3(PK_LANES), lds, ctx.stream, (unsigned char*)dTuples, nRows, sch);
    RSQ_HIP(hipGetLastError());
}

}  // namespace rsq
