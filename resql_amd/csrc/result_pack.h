// result_pack.h — how the cell of a column becomes a field of a packed ReSQL tuple (reference src/schema.h:76-106: fields back to back,
// strings by value), for both sides of rsq_ctx_set_result_pack: the device tail of a materialisation (result_pack.hip k_pack_tuples) and
// the tests' host driver.  columnsToTuples (order_limit.h) over a zeroed buffer, through storeValue, stays the definition of the bytes;
// this header is held against it (tests/cpp/result_pack_test.cpp).  It is rowstore.h read backwards:
//   layout   field c lies at the sum of sizeInTuple(type, true) of the fields in front of it:
//            BOOL 1, INT / DATE 4, BIGINT / DECIMAL 8, CHAR(1) 2, CHAR(n) / VARCHAR(n) n + 1
//   numeric  BOOL / INT / DATE / BIGINT / DECIMAL: the field is the cell's columnWidth bytes
//   CHAR(1)  the cell's byte, then 0
//   string   CHAR(n) / VARCHAR(n), a field of n + 1 bytes: the cell's bytes up to, and not including, its first NUL within n; every byte
//            behind that is 0 - what lies behind a NUL in the column never reaches the tuple
// Every byte of a tuple belongs to one field and every byte of a field is written: a packed relation needs no memset.
// Also here: whether a relation is packed on the device at all (fitsDevice) - pure, so that the host driver can stand at its edges.
// No HIP call: compiled by hipcc for both sides and by g++ for the host alone.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define RPACK_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define RPACK_FN inline
#endif

namespace rsq {
namespace rpack {

enum Category { CAT_NUMERIC = 0, CAT_STRING = 1 };

enum { MAX_COLUMNS = 64 };                                            // materialised columns the device path takes
constexpr int64_t MAX_TUPLE_BYTES = (int64_t)2 << 30;                  // rows x tuple size it takes: one device buffer, one pinned buffer, one copy
constexpr int64_t DEVICE_SPARE_BYTES = (int64_t)1 << 30;               // what stays free on the device behind the tuples

// the field of `fieldSize` bytes at dst from the cell of `width` bytes: all fieldSize bytes are written.
// CAT_NUMERIC: the cell's bytes, zeros behind them (fieldSize > width is CHAR(1)'s second byte); CAT_STRING: the NUL rule, fieldSize = width + 1
RPACK_FN void field(int category, int width, int fieldSize, const unsigned char* cell, unsigned char* dst) {
    int c = 0;
    if (category == CAT_STRING) {
        for (; c < width && cell[c]; c++) dst[c] = cell[c];
    } else {
#if defined(__HIP_DEVICE_COMPILE__)
        for (; c < width; c++) dst[c] = cell[c];
#else
        memcpy(dst, cell, (size_t)width); c = width;
#endif
    }
    for (; c < fieldSize; c++) dst[c] = 0;
}

// Does a relation of `rows` tuples of `tupleSize` bytes go through the device path, with freeDeviceBytes free on the device before
// anything is allocated for it?  Row numbers are 32 bits, the tuples stay at or below MAX_TUPLE_BYTES and leave DEVICE_SPARE_BYTES free.
inline bool fitsDevice(int64_t rows, int64_t tupleSize, int64_t freeDeviceBytes) {
    if (rows < 0 || tupleSize <= 0 || rows >= ((int64_t)1 << 32)) return false;
    if (rows > MAX_TUPLE_BYTES / tupleSize) return false;            // (rows x tupleSize > MAX_TUPLE_BYTES, without forming the product)
    return rows * tupleSize <= freeDeviceBytes - DEVICE_SPARE_BYTES;
}

}  // namespace rpack
}  // namespace rsq
