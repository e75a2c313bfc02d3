// rowstore.h — how a field of a packed ReSQL tuple (reference src/schema.h:76-106: fields back to back, strings by value) becomes the
// cell of a column, for both sides: the host bridge (rowstore.cpp transposeRowstoreHost) and the device bridge (rowstore_device.hip).
//   layout   field i lies at the sum of sizeInTuple(type, true) of the fields in front of it:
//            BOOL 1, INT / DATE 4, BIGINT / DECIMAL 8, CHAR(1) 2, CHAR(n) / VARCHAR(n) n + 1
//   width    a cell has columnWidth(type) bytes: 1 / 4 / 8 / len
//   numeric  the cell is the field's first `width` bytes; a field lies at any byte offset, so it is copied as bytes
//   string   the cell is the field's bytes up to, and not including, its first NUL within len; every byte behind that is 0 - what lies
//            behind a NUL in the tuple never reaches the column.  CHAR(1) is this rule with len = 1.
// Compiled by hipcc for both sides and by g++ for the host alone (tests/cpp/rowstore_test.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "expr.h"

#if defined(__HIPCC__)
#define ROWST_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define ROWST_FN inline
#endif

namespace rsq {
namespace rowst {

enum Category { CAT_NUMERIC = 0, CAT_STRING = 1 };

// the cell of the field at `field`: all `width` bytes of it are written
ROWST_FN void cell(int category, int width, const unsigned char* field, unsigned char* dst) {
    if (category == CAT_STRING) {
        int c = 0;
        for (; c < width && field[c]; c++) dst[c] = field[c];
        for (; c < width; c++) dst[c] = 0;
    } else {
#if defined(__HIP_DEVICE_COMPILE__)
        for (int c = 0; c < width; c++) dst[c] = field[c];
#else
        memcpy(dst, field, (size_t)width);
#endif
    }
}

}  // namespace rowst

// a schema's tuple: every field's offset, its cell's width and category, and the tuple's size
struct RowstoreLayout {
    std::vector<int> offset, width, category;
    int tupleSize = 0;
};
// raises what sizeInTuple / columnWidth raise for a type no column holds (FLOAT: "unsupported column type")
RowstoreLayout rowstoreLayout(const std::vector<Type>& types);
// the tuples the blocks hold: content_size / tupleSize of each, a remainder of bytes is ignored
int64_t rowstoreRows(const size_t* contentSize, int32_t nBlocks, int tupleSize);
// the host bridge: cols[i] = column i of the n tuples, block after block
void transposeRowstoreHost(const std::vector<Type>& types, const uint8_t* const* blocks, const size_t* contentSize, int32_t nBlocks,
                           std::vector<std::vector<uint8_t>>& cols, int64_t& n);

}  // namespace rsq
