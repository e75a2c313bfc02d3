// order_limit.h — what ORDER BY ... LIMIT k over a materialisation shares between its sides (rsq_ctx_set_order_limit):
//   image    the first sort key's cell as an unsigned number in which "earlier in the requested order" is "larger" - the rule of
//            aot_kernels.hip topk_image: key ^ 2^63, complemented for ascending order.  The cell is read at its own width: 4 bytes
//            (INT, DATE: signed 32 bits, sign-extended - compareTyped's order, a DATE at or above 2^31 sorts as negative) or 8 bytes
//            (BIGINT, DECIMAL); a 4-byte cell is never read as 8.  The device selection (order_limit.hip) and the tests' host driver
//            call the same function.
//   tuples   rows [lo, hi) of struct-of-arrays columns at columnWidth packed into ReSQL tuples (strings by value, NUL terminated):
//            the loop of the materialisation's tail (tail.cpp), which runs it over all rows of the full path and over the candidate
//            columns of the device path.
// No HIP call: compiled by hipcc for both sides and by g++ for the host alone (tests/cpp/order_limit_test.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "hostref.h"

#if defined(__HIPCC__)
#define ORDLIM_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define ORDLIM_FN inline
#endif

namespace rsq {
namespace ordlim {

// `cell` is aligned to `width` (4 or 8): a column's cell
ORDLIM_FN uint64_t image(const void* cell, int width, bool desc) {
    const int64_t v = width == 4 ? (int64_t)*(const int32_t*)cell : *(const int64_t*)cell;
    const uint64_t u = (uint64_t)v ^ 0x8000000000000000ull;
    return desc ? u : ~u;
}

}  // namespace ordlim

// tuples[(r - lo) * tupleSize + offset of column c] = cell r of cols[c], for r in [lo, hi); the bytes of a tuple that no field covers
// are left as they are
inline void columnsToTuples(const std::vector<Type>& types, const uint8_t* const* cols, size_t lo, size_t hi, uint8_t* tuples, size_t tupleSize) {
    std::vector<char> strbuf;
    size_t off = 0;
    for (size_t c = 0; c < types.size(); c++) {
        const Type& t = types[c];
        const size_t w = (size_t)columnWidth(t);
        const uint8_t* src = cols[c];
        if (t.isString()) strbuf.assign(w + 1, 0);
        for (size_t r = lo; r < hi; r++) {
            uint8_t* dst = tuples + (r - lo) * tupleSize + off;
            if (t.isString()) {
                memcpy(strbuf.data(), src + r * w, w); strbuf[w] = 0;
                Val v; v.s = strbuf.data();
                storeValue(dst, v, t);
            } else memcpy(dst, src + r * w, w);      // same little-endian value widths as the packed tuple
        }
        off += (size_t)sizeInTuple(t, true);
    }
}

}  // namespace rsq
