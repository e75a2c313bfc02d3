// order_sort.h — what ORDER BY over a materialisation shares between its sides (rsq_ctx_set_order_sort): the device sort
// (order_sort.hip), the engine's decision (engine.cpp orderSortOnDevice) and the tests' host driver (tests/cpp/order_sort_test.cpp).
//   image    a key cell as an unsigned number in which "earlier in the requested order" is "smaller": ~ordlim::image.  The cell is read
//            at its own width - 4 bytes (INT, DATE: signed 32 bits, sign-extended, compareTyped's order) or 8 (BIGINT, DECIMAL).
//   layout   from the minimum and maximum image of every key: key j takes bits_j = 64 - clz(max_j - min_j) bits (a constant key none);
//            the keys' (image - min) are concatenated, first key most significant, into one bit string, which is cut into 64-bit
//            words from its least significant end.  Word 0 is the least significant: an LSD radix sort takes the words in that order.
//            A key lies in one word or straddles two: a word is made of at most MAX_KEYS pieces.
//   word     the w-th word of a row from its keys' images
//   fits     whether an execution's buffers fit the device (RSQ_ORDER_SORT_FALLBACK_DOES_NOT_FIT), asked before anything is allocated
// No HIP call: compiled by hipcc for both sides and by g++ for the host alone.
#pragma once

#include <cstddef>
#include <cstdint>

#include "order_limit.h"
#include "result_pack.h"

#if defined(__HIPCC__)
#define OSORT_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define OSORT_FN inline
#endif

namespace rsq {
namespace osort {

enum { MAX_KEYS = 8, MAX_WORDS = 8 };          // 8 keys of 64 bits are 8 words

// `cell` is aligned to `width` (4 or 8): a column's cell
OSORT_FN uint64_t image(const void* cell, int width, bool desc) { return ~ordlim::image(cell, width, desc); }

// bits [srcShift, srcShift + bits) of key `key`'s (image - min) lie at bits [dstShift, dstShift + bits) of the word
struct Piece { int32_t key, srcShift, dstShift, bits; };
struct Word { int32_t bits, nPieces; Piece piece[MAX_KEYS]; };
struct Layout {
    int32_t nKeys, totalBits, nWords, pad;
    int32_t bits[MAX_KEYS];
    uint64_t min[MAX_KEYS];
    Word word[MAX_WORDS];
};

OSORT_FN uint64_t lowMask(int bits) { return bits >= 64 ? ~0ull : ((1ull << bits) - 1ull); }

inline int bitsOf(uint64_t span) {          // 64 - clz(span); 0 for 0
    int b = 0;
    while (span) { b++; span >>= 1; }
    return b;
}

// mins[j] <= maxs[j]: the least and greatest image of key j over the rows; 1 <= nKeys <= MAX_KEYS
inline Layout layoutOf(const uint64_t* mins, const uint64_t* maxs, int nKeys) {
    Layout L{};
    L.nKeys = nKeys;
    int pos = 0;          // bits of the string below the key being placed
    for (int j = nKeys - 1; j >= 0; j--) {
        L.min[j] = mins[j];
        const int b = bitsOf(maxs[j] - mins[j]);
        L.bits[j] = b;
        int taken = 0;
        while (taken < b) {
            const int w = (pos + taken) / 64, at = (pos + taken) % 64;
            const int n = b - taken < 64 - at ? b - taken : 64 - at;
            Word& W = L.word[w];
            W.piece[W.nPieces++] = Piece{j, taken, at, n};
            W.bits = at + n;
            taken += n;
        }
        pos += b;
    }
    L.totalBits = pos;
    L.nWords = (pos + 63) / 64;
    return L;
}

// the word of a row whose keys' images are images[0 .. nKeys)
OSORT_FN uint64_t wordOf(const Word& W, const uint64_t* mins, const uint64_t* images) {
    uint64_t v = 0;
    for (int p = 0; p < W.nPieces; p++) {
        const Piece& pc = W.piece[p];
        v |= (((images[pc.key] - mins[pc.key]) >> pc.srcShift) & lowMask(pc.bits)) << pc.dstShift;
    }
    return v;
}

// radix passes of 8 bits the words take (radixSortPairs sorts whole digits)
inline int passesOf(const Layout& L) {
    int p = 0;
    for (int w = 0; w < L.nWords; w++) p += (L.word[w].bits + 7) / 8;
    return p;
}

// device memory of an execution over `rows` rows of which outRows come back, tuples of tupleSize bytes: two key arrays, two
// permutations, the sort's temporary (sortTempBytes: radixSortTempBytes(rows)), the scan-order tuples and the ordered tuples, each
// rounded up to 256 bytes
inline int64_t deviceBytes(int64_t rows, int64_t outRows, int64_t tupleSize, int64_t sortTempBytes) {
    auto up = [](int64_t b) { return (b + 255) & ~(int64_t)255; };
    return 2 * up(rows * 8) + 2 * up(rows * 4) + up(sortTempBytes) + up(rows * tupleSize) + up(outRows * tupleSize);
}

// Does it go through the device path, with freeDeviceBytes free on the device before anything is allocated for it?  Row numbers are 32
// bits, the scan-order tuples stay at or below rpack::MAX_TUPLE_BYTES, and all buffers leave rpack::DEVICE_SPARE_BYTES free.
inline bool fitsDevice(int64_t rows, int64_t outRows, int64_t tupleSize, int64_t sortTempBytes, int64_t freeDeviceBytes) {
    if (rows < 0 || outRows < 0 || outRows > rows || tupleSize <= 0 || sortTempBytes < 0 || rows >= ((int64_t)1 << 32)) return false;
    if (rows > rpack::MAX_TUPLE_BYTES / tupleSize) return false;          // (rows x tupleSize > MAX_TUPLE_BYTES, without forming the product)
    return deviceBytes(rows, outRows, tupleSize, sortTempBytes) <= freeDeviceBytes - rpack::DEVICE_SPARE_BYTES;
}

}  // namespace osort
}  // namespace rsq
