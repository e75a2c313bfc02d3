// Exercises resql_amd/csrc/result_pack.h on the host: rpack::field - the bytes the device tail of a materialisation writes for one field
// of a packed tuple - against columnsToTuples (order_limit.h) over a zeroed buffer, which stays the definition through storeValue, for
// every column type; the header's side starts from a buffer of 0xEE bytes, so a byte it leaves unwritten shows.  The strings are the
// ones where the two could part: CHAR(1), a full-width string without a NUL, an empty one, a NUL followed by non-zero bytes.  Then
// rpack::fitsDevice, the decision behind RSQ_RESULT_PACK_FALLBACK_DOES_NOT_FIT, at its edges.
// Every buffer is a heap block of exactly the bytes that may be touched, so a byte read or written beside a column or a relation is a
// finding of the address sanitizer.  Host code only.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "order_limit.h"
#include "result_pack.h"

using namespace rsq;

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { if (failures < 50) { fprintf(stderr, "result_pack_test: %s failed at line %d: ", #c, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } failures++; } } while (0)

static Type stringType(int tag, int len) { Type t(tag); t.len = len; return t; }
static std::string S(const char* bytes, size_t n) { return std::string(bytes, n); }

// the header's tuples of rows [0, n): field c at the sum of the sizes in front of it, every field through rpack::field
static void packWithHeader(const std::vector<Type>& types, const uint8_t* const* cols, size_t n, uint8_t* out, size_t ts) {
    size_t off = 0;
    for (size_t c = 0; c < types.size(); c++) {
        const int w = columnWidth(types[c]), fs = sizeInTuple(types[c], true);
        for (size_t r = 0; r < n; r++)
            rpack::field(types[c].isString() ? rpack::CAT_STRING : rpack::CAT_NUMERIC, w, fs, cols[c] + r * (size_t)w, out + r * ts + off);
        off += (size_t)fs;
    }
    CHECK(off == ts, "the fields cover %zu of %zu bytes", off, ts);
}

static void checkAgainstColumnsToTuples(const std::vector<Type>& types, const std::vector<std::string>& columns, size_t n, const char* what) {
    size_t ts = 0;
    for (const Type& t : types) ts += (size_t)sizeInTuple(t, true);
    std::vector<uint8_t*> owned;
    for (size_t c = 0; c < types.size(); c++) {
        CHECK(columns[c].size() == n * (size_t)columnWidth(types[c]), "%s: column %zu holds %zu bytes", what, c, columns[c].size());
        uint8_t* b = (uint8_t*)malloc(columns[c].size() ? columns[c].size() : 1);
        memcpy(b, columns[c].data(), columns[c].size());
        owned.push_back(b);
    }
    std::vector<const uint8_t*> cols(owned.begin(), owned.end());
    uint8_t* want = (uint8_t*)calloc(n * ts ? n * ts : 1, 1);
    columnsToTuples(types, cols.data(), 0, n, want, ts);
    uint8_t* got = (uint8_t*)malloc(n * ts ? n * ts : 1);
    memset(got, 0xEE, n * ts);
    packWithHeader(types, cols.data(), n, got, ts);
    for (size_t i = 0; i < n * ts; i++)
        if (got[i] != want[i]) { CHECK(false, "%s: byte %zu of row %zu is %02x, columnsToTuples wrote %02x", what, i % ts, i / ts, got[i], want[i]); break; }
    free(want); free(got);
    for (uint8_t* b : owned) free(b);
}

template <typename V> static std::string bytesOf(const std::vector<V>& v) { return std::string((const char*)v.data(), v.size() * sizeof(V)); }

static void checkFields() {
    // every type in one tuple: INT, CHAR(5), BIGINT, CHAR(1), VARCHAR(3), BOOL, DATE, DECIMAL - 37 bytes
    {
        const std::vector<Type> types = {Type(RSQ_INT), stringType(RSQ_CHAR, 5), Type(RSQ_BIGINT), stringType(RSQ_CHAR, 1), stringType(RSQ_VARCHAR, 3), Type(RSQ_BOOL),
                                         Type(RSQ_DATE), Type::decimal(15, 2)};
        const std::vector<std::string> columns = {
            bytesOf(std::vector<int32_t>{INT_MIN, -1, 7, INT_MAX}),
            S("abcde", 5) + S("x\0JUN", 5) + S("\0\0\0\0\0", 5) + S("\0bcde", 5),          // full width, bytes behind a NUL, empty, a NUL in front of non-zero bytes
            bytesOf(std::vector<int64_t>{LLONG_MIN, 0x0102030405060708ll, -2, LLONG_MAX}),
            S("R\0z\xff", 4),
            S("xyz", 3) + S("q\0\0", 3) + S("\0ab", 3) + S("ab\0", 3),
            bytesOf(std::vector<uint8_t>{1, 0, 255, 2}),
            bytesOf(std::vector<uint32_t>{19920101u, 0x80000005u, 0, 0xffffffffu}),
            bytesOf(std::vector<int64_t>{LLONG_MAX, -100, 12345, LLONG_MIN})};
        checkAgainstColumnsToTuples(types, columns, 4, "all types");
    }
    // each type alone, so that a field's first and last byte are the relation's
    {
        checkAgainstColumnsToTuples({Type(RSQ_BOOL)}, {bytesOf(std::vector<uint8_t>{0, 1, 0xEE})}, 3, "BOOL");
        checkAgainstColumnsToTuples({Type(RSQ_INT)}, {bytesOf(std::vector<int32_t>{INT_MIN, 0, (int32_t)0xEEEEEEEE})}, 3, "INT");
        checkAgainstColumnsToTuples({Type(RSQ_DATE)}, {bytesOf(std::vector<uint32_t>{0, 19981231u, 0x80000000u})}, 3, "DATE");
        checkAgainstColumnsToTuples({Type(RSQ_BIGINT)}, {bytesOf(std::vector<int64_t>{LLONG_MIN, -1, LLONG_MAX})}, 3, "BIGINT");
        checkAgainstColumnsToTuples({Type::decimal(18, 4)}, {bytesOf(std::vector<int64_t>{LLONG_MIN, 1, LLONG_MAX})}, 3, "DECIMAL");
        checkAgainstColumnsToTuples({stringType(RSQ_CHAR, 1)}, {S("A\0\xee", 3)}, 3, "CHAR(1)");
        checkAgainstColumnsToTuples({stringType(RSQ_VARCHAR, 1)}, {S("A\0\xee", 3)}, 3, "VARCHAR(1)");
        checkAgainstColumnsToTuples({stringType(RSQ_CHAR, 4)}, {S("full", 4) + S("\0\0\0\0", 4) + S("a\0zz", 4) + S("\0zzz", 4) + S("ab  ", 4)}, 5, "CHAR(4)");
        checkAgainstColumnsToTuples({stringType(RSQ_VARCHAR, 7)}, {S("fullwid", 7) + S("\0\0\0\0\0\0\0", 7) + S("abc\0xyz", 7) + S("\0\xee\xee\xee\xee\xee\xee", 7)}, 4, "VARCHAR(7)");
        checkAgainstColumnsToTuples({Type(RSQ_INT)}, {std::string()}, 0, "no rows");
    }
    // a long string: a NUL at every position of a VARCHAR(300), non-zero bytes behind it
    {
        const size_t len = 300, n = len + 1;
        std::string col(n * len, 'k');
        for (size_t r = 0; r < len; r++) col[r * len + r] = '\0';          // (the last row keeps its full width)
        checkAgainstColumnsToTuples({stringType(RSQ_VARCHAR, (int)len), Type(RSQ_BIGINT)}, {col, std::string(n * 8, '\x5a')}, n, "VARCHAR(300)");
    }
}

static void checkFit() {
    const int64_t GiB = (int64_t)1 << 30, cap = rpack::MAX_TUPLE_BYTES, spare = rpack::DEVICE_SPARE_BYTES, plenty = (int64_t)256 << 30;
    CHECK(cap == 2 * GiB && spare == GiB, "the cap is %lld, the spare %lld", (long long)cap, (long long)spare);
    // row numbers are 32 bits
    CHECK(rpack::fitsDevice(((int64_t)1 << 31) , 1, plenty), "2^31 one-byte tuples");
    CHECK(!rpack::fitsDevice(((int64_t)1 << 32), 1, INT64_MAX), "2^32 rows");
    CHECK(!rpack::fitsDevice(((int64_t)1 << 32) - 1, 1, INT64_MAX), "2^32 - 1 one-byte tuples are above the cap");
    // rows x tuple size against the cap, to the byte
    CHECK(rpack::fitsDevice(cap / 4, 4, plenty), "exactly the cap");
    CHECK(!rpack::fitsDevice(cap / 4 + 1, 4, plenty), "four bytes above the cap");
    CHECK(rpack::fitsDevice(cap / 34, 34, plenty) && !rpack::fitsDevice(cap / 34 + 1, 34, plenty), "a tuple size that does not divide the cap");
    CHECK(rpack::fitsDevice(1, cap, plenty) && !rpack::fitsDevice(1, cap + 1, plenty) && !rpack::fitsDevice(2, cap, plenty), "one tuple of the cap's size");
    CHECK(!rpack::fitsDevice(((int64_t)1 << 32) - 1, INT64_MAX, INT64_MAX), "a product that does not fit 64 bits");
    // what is free, with 1 GiB to spare, to the byte
    CHECK(rpack::fitsDevice(1000, 100, spare + 100000), "exactly what is free");
    CHECK(!rpack::fitsDevice(1000, 100, spare + 99999), "one byte more than is free");
    CHECK(!rpack::fitsDevice(1, 1, spare) && rpack::fitsDevice(1, 1, spare + 1), "one byte");
    CHECK(!rpack::fitsDevice(1, 1, 0) && !rpack::fitsDevice(1, 1, -1), "nothing free");
    CHECK(rpack::fitsDevice(cap / 4, 4, cap + spare) && !rpack::fitsDevice(cap / 4, 4, cap + spare - 1), "the cap with exactly the spare behind it");
    CHECK(rpack::fitsDevice(1000, 100, INT64_MAX), "what the query holds already is not asked for again");
    // no rows fit (the driver reports SMALL before it asks); nonsense does not
    CHECK(rpack::fitsDevice(0, 4, spare), "no rows");
    CHECK(!rpack::fitsDevice(-1, 4, plenty) && !rpack::fitsDevice(1, 0, plenty) && !rpack::fitsDevice(1, -4, plenty), "negative rows, an empty tuple");
}

int main() {
    checkFields();
    checkFit();
    if (failures) { fprintf(stderr, "result_pack_test: %d check(s) failed\n", failures); return 1; }
    printf("result_pack_test ok\n");
    return 0;
}
