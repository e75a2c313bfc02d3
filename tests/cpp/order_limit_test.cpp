// Exercises resql_amd/csrc/order_limit.h on the host: the image of a first sort key's cell - the number the device selection orders rows
// by - against compareTyped (hostref.cpp), the comparison the reference's quicksort makes, over the values where the two could part
// (INT_MIN, -1, 0, INT_MAX, INT64_MIN, INT64_MAX, a DATE at and above 2^31), ascending and descending; and columnsToTuples, the loop
// that packs struct-of-arrays columns into ReSQL tuples for both paths of the materialisation's tail, against tuples spelled out here.
// Every buffer is a heap block of exactly the bytes that may be touched - a 4-byte cell is a 4-byte block, so a cell read as 8 bytes
// is a finding of the address sanitizer.  Host code only.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "order_limit.h"

using namespace rsq;

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { if (failures < 50) { fprintf(stderr, "order_limit_test: %s failed at line %d: ", #c, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } failures++; } } while (0)

static Type stringType(int tag, int len) { Type t(tag); t.len = len; return t; }

// the image of a value held in a heap block of exactly `width` bytes
static uint64_t imageOf(int64_t v, int width, bool desc) {
    void* cell = malloc((size_t)width);
    if (width == 4) { const int32_t x = (int32_t)v; memcpy(cell, &x, 4); } else memcpy(cell, &v, 8);
    const uint64_t u = ordlim::image(cell, width, desc);
    free(cell);
    return u;
}

static int compareOf(const Type& t, int64_t a, int64_t b, int width) {
    uint8_t* l = (uint8_t*)malloc((size_t)width); uint8_t* r = (uint8_t*)malloc((size_t)width);
    if (width == 4) { const int32_t x = (int32_t)a, y = (int32_t)b; memcpy(l, &x, 4); memcpy(r, &y, 4); } else { memcpy(l, &a, 8); memcpy(r, &b, 8); }
    const int c = compareTyped(t, l, r);
    free(l); free(r);
    return c;
}

// "a comes before b in the requested order" is "image(a) > image(b)", and equal keys have equal images
static void checkImages() {
    const std::vector<int64_t> v32 = {INT_MIN, INT_MIN + 1, -2, -1, 0, 1, 2, 19920101, 19981231, INT_MAX - 1, INT_MAX,
                                      (int64_t)(int32_t)0x80000000u, (int64_t)(int32_t)0x80000005u, (int64_t)(int32_t)0xFFFFFFFFu};      // (DATEs at and above 2^31 as the cell holds them)
    const std::vector<int64_t> v64 = {LLONG_MIN, LLONG_MIN + 1, (int64_t)INT_MIN - 1, INT_MIN, -1, 0, 1, INT_MAX, (int64_t)INT_MAX + 1, (int64_t)1 << 32,
                                      ((int64_t)1 << 32) - 1, -((int64_t)1 << 32), LLONG_MAX - 1, LLONG_MAX};
    struct Case { Type type; int width; const std::vector<int64_t>* values; };
    const Case cases[] = {{Type(RSQ_INT), 4, &v32}, {Type(RSQ_DATE), 4, &v32}, {Type(RSQ_BIGINT), 8, &v64}, {Type::decimal(15, 2), 8, &v64}};
    for (const Case& c : cases)
        for (int64_t a : *c.values)
            for (int64_t b : *c.values) {
                const int cmp = compareOf(c.type, a, b, c.width);
                for (int desc = 0; desc < 2; desc++) {
                    const uint64_t ia = imageOf(a, c.width, desc != 0), ib = imageOf(b, c.width, desc != 0);
                    const bool before = desc ? cmp > 0 : cmp < 0;
                    CHECK((ia > ib) == before, "type %d width %d desc %d: %lld against %lld", c.type.tag, c.width, desc, (long long)a, (long long)b);
                    CHECK((ia == ib) == (cmp == 0), "type %d width %d desc %d: %lld equals %lld", c.type.tag, c.width, desc, (long long)a, (long long)b);
                }
            }
    // the rule itself: key ^ 2^63, complemented for ascending order; a 4-byte cell is sign-extended
    CHECK(imageOf(0, 8, true) == 0x8000000000000000ull, "0 descending");
    CHECK(imageOf(0, 8, false) == 0x7fffffffffffffffull, "0 ascending");
    CHECK(imageOf(-1, 4, true) == 0x7fffffffffffffffull, "-1 as a 4-byte cell");
    CHECK(imageOf(INT_MIN, 4, true) == 0x7fffffff80000000ull, "INT_MIN as a 4-byte cell");
    CHECK(imageOf(LLONG_MIN, 8, true) == 0 && imageOf(LLONG_MAX, 8, true) == ~0ull, "the ends descending");
    CHECK(imageOf(LLONG_MIN, 8, false) == ~0ull && imageOf(LLONG_MAX, 8, false) == 0, "the ends ascending");
}

static std::string S(const char* bytes, size_t n) { return std::string(bytes, n); }

// INT, CHAR(5), BIGINT, CHAR(1), VARCHAR(3), BOOL, DATE, DECIMAL: fields at 0, 4, 10, 18, 20, 24, 25, 29; 37 bytes a tuple
static void checkTuples() {
    const std::vector<Type> types = {Type(RSQ_INT), stringType(RSQ_CHAR, 5), Type(RSQ_BIGINT), stringType(RSQ_CHAR, 1), stringType(RSQ_VARCHAR, 3), Type(RSQ_BOOL),
                                     Type(RSQ_DATE), Type::decimal(15, 2)};
    const size_t n = 3, ts = 37;
    const int32_t ci[n] = {INT_MIN, -1, 7};
    const std::string c5 = S("abcde", 5) + S("x\0JUN", 5) + S("\0\0\0\0\0", 5);       // a full value, a short one with bytes behind its NUL, an empty one
    const int64_t cb[n] = {LLONG_MIN, 0x0102030405060708ll, -2};
    const std::string c1 = S("R\0z", 3);
    const std::string v3 = S("xyz", 3) + S("q\0\0", 3) + S("\0ab", 3);
    const uint8_t co[n] = {1, 0, 255};
    const uint32_t cd[n] = {19920101u, 0x80000005u, 0};
    const int64_t cm[n] = {LLONG_MAX, -100, 12345};
    // every column in a heap block of exactly its bytes
    auto block = [](const void* p, size_t bytes) { uint8_t* b = (uint8_t*)malloc(bytes); memcpy(b, p, bytes); return b; };
    std::vector<uint8_t*> owned = {block(ci, sizeof ci), block(c5.data(), c5.size()), block(cb, sizeof cb), block(c1.data(), c1.size()), block(v3.data(), v3.size()),
                                   block(co, sizeof co), block(cd, sizeof cd), block(cm, sizeof cm)};
    std::vector<const uint8_t*> cols(owned.begin(), owned.end());
    auto tuple = [&](int32_t i, const std::string& s5, int64_t b, char one, const std::string& s3, uint8_t o, uint32_t d, int64_t m) {
        std::string t(ts, '\0');
        memcpy(&t[0], &i, 4); memcpy(&t[4], s5.data(), s5.size()); memcpy(&t[10], &b, 8); t[18] = one; memcpy(&t[20], s3.data(), s3.size());
        t[24] = (char)o; memcpy(&t[25], &d, 4); memcpy(&t[29], &m, 8);
        return t;
    };
    const std::string want[n] = {tuple(INT_MIN, "abcde", LLONG_MIN, 'R', "xyz", 1, 19920101u, LLONG_MAX),
                                 tuple(-1, "x", 0x0102030405060708ll, '\0', "q", 0, 0x80000005u, -100),      // (what lies behind a NUL never reaches the tuple)
                                 tuple(7, "", -2, 'z', "", 255, 0, 12345)};
    // all rows at once, and every sub-range into a block of exactly its tuples: the ranges the host threads of the tail split the rows into
    for (size_t lo = 0; lo <= n; lo++)
        for (size_t hi = lo; hi <= n; hi++) {
            uint8_t* out = (uint8_t*)calloc(hi > lo ? (hi - lo) * ts : 1, 1);
            columnsToTuples(types, cols.data(), lo, hi, out, ts);
            for (size_t r = lo; r < hi; r++)
                CHECK(S((const char*)out + (r - lo) * ts, ts) == want[r], "row %zu of rows [%zu, %zu)", r, lo, hi);
            free(out);
        }
    for (uint8_t* b : owned) free(b);
}

int main() {
    checkImages();
    checkTuples();
    if (failures) { fprintf(stderr, "order_limit_test: %d check(s) failed\n", failures); return 1; }
    printf("order_limit_test ok\n");
    return 0;
}
