// Exercises resql_amd/csrc/order_sort.h on the host: the image of a sort key's cell - "earlier in the requested order" is "smaller" -
// against compareTyped (hostref.cpp) at the types' ends, both widths and directions; the layout of the composite key at its edges
// (no bits, exactly 64, 65, three full-range BIGINTs, a key that straddles a word boundary); the composite words of rows against a
// comparison by compareTyped over the same cells; and fitsDevice, the decision behind RSQ_ORDER_SORT_FALLBACK_DOES_NOT_FIT, at its limits.
// Every cell is a heap block of exactly its width - a 4-byte cell read as 8 bytes is a finding of the address sanitizer.  Host code only.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "order_sort.h"

using namespace rsq;

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { if (failures < 50) { fprintf(stderr, "order_sort_test: %s failed at line %d: ", #c, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } failures++; } } while (0)

struct Cell {          // a value in a heap block of exactly `width` bytes
    void* p; int width;
    Cell(int64_t v, int w) : p(malloc((size_t)w)), width(w) { if (w == 4) { const int32_t x = (int32_t)v; memcpy(p, &x, 4); } else memcpy(p, &v, 8); }
    Cell(const Cell& o) : p(malloc((size_t)o.width)), width(o.width) { memcpy(p, o.p, (size_t)width); }
    Cell& operator=(const Cell&) = delete;
    ~Cell() { free(p); }
};

static uint64_t imageOf(int64_t v, int width, bool desc) { Cell c(v, width); return osort::image(c.p, width, desc); }

static const std::vector<int64_t> V32 = {INT_MIN, INT_MIN + 1, -2, -1, 0, 1, 2, 19920101, 19981231, INT_MAX - 1, INT_MAX,
                                         (int64_t)(int32_t)0x80000000u, (int64_t)(int32_t)0x80000005u, (int64_t)(int32_t)0xFFFFFFFFu};      // (DATEs at and above 2^31 as the cell holds them)
static const std::vector<int64_t> V64 = {LLONG_MIN, LLONG_MIN + 1, (int64_t)INT_MIN - 1, INT_MIN, -1, 0, 1, INT_MAX, (int64_t)INT_MAX + 1, (int64_t)1 << 32,
                                         ((int64_t)1 << 32) - 1, -((int64_t)1 << 32), LLONG_MAX - 1, LLONG_MAX};

// "a comes before b in the requested order" is "image(a) < image(b)", and equal keys have equal images
static void checkImages() {
    struct Case { Type type; int width; const std::vector<int64_t>* values; };
    const Case cases[] = {{Type(RSQ_INT), 4, &V32}, {Type(RSQ_DATE), 4, &V32}, {Type(RSQ_BIGINT), 8, &V64}, {Type::decimal(15, 2), 8, &V64}};
    for (const Case& c : cases)
        for (int64_t a : *c.values)
            for (int64_t b : *c.values) {
                Cell l(a, c.width), r(b, c.width);
                const int cmp = compareTyped(c.type, (const uint8_t*)l.p, (const uint8_t*)r.p);
                for (int desc = 0; desc < 2; desc++) {
                    const uint64_t ia = osort::image(l.p, c.width, desc != 0), ib = osort::image(r.p, c.width, desc != 0);
                    const bool before = desc ? cmp > 0 : cmp < 0;
                    CHECK((ia < ib) == before, "type %d width %d desc %d: %lld against %lld", c.type.tag, c.width, desc, (long long)a, (long long)b);
                    CHECK((ia == ib) == (cmp == 0), "type %d width %d desc %d: %lld equals %lld", c.type.tag, c.width, desc, (long long)a, (long long)b);
                }
            }
    // the rule itself: key ^ 2^63, complemented for descending order; a 4-byte cell is sign-extended
    CHECK(imageOf(0, 8, false) == 0x8000000000000000ull, "0 ascending");
    CHECK(imageOf(0, 8, true) == 0x7fffffffffffffffull, "0 descending");
    CHECK(imageOf(-1, 4, false) == 0x7fffffffffffffffull, "-1 as a 4-byte cell");
    CHECK(imageOf(INT_MIN, 4, false) == 0x7fffffff80000000ull && imageOf(INT_MAX, 4, false) == 0x800000007fffffffull, "the ends of a 4-byte cell");
    CHECK(imageOf(LLONG_MIN, 8, false) == 0 && imageOf(LLONG_MAX, 8, false) == ~0ull, "the ends ascending");
    CHECK(imageOf(LLONG_MIN, 8, true) == ~0ull && imageOf(LLONG_MAX, 8, true) == 0, "the ends descending");
    for (int desc = 0; desc < 2; desc++)
        CHECK(imageOf(-7, 4, desc != 0) == ~ordlim::image(Cell(-7, 4).p, 4, desc != 0), "the complement of order_limit.h's image");
}

static void checkLayouts() {
    {   // no key varies: no bits, no word
        const uint64_t mn[3] = {5, ~0ull, 0}, mx[3] = {5, ~0ull, 0};
        const osort::Layout L = osort::layoutOf(mn, mx, 3);
        CHECK(L.totalBits == 0 && L.nWords == 0 && osort::passesOf(L) == 0 && L.bits[0] == 0 && L.bits[1] == 0 && L.bits[2] == 0, "constant keys take %d bits", L.totalBits);
    }
    {   // bits = 64 - clz(max - min): 1 for a span of 1, 8 for 255, 9 for 256, 64 for the whole range
        const uint64_t mn[4] = {10, 0, 1000, 0}, mx[4] = {11, 255, 1256, ~0ull};
        const osort::Layout L = osort::layoutOf(mn, mx, 4);
        CHECK(L.bits[0] == 1 && L.bits[1] == 8 && L.bits[2] == 9 && L.bits[3] == 64, "bits %d %d %d %d", L.bits[0], L.bits[1], L.bits[2], L.bits[3]);
        CHECK(L.totalBits == 82 && L.nWords == 2, "82 bits in %d words", L.nWords);
        // the last key is the least significant: all of word 0; the others lie in word 1, key 2 lowest
        CHECK(L.word[0].bits == 64 && L.word[0].nPieces == 1 && L.word[0].piece[0].key == 3 && L.word[0].piece[0].bits == 64, "word 0");
        CHECK(L.word[1].bits == 18 && L.word[1].nPieces == 3 && L.word[1].piece[0].key == 2 && L.word[1].piece[0].dstShift == 0 && L.word[1].piece[1].key == 1 &&
              L.word[1].piece[1].dstShift == 9 && L.word[1].piece[2].key == 0 && L.word[1].piece[2].dstShift == 17, "word 1");
        CHECK(osort::passesOf(L) == 8 + 3, "%d passes", osort::passesOf(L));
    }
    {   // exactly 64 bits: one full word; one bit more: two words, the first key's top bit alone in the second
        const uint64_t mn[2] = {0, 0}, mx64[2] = {(1ull << 32) - 1, (1ull << 32) - 1}, mx65[2] = {(1ull << 33) - 1, (1ull << 32) - 1};
        const osort::Layout A = osort::layoutOf(mn, mx64, 2), B = osort::layoutOf(mn, mx65, 2);
        CHECK(A.totalBits == 64 && A.nWords == 1 && A.word[0].bits == 64 && A.word[0].nPieces == 2 && osort::passesOf(A) == 8, "64 bits");
        CHECK(B.totalBits == 65 && B.nWords == 2 && B.word[0].bits == 64 && B.word[1].bits == 1 && osort::passesOf(B) == 9, "65 bits");
        // the first key straddles the boundary: 32 bits in word 0 from bit 32, its 33rd bit in word 1
        CHECK(B.word[0].nPieces == 2 && B.word[0].piece[1].key == 0 && B.word[0].piece[1].srcShift == 0 && B.word[0].piece[1].dstShift == 32 && B.word[0].piece[1].bits == 32, "the straddling key's low piece");
        CHECK(B.word[1].nPieces == 1 && B.word[1].piece[0].key == 0 && B.word[1].piece[0].srcShift == 32 && B.word[1].piece[0].dstShift == 0 && B.word[1].piece[0].bits == 1, "... and its high piece");
    }
    {   // three full-range BIGINTs: three words, one key each, the last key first; eight: eight words
        const uint64_t mn[8] = {0, 0, 0, 0, 0, 0, 0, 0}, mx[8] = {~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull};
        const osort::Layout L = osort::layoutOf(mn, mx, 3), M = osort::layoutOf(mn, mx, 8);
        CHECK(L.totalBits == 192 && L.nWords == 3 && osort::passesOf(L) == 24, "192 bits");
        for (int w = 0; w < 3; w++) CHECK(L.word[w].bits == 64 && L.word[w].nPieces == 1 && L.word[w].piece[0].key == 2 - w, "word %d", w);
        CHECK(M.totalBits == 512 && M.nWords == (int)osort::MAX_WORDS && osort::passesOf(M) == 64, "512 bits");
    }
}

// rows of several keys: the order of their composite words, most significant word first, is the order compareTyped gives over the cells
struct KeySpec { Type type; int width; bool desc; const std::vector<int64_t>* values; };

static void checkWords(const std::vector<KeySpec>& keys, size_t nRows, const char* what) {
    const int K = (int)keys.size();
    std::vector<std::vector<Cell>> cells((size_t)K);
    for (int k = 0; k < K; k++)
        for (size_t r = 0; r < nRows; r++) {
            const std::vector<int64_t>& v = *keys[(size_t)k].values;
            cells[(size_t)k].emplace_back(v[(r * (size_t)(2 * k + 3) + (size_t)k + r / 5) % v.size()], keys[(size_t)k].width);
        }
    std::vector<uint64_t> images(nRows * (size_t)K);
    uint64_t mn[osort::MAX_KEYS], mx[osort::MAX_KEYS];
    for (int k = 0; k < K; k++) {
        mn[k] = ~0ull; mx[k] = 0;
        for (size_t r = 0; r < nRows; r++) {
            const uint64_t im = osort::image(cells[(size_t)k][r].p, keys[(size_t)k].width, keys[(size_t)k].desc);
            images[r * (size_t)K + (size_t)k] = im;
            mn[k] = im < mn[k] ? im : mn[k]; mx[k] = im > mx[k] ? im : mx[k];
        }
    }
    const osort::Layout L = osort::layoutOf(mn, mx, K);
    int sum = 0;
    for (int k = 0; k < K; k++) sum += L.bits[k];
    CHECK(sum == L.totalBits && L.nWords == (sum + 63) / 64, "%s: %d bits in %d words", what, L.totalBits, L.nWords);
    for (int w = 0; w < L.nWords; w++) CHECK(L.word[w].bits == (w + 1 < L.nWords ? 64 : sum - 64 * w), "%s: word %d holds %d bits", what, w, L.word[w].bits);
    for (size_t a = 0; a < nRows; a++)
        for (size_t b = 0; b < nRows; b++) {
            int byCells = 0;          // -1: a first, 1: b first, 0: equal on every key
            for (int k = 0; k < K && !byCells; k++) {
                const int c = compareTyped(keys[(size_t)k].type, (const uint8_t*)cells[(size_t)k][a].p, (const uint8_t*)cells[(size_t)k][b].p);
                if (c) byCells = (c < 0) != keys[(size_t)k].desc ? -1 : 1;
            }
            int byWords = 0;
            for (int w = L.nWords - 1; w >= 0 && !byWords; w--) {
                const uint64_t x = osort::wordOf(L.word[w], L.min, &images[a * (size_t)K]), y = osort::wordOf(L.word[w], L.min, &images[b * (size_t)K]);
                CHECK(L.word[w].bits == 64 || (x >> L.word[w].bits) == 0, "%s: word %d has bits above its %d", what, w, L.word[w].bits);
                if (x != y) byWords = x < y ? -1 : 1;
            }
            CHECK(byCells == byWords, "%s: rows %zu and %zu compare %d by their cells, %d by their words", what, a, b, byCells, byWords);
        }
}

static void checkFit() {
    const int64_t GiB = (int64_t)1 << 30, cap = rpack::MAX_TUPLE_BYTES, spare = rpack::DEVICE_SPARE_BYTES, plenty = (int64_t)256 << 30;
    CHECK(cap == 2 * GiB && spare == GiB, "the cap is %lld, the spare %lld", (long long)cap, (long long)spare);
    // the buffers: two key arrays, two permutations, the temporary, both tuple buffers, each rounded up to 256 bytes
    CHECK(osort::deviceBytes(1000, 1000, 100, 5000) == 2 * 8192 + 2 * 4096 + 5120 + 2 * 100096, "deviceBytes is %lld", (long long)osort::deviceBytes(1000, 1000, 100, 5000));
    CHECK(osort::deviceBytes(1000, 10, 100, 5000) == 2 * 8192 + 2 * 4096 + 5120 + 100096 + 1024, "with a LIMIT");
    const int64_t need = osort::deviceBytes(1000, 1000, 100, 5000);
    CHECK(osort::fitsDevice(1000, 1000, 100, 5000, spare + need), "exactly what is free");
    CHECK(!osort::fitsDevice(1000, 1000, 100, 5000, spare + need - 1), "one byte more than is free");
    CHECK(osort::fitsDevice(1000, 1000, 100, 5000, INT64_MAX), "what the query holds already is not asked for again");
    CHECK(!osort::fitsDevice(1, 1, 1, 0, spare) && !osort::fitsDevice(1, 1, 1, 0, 0) && !osort::fitsDevice(1, 1, 1, 0, -1), "nothing free");
    // row numbers are 32 bits
    CHECK(!osort::fitsDevice((int64_t)1 << 32, 0, 1, 0, INT64_MAX) && !osort::fitsDevice(((int64_t)1 << 32) - 1, 0, 1, 0, INT64_MAX), "2^32 rows; 2^32 - 1 one-byte tuples are above the cap");
    CHECK(osort::fitsDevice((int64_t)1 << 31, 0, 1, 0, plenty), "2^31 one-byte tuples");
    // rows x tuple size against the cap, to the byte
    CHECK(osort::fitsDevice(cap / 4, 0, 4, 0, plenty) && !osort::fitsDevice(cap / 4 + 1, 0, 4, 0, plenty), "the cap");
    CHECK(osort::fitsDevice(cap / 34, 5, 34, 0, plenty) && !osort::fitsDevice(cap / 34 + 1, 5, 34, 0, plenty), "a tuple size that does not divide the cap");
    CHECK(!osort::fitsDevice(((int64_t)1 << 32) - 1, 1, INT64_MAX, 0, INT64_MAX), "a product that does not fit 64 bits");
    // nonsense does not fit
    CHECK(!osort::fitsDevice(-1, 0, 4, 0, plenty) && !osort::fitsDevice(10, 11, 4, 0, plenty) && !osort::fitsDevice(10, -1, 4, 0, plenty) && !osort::fitsDevice(10, 10, 0, 0, plenty) &&
          !osort::fitsDevice(10, 10, 4, -1, plenty), "negative rows, more output rows than rows, an empty tuple, a negative temporary");
    CHECK(osort::fitsDevice(0, 0, 4, 0, plenty), "no rows (the driver reports SMALL before it asks)");
}

int main() {
    checkImages();
    checkLayouts();
    const std::vector<int64_t> small = {3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13}, one = {42};
    checkWords({{Type(RSQ_INT), 4, false, &V32}, {Type(RSQ_BIGINT), 8, true, &V64}}, 60, "INT asc, BIGINT desc over their ends (two words)");
    checkWords({{Type(RSQ_BIGINT), 8, false, &V64}, {Type(RSQ_BIGINT), 8, true, &V64}, {Type::decimal(15, 2), 8, false, &V64}}, 70, "three full-range keys (three words)");
    checkWords({{Type(RSQ_DATE), 4, true, &V32}, {Type(RSQ_INT), 4, false, &one}, {Type(RSQ_INT), 4, false, &small}}, 60, "a constant key between two varying ones");
    checkWords({{Type(RSQ_INT), 4, false, &one}, {Type(RSQ_BIGINT), 8, true, &one}}, 9, "all keys constant");
    checkWords({{Type(RSQ_BIGINT), 8, false, &V64}, {Type(RSQ_INT), 4, false, &small}, {Type(RSQ_INT), 4, true, &small}, {Type(RSQ_DATE), 4, false, &small},
                {Type(RSQ_BIGINT), 8, true, &small}, {Type(RSQ_INT), 4, false, &small}, {Type::decimal(15, 2), 8, false, &small}, {Type(RSQ_INT), 4, true, &small}}, 80,
               "8 keys, the first straddling a word boundary");
    checkFit();
    if (failures) { fprintf(stderr, "order_sort_test: %d check(s) failed\n", failures); return 1; }
    printf("order_sort_test ok\n");
    return 0;
}
