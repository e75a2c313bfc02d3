// Exercises resql_amd/csrc/result_text.h (the text of a result cell as the device writes it) against the host's definition:
// serializeSqlValue (expr.cpp) of loadValue (hostref.cpp) for single cells, serializeResultView for whole rows.  For every type
// category a fixed edge list and 20 000 seeded values: cellTextLength is the host text's length, writeCellText writes the host's bytes
// and returns that length, maxCellTextLength bounds it.  Every buffer the header reads or writes is a heap block of exactly the bytes
// it may touch - a string cell is handed over WITHOUT its byte n - so the address sanitizer sees any step beyond them.  Host code only.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hostref.h"
#include "result_text.h"

using namespace rsq;

static int failures = 0;
static long checked = 0;
#define CHECK(c, ...) do { if (!(c)) { if (failures < 50) { fprintf(stderr, "result_text_test: %s failed at line %d: ", #c, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } failures++; } } while (0)

static uint64_t rngState = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() { rngState ^= rngState << 13; rngState ^= rngState >> 7; rngState ^= rngState << 17; return rngState; }

static Type charType(int tag, int len) { Type t(tag); t.len = len; return t; }
static int categoryOf(const Type& t) {
    switch (t.tag) {
        case RSQ_INT: return rtxt::CAT_INT;
        case RSQ_BIGINT: return rtxt::CAT_BIGINT;
        case RSQ_DECIMAL: return rtxt::CAT_DECIMAL;
        case RSQ_DATE: return rtxt::CAT_DATE;
        case RSQ_BOOL: return rtxt::CAT_BOOL;
        case RSQ_CHAR: return rtxt::CAT_CHAR;
        default: return rtxt::CAT_VARCHAR;
    }
}
static int lenOrScaleOf(const Type& t) { return t.tag == RSQ_DECIMAL ? t.scale : (t.tag == RSQ_CHAR || t.tag == RSQ_VARCHAR) ? t.len : 0; }
// the bytes of a cell the header may read: the value's width, a string's n bytes (its field has n + 1)
static size_t readableBytes(const Type& t) { return (t.tag == RSQ_CHAR && t.len > 1) || t.tag == RSQ_VARCHAR ? (size_t)t.len : t.tag == RSQ_CHAR ? 1 : (size_t)sizeInTuple(t, true); }

static std::string shown(const std::string& f) {
    std::string s;
    char b[8];
    for (unsigned char c : f) { if (c >= 32 && c < 127) s += (char)c; else { snprintf(b, sizeof b, "\\x%02x", c); s += b; } }
    return s;
}

// `field`: the cell as a tuple holds it, sizeInTuple bytes
static void checkCell(const Type& t, const std::vector<uint8_t>& field) {
    const std::string want = serializeSqlValue(loadValue(field.data(), t), t);
    const int cat = categoryOf(t), ls = lenOrScaleOf(t);
    const size_t nRead = readableBytes(t);
    unsigned char* cell = (unsigned char*)malloc(nRead ? nRead : 1);
    memcpy(cell, field.data(), nRead);
    const int len = rtxt::cellTextLength(cat, ls, cell);
    CHECK(len == (int)want.size(), "type %d(%d,%d): length %d, the host's text '%s' has %zu", t.tag, t.len, t.scale, len, shown(want).c_str(), want.size());
    CHECK(len <= rtxt::maxCellTextLength(cat, ls), "type %d(%d,%d): length %d above the bound %d", t.tag, t.len, t.scale, len, rtxt::maxCellTextLength(cat, ls));
    if (len == (int)want.size()) {
        unsigned char* out = (unsigned char*)malloc(len ? (size_t)len : 1);
        const int wrote = rtxt::writeCellText(cat, ls, cell, out);
        CHECK(wrote == len, "type %d(%d,%d): wrote %d of %d bytes", t.tag, t.len, t.scale, wrote, len);
        CHECK(memcmp(out, want.data(), (size_t)len) == 0, "type %d(%d,%d): '%s', the host writes '%s'", t.tag, t.len, t.scale,
              shown(std::string((const char*)out, (size_t)len)).c_str(), shown(want).c_str());
        free(out);
    }
    free(cell);
    checked++;
}

static void checkNumber(const Type& t, int64_t v) {
    std::vector<uint8_t> field((size_t)sizeInTuple(t, true));
    if (t.tag == RSQ_INT || t.tag == RSQ_DATE) { int32_t x = (int32_t)v; memcpy(field.data(), &x, 4); }
    else if (t.tag == RSQ_BOOL) field[0] = (uint8_t)v;
    else memcpy(field.data(), &v, 8);
    checkCell(t, field);
}
// `bytes` go into the field as they are (at most n + 1 of them); the rest is NUL
static void checkString(const Type& t, const std::string& bytes) {
    std::vector<uint8_t> field((size_t)sizeInTuple(t, true), 0);
    memcpy(field.data(), bytes.data(), std::min(bytes.size(), field.size()));
    if (t.len > 1 || t.tag == RSQ_VARCHAR) field[(size_t)t.len] = 0;          // (a well-formed field: NUL at byte n at the latest)
    checkCell(t, field);
}

// 0, +-1, the ends of both integer widths, every power of ten with its neighbours, both signs
static std::vector<int64_t> edgeNumbers() {
    std::vector<int64_t> v = {0, 1, -1, INT_MIN, INT_MAX, (int64_t)INT_MIN - 1, (int64_t)INT_MAX + 1, INT64_MIN, INT64_MAX, INT64_MIN + 1, 19920101, 99991231, 0xFFFFFFFFll, -19920101};
    int64_t p = 1;
    for (int k = 0; k <= 18; k++) {
        for (int64_t d = -1; d <= 1; d++) { v.push_back(p + d); v.push_back(-(p + d)); }
        if (k < 18) p *= 10;
    }
    return v;
}

static int64_t seededNumber() {
    const uint64_t bits = rnd() >> (rnd() % 64);          // every digit count is met
    return (rnd() & 1) ? (int64_t)bits : (int64_t)(0 - bits);
}
static std::string seededString(int n) {
    const size_t len = (size_t)(rnd() % (uint64_t)(n + 2));          // 0 .. n + 1 bytes in front of the first NUL (n + 1: the field is full)
    std::string s;
    for (size_t i = 0; i < len; i++) s += (char)(rnd() % 4 == 0 ? ' ' : 1 + rnd() % 255);
    s += '\0';
    while ((int)s.size() < n + 1) s += (char)(rnd() % 256);           // whatever lies behind the NUL is never printed
    return s;
}

int main() {
    const std::vector<int64_t> edges = edgeNumbers();
    std::vector<Type> numeric = {Type(RSQ_INT), Type(RSQ_BIGINT), Type(RSQ_DATE), Type(RSQ_BOOL)};
    for (int s : {0, 1, 2, 6, 18}) numeric.push_back(Type::decimal(18, s));
    for (const Type& t : numeric) {
        for (int64_t v : edges) checkNumber(t, v);
        if (t.tag == RSQ_DECIMAL) {          // |raw| < 10^scale: zeros in front
            int64_t p = 1;
            for (int k = 0; k < t.scale; k++) { checkNumber(t, p); checkNumber(t, -p); checkNumber(t, p * 9); checkNumber(t, -(p * 9)); p *= 10; }
        }
        for (int i = 0; i < 20000; i++) checkNumber(t, seededNumber());
    }
    const Type c1 = charType(RSQ_CHAR, 1), c10 = charType(RSQ_CHAR, 10), c2 = charType(RSQ_CHAR, 2), v25 = charType(RSQ_VARCHAR, 25), v1 = charType(RSQ_VARCHAR, 1);
    for (int b = 0; b < 256; b++) checkString(c1, std::string(1, (char)b));          // (NUL prints one blank)
    for (const Type& t : {c2, c10, v25, v1}) {
        checkString(t, "");
        checkString(t, std::string((size_t)t.len, 'x'));                       // full: no NUL inside n bytes
        checkString(t, std::string((size_t)t.len, ' '));
        checkString(t, std::string("a") + std::string((size_t)t.len - 1, ' '));          // trailing blanks
        checkString(t, std::string("a\0bcdefghi", 10));                          // bytes behind a NUL
        checkString(t, std::string((size_t)t.len - 1, 'y'));
        checkString(t, std::string((size_t)t.len, '\xff'));
    }
    for (const Type& t : {c1, c2, c10, v25, v1, charType(RSQ_CHAR, 200), charType(RSQ_VARCHAR, 100)})
        for (int i = 0; i < 20000; i++) checkString(t, seededString(t.len));

    // whole rows against serializeResultView: a tuple buffer of exactly n_rows * tuple_size bytes, the text of exactly the summed lengths
    const std::vector<Type> row = {Type(RSQ_INT), Type(RSQ_BIGINT), Type::decimal(15, 2), Type::decimal(18, 0), Type::decimal(12, 6), Type(RSQ_DATE), Type(RSQ_BOOL), c1, c10, v25};
    std::vector<rsq_type> types;
    std::vector<int32_t> offsets;
    int tupleSize = 0;
    for (const Type& t : row) { types.push_back(t.toC()); offsets.push_back(tupleSize); tupleSize += sizeInTuple(t, true); }
    for (int64_t nRows : {0, 1, 257, 2000}) {
        uint8_t* tuples = (uint8_t*)malloc((size_t)nRows * (size_t)tupleSize + (nRows ? 0 : 1));
        for (int64_t r = 0; r < nRows; r++)
            for (size_t c = 0; c < row.size(); c++) {
                uint8_t* cell = tuples + r * tupleSize + offsets[c];
                const Type& t = row[c];
                if (t.tag == RSQ_CHAR || t.tag == RSQ_VARCHAR) {
                    const std::string s = seededString(t.len);
                    memcpy(cell, s.data(), (size_t)sizeInTuple(t, true));
                    if (t.len > 1 || t.tag == RSQ_VARCHAR) cell[t.len] = 0;
                } else {
                    const int64_t v = r % 7 == 0 ? edges[(size_t)(rnd() % edges.size())] : seededNumber();
                    memcpy(cell, &v, (size_t)sizeInTuple(t, true));          // (little-endian: the low bytes)
                }
            }
        rsq_result_view view{};
        view.n_cols = (int32_t)row.size(); view.types = types.data(); view.offsets = offsets.data(); view.tuple_size = tupleSize; view.n_rows = nRows; view.tuples = tuples;
        const std::string want = serializeResultView(view);
        size_t total = 0;
        for (int64_t r = 0; r < nRows; r++) {
            for (size_t c = 0; c < row.size(); c++) total += (size_t)rtxt::cellTextLength(categoryOf(row[c]), lenOrScaleOf(row[c]), tuples + r * tupleSize + offsets[c]);
            total += row.size() + 1;
        }
        CHECK(total == want.size(), "%lld rows: %zu bytes of text, the host writes %zu", (long long)nRows, total, want.size());
        if (total == want.size()) {
            unsigned char* text = (unsigned char*)malloc(total ? total : 1);
            unsigned char* p = text;
            for (int64_t r = 0; r < nRows; r++) {
                for (size_t c = 0; c < row.size(); c++) {
                    p += rtxt::writeCellText(categoryOf(row[c]), lenOrScaleOf(row[c]), tuples + r * tupleSize + offsets[c], p);
                    *p++ = '|';
                }
                *p++ = '\n';
            }
            CHECK((size_t)(p - text) == total && memcmp(text, want.data(), total) == 0, "%lld rows: the text differs from serializeResultView's", (long long)nRows);
            free(text);
        }
        free(tuples);
        checked++;
    }
    if (failures) { fprintf(stderr, "result_text_test: %d failure(s)\n", failures); return 1; }
    printf("result_text_test ok (%ld cells and relations)\n", checked);
    return 0;
}
