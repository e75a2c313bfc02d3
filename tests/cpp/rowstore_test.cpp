// Exercises resql_amd/csrc/rowstore.h (the cell of a packed tuple's field, as both bridges write it) and transposeRowstoreHost
// (rowstore.cpp) on tuples of the EDGE shape - BOOL, CHAR(1), INT, CHAR(7), BIGINT, DATE, VARCHAR(25), DECIMAL(15,2): 61 bytes, the BIGINT
// at offset 15 and the DECIMAL at 53 - against cells spelled out here.  Every buffer handed over is a heap block of exactly the bytes
// that may be touched - a string field WITHOUT its byte len, a block of exactly its content size - so the address sanitizer sees any step
// beyond them.  Host code only.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rowstore.h"

using namespace rsq;

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { if (failures < 50) { fprintf(stderr, "rowstore_test: %s failed at line %d: ", #c, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } failures++; } } while (0)

static Type stringType(int tag, int len) { Type t(tag); t.len = len; return t; }
static std::vector<Type> edgeTypes() {
    return {Type(RSQ_BOOL), stringType(RSQ_CHAR, 1), Type(RSQ_INT), stringType(RSQ_CHAR, 7), Type(RSQ_BIGINT), Type(RSQ_DATE), stringType(RSQ_VARCHAR, 25),
            Type::decimal(15, 2)};
}

// the cell of `field` (exactly the bytes the rule may read) into a block of exactly `width` bytes
static std::string cellOf(int category, int width, const std::string& field) {
    std::vector<uint8_t>* in = new std::vector<uint8_t>(field.begin(), field.end());
    uint8_t* out = (uint8_t*)malloc((size_t)width ? (size_t)width : 1);
    memset(out, 0xEE, (size_t)width);
    rowst::cell(category, width, in->data(), out);
    std::string got((const char*)out, (size_t)width);
    free(out);
    delete in;
    return got;
}
static std::string S(const char* bytes, size_t n) { return std::string(bytes, n); }

static void checkCells() {
    // strings: up to the first NUL within len, zeros behind it - the field's bytes behind a NUL never arrive
    CHECK(cellOf(rowst::CAT_STRING, 7, S("ab\0XY\0Z", 7)) == S("ab\0\0\0\0\0", 7), "junk behind a NUL");
    CHECK(cellOf(rowst::CAT_STRING, 7, S("ABCDEFG", 7)) == S("ABCDEFG", 7), "a string of exactly len bytes");
    CHECK(cellOf(rowst::CAT_STRING, 7, S("\0JUNKJU", 7)) == S("\0\0\0\0\0\0\0", 7), "an empty string");
    CHECK(cellOf(rowst::CAT_STRING, 7, S("abcdef\0", 7)) == S("abcdef\0", 7), "a NUL in the last byte");
    CHECK(cellOf(rowst::CAT_STRING, 1, S("R", 1)) == S("R", 1), "CHAR(1)");
    CHECK(cellOf(rowst::CAT_STRING, 1, S("\0", 1)) == S("\0", 1), "CHAR(1) NUL");
    CHECK(cellOf(rowst::CAT_STRING, 0, S("", 0)) == S("", 0), "a string of no bytes");
    // numbers: the first width bytes as they are, NULs among them included
    CHECK(cellOf(rowst::CAT_NUMERIC, 4, S("\0\0\0\x80", 4)) == S("\0\0\0\x80", 4), "INT minimum");
    CHECK(cellOf(rowst::CAT_NUMERIC, 8, S("\xff\0\xff\0\xff\0\xff\x7f", 8)) == S("\xff\0\xff\0\xff\0\xff\x7f", 8), "BIGINT bytes");
    CHECK(cellOf(rowst::CAT_NUMERIC, 1, S("\x01", 1)) == S("\x01", 1), "BOOL");
}

static void checkLayout() {
    const RowstoreLayout l = rowstoreLayout(edgeTypes());
    const std::vector<int> offset = {0, 1, 3, 7, 15, 23, 27, 53}, width = {1, 1, 4, 7, 8, 4, 25, 8};
    const std::vector<int> category = {rowst::CAT_NUMERIC, rowst::CAT_STRING, rowst::CAT_NUMERIC, rowst::CAT_STRING, rowst::CAT_NUMERIC, rowst::CAT_NUMERIC,
                                       rowst::CAT_STRING, rowst::CAT_NUMERIC};
    CHECK(l.tupleSize == 61, "tuple size %d", l.tupleSize);
    CHECK(l.offset == offset, "offsets");
    CHECK(l.width == width, "widths");
    CHECK(l.category == category, "categories");
    // a type no column holds: today's error, from the layout already
    std::vector<Type> bad = edgeTypes();
    bad.push_back(Type(RSQ_FLOAT));
    bool raised = false;
    try { (void)rowstoreLayout(bad); }
    catch (const Error& e) { raised = e.status == RSQ_ERR_INVALID && std::string(e.what()) == "unsupported column type"; }
    CHECK(raised, "FLOAT is refused with the host path's error");
}

// one EDGE tuple: every field as the bytes a tuple holds (strings with their junk), 61 bytes in all
static std::string tuple(uint8_t flag, const std::string& code2, int32_t i, const std::string& tag8, int64_t big, uint32_t date, const std::string& text26, int64_t dec) {
    std::string t;
    t.append((const char*)&flag, 1);
    t += code2;
    t.append((const char*)&i, 4);
    t += tag8;
    t.append((const char*)&big, 8);
    t.append((const char*)&date, 4);
    t += text26;
    t.append((const char*)&dec, 8);
    if (t.size() != 61) { fprintf(stderr, "rowstore_test: a hand-written tuple has %zu bytes\n", t.size()); exit(2); }
    return t;
}

// a heap block of exactly the bytes given
static uint8_t* heapBlock(const std::string& bytes) {
    uint8_t* p = (uint8_t*)malloc(bytes.size() ? bytes.size() : 1);
    memcpy(p, bytes.data(), bytes.size());
    return p;
}

template <typename V> static std::string cells(std::initializer_list<V> values) {
    std::string s;
    for (V v : values) s.append((const char*)&v, sizeof v);
    return s;
}
static std::string columnText(const std::vector<uint8_t>& c) { return std::string(c.begin(), c.end()); }

static void checkTranspose() {
    const std::vector<Type> types = edgeTypes();
    const std::string t0 = tuple(1, S("A\x7f", 2), INT32_MIN, S("ab\0QRST\x55", 8), INT64_MIN, 19980802u, S("inner\0nul behind it, junk!", 26), -1);
    const std::string t1 = tuple(0, S("N\x01", 2), INT32_MAX, S("ABCDEFG\x66", 8), INT64_MAX, 19920101u, S("exactly twenty-five bytes\x77", 26), 99999999999999999ll);
    const std::string t2 = tuple(1, S("R\0", 2), -1, S("\0ZZZZZZZ", 8), -1, 0u, S("\0unk junk junk junk junk j", 26), INT64_MIN);
    // block 0: two tuples and a remainder of 5 bytes; block 1: 30 bytes, less than one tuple; block 2: one tuple exactly
    const std::string b0 = t0 + t1 + S("\x11\x22\x33\x44\x55", 5), b1 = std::string(30, '\x5a'), b2 = t2;
    uint8_t* blocks[3] = {heapBlock(b0), heapBlock(b1), heapBlock(b2)};
    const size_t sizes[3] = {b0.size(), b1.size(), b2.size()};
    CHECK(rowstoreRows(sizes, 3, 61) == 3, "rows of the blocks");
    std::vector<std::vector<uint8_t>> cols;
    int64_t n = -1;
    transposeRowstoreHost(types, blocks, sizes, 3, cols, n);
    CHECK(n == 3 && cols.size() == 8, "n = %lld, %zu columns", (long long)n, cols.size());
    if (n == 3 && cols.size() == 8) {
        CHECK(columnText(cols[0]) == S("\x01\0\x01", 3), "BOOL column");
        CHECK(columnText(cols[1]) == S("ANR", 3), "CHAR(1) column: the second byte of the field stays behind");
        CHECK(columnText(cols[2]) == cells<int32_t>({INT32_MIN, INT32_MAX, -1}), "INT column");
        CHECK(columnText(cols[3]) == S("ab", 2) + std::string(5, '\0') + S("ABCDEFG", 7) + std::string(7, '\0'), "CHAR(7) column");
        CHECK(columnText(cols[4]) == cells<int64_t>({INT64_MIN, INT64_MAX, -1}), "BIGINT column (offset 15)");
        CHECK(columnText(cols[5]) == cells<uint32_t>({19980802u, 19920101u, 0u}), "DATE column");
        CHECK(columnText(cols[6]) == S("inner", 5) + std::string(20, '\0') + S("exactly twenty-five bytes", 25) + std::string(25, '\0'), "VARCHAR(25) column");
        CHECK(columnText(cols[7]) == cells<int64_t>({-1, 99999999999999999ll, INT64_MIN}), "DECIMAL column (offset 53)");
    }
    // the same through the header's cell function, field by field
    const RowstoreLayout l = rowstoreLayout(types);
    const std::string* tuples[3] = {&t0, &t1, &t2};
    for (int r = 0; r < 3 && cols.size() == 8; r++)
        for (int c = 0; c < 8; c++) {
            const int w = l.width[(size_t)c];
            const std::string got = cellOf(l.category[(size_t)c], w, tuples[r]->substr((size_t)l.offset[(size_t)c], (size_t)w));
            CHECK(got == columnText(cols[(size_t)c]).substr((size_t)r * (size_t)w, (size_t)w), "row %d column %d", r, c);
        }
    // only a block shorter than one tuple; then no blocks at all
    n = -1;
    transposeRowstoreHost(types, blocks + 1, sizes + 1, 1, cols, n);
    CHECK(n == 0 && cols.size() == 8 && cols[6].empty(), "a block shorter than one tuple holds no rows");
    n = -1;
    transposeRowstoreHost(types, nullptr, nullptr, 0, cols, n);
    CHECK(n == 0 && cols.size() == 8 && cols[0].empty(), "zero blocks");
    for (uint8_t* p : blocks) free(p);
}

int main() {
    checkCells();
    checkLayout();
    checkTranspose();
    if (failures) { fprintf(stderr, "rowstore_test: %d check(s) failed\n", failures); return 1; }
    printf("rowstore_test ok\n");
    return 0;
}
