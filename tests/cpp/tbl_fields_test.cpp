// Exercises resql_amd/csrc/tbl_fields.h (the plain field forms the device parses) against tblParseLine of tbl.cpp (the host path's
// line function): whatever a plain form accepts, the host accepts with the same cell bytes; every canonical form is plain; the listed
// odd forms are odd; field splitting counts what the host counts.  argv[1]: a file of hex-coded fields, one per line (the fields of
// tests/test_tbl_ingest.py's ACCEPTED / REJECTED lines, written by tests/test_tbl_fields_host.py).  Host code only.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "tbl.h"
#include "tbl_fields.h"

using namespace rsq;

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "tbl_fields_test: %s failed at line %d: ", #c, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); failures++; } } while (0)

static Type typeOf(int tag, int len = 0) { Type t(tag); t.len = len; if (tag == RSQ_DECIMAL) { t.precision = 12; t.scale = 2; } return t; }
// the type categories, strings at three widths (CHAR(1) keeps one byte, CHAR(5) / VARCHAR(8) truncate the long fields)
static const std::vector<Type> kTypes = {typeOf(RSQ_INT), typeOf(RSQ_BIGINT), typeOf(RSQ_DECIMAL), typeOf(RSQ_DATE), typeOf(RSQ_BOOL),
                                         typeOf(RSQ_CHAR, 1), typeOf(RSQ_CHAR, 5), typeOf(RSQ_VARCHAR, 8)};

static bool plain(const Type& t, const std::string& f, uint8_t* cell) {
    const unsigned char* p = (const unsigned char*)f.data();
    const int len = (int)f.size();
    switch (t.tag) {
        case RSQ_INT: { int32_t v; if (!tblf::plainInt(p, len, &v)) return false; memcpy(cell, &v, 4); return true; }
        case RSQ_BIGINT: { int64_t v; if (!tblf::plainBigint(p, len, &v)) return false; memcpy(cell, &v, 8); return true; }
        case RSQ_DECIMAL: { int64_t v; if (!tblf::plainDecimal(p, len, &v)) return false; memcpy(cell, &v, 8); return true; }
        case RSQ_DATE: { uint32_t v; if (!tblf::plainDate(p, len, &v)) return false; memcpy(cell, &v, 4); return true; }
        case RSQ_BOOL: return tblf::plainBool(p, len, cell);
        default: return tblf::plainString(p, len, cell, columnWidth(t));
    }
}

// the host's answer for one field: the field as the only one of a line with a trailing terminator (so that an empty field is a field)
static bool host(const Type& t, const std::string& f, uint8_t* cell) {
    std::string line = f + "|";
    std::vector<char> buf(line.begin(), line.end());
    buf.push_back('\0');
    std::vector<Type> types{t};
    uint8_t* cells[1] = {cell};
    std::string what;
    return tblParseLine(types, buf.data(), line.size(), '|', cells, what) == nullptr;
}

static std::string shown(const std::string& f) {
    std::string s;
    char b[8];
    for (unsigned char c : f) { if (c >= 32 && c < 127) s += (char)c; else { snprintf(b, sizeof b, "\\x%02x", c); s += b; } }
    return s;
}

// plain-accepted => the host accepts, with the same cell bytes.  Returns whether the field is plain.
static bool agree(const Type& t, const std::string& f) {
    uint8_t a[16] = {0}, b[16] = {0};
    if (!plain(t, f, a)) return false;
    const bool ok = host(t, f, b);
    CHECK(ok, "type %d: plain accepts '%s', the host refuses it", t.tag, shown(f).c_str());
    CHECK(memcmp(a, b, 16) == 0, "type %d: cells differ for '%s'", t.tag, shown(f).c_str());
    return true;
}

struct Canon { int type; const char* field; long long value; };      // type: index into kTypes
struct CanonText { int type; const char* field; const char* cell; };

int main(int argc, char** argv) {
    std::vector<std::string> fields;
    if (argc > 1) {
        FILE* f = fopen(argv[1], "r");
        if (!f) { fprintf(stderr, "tbl_fields_test: cannot open %s\n", argv[1]); return 2; }
        char lineBuf[4096];
        while (fgets(lineBuf, sizeof lineBuf, f)) {
            std::string s;
            for (char* p = lineBuf; p[0] && p[1] && p[0] != '\n'; p += 2) { char h[3] = {p[0], p[1], 0}; s += (char)strtol(h, nullptr, 16); }
            fields.push_back(s);
        }
        fclose(f);
        CHECK(fields.size() >= 30, "only %zu fields read", fields.size());
    }
    // the fixed edge list
    for (const char* e : {"999999999", "1000000000", "2147483647", "-2147483648", "-0", "00012", "123456789012345678", "1234567890123456789",
                          "-123456789012345678", "-1234567890123456789", "999999999999999999", "9223372036854775807", "9223372036854775808",
                          ".", "-.", "1.", ".5", "-.5", "1.2.3", "-", "--1", "1-", "1995-3-15", "1995-03/15", "19950-3-15", "1995-03-15x", "1995/03/15",
                          "0000-00-00", "1995-03-15", "true ", "", "true", "false", "TRUE", " 1", "+1", "1 ", "12.5", "-0.07", "3000000000"})
        fields.push_back(e);
    for (const std::string& f : fields) for (const Type& t : kTypes) agree(t, f);

    // 20 000 seeded fields of length 0..12 over the characters the grammars turn on
    {
        static const char alphabet[] = "0123456789-+./ truefalsx";
        unsigned long long state = 20240613ull;
        auto next = [&]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(state >> 33); };
        int plainSeen[8] = {0};
        for (int i = 0; i < 20000; i++) {
            std::string f;
            const int len = (int)(next() % 13);
            for (int k = 0; k < len; k++) f += alphabet[next() % (sizeof alphabet - 1)];
            for (size_t t = 0; t < kTypes.size(); t++) plainSeen[t] += agree(kTypes[t], f) ? 1 : 0;
        }
        // (a random field is never a date or a bool: those forms are met through the lists)
        for (size_t t = 0; t < kTypes.size(); t++) if (t != 3 && t != 4) CHECK(plainSeen[t] > 0, "no seeded field was plain for type %zu", t);
    }

    // every canonical form is plain, with the value the grammar says
    static const Canon canon[] = {
        {0, "0", 0}, {0, "1", 1}, {0, "-3", -3}, {0, "999999999", 999999999}, {0, "-999999999", -999999999}, {0, "00012", 12}, {0, "-0", 0},
        {1, "2", 2}, {1, "-3", -3}, {1, "3000000000", -1294967296ll}, {1, "999999999999999999", (long long)(int32_t)999999999999999999ll},
        {1, "-123456789012345678", (long long)(int32_t)-123456789012345678ll},
        {2, "3.50", 350}, {2, "12.5", 125}, {2, "-0.07", -7}, {2, "7", 7}, {2, "-.5", -5}, {2, "1.", 1}, {2, ".5", 5}, {2, "123456789012345.678", 123456789012345678ll},
        {3, "1995-03-15", 19950315}, {3, "1995/03/15", 19950315}, {3, "1992-01-01", 19920101}, {3, "0000-00-00", 0}, {3, "9999/99/99", 99999999},
        {4, "true", 1}, {4, "false", 0},
    };
    for (const Canon& c : canon) {
        uint8_t cell[16] = {0};
        const Type& t = kTypes[(size_t)c.type];
        CHECK(plain(t, c.field, cell), "canonical form '%s' of type %d is not plain", c.field, t.tag);
        long long got = 0;
        if (columnWidth(t) == 8) { int64_t v; memcpy(&v, cell, 8); got = v; }
        else if (columnWidth(t) == 4 && t.tag == RSQ_INT) { int32_t v; memcpy(&v, cell, 4); got = v; }
        else if (columnWidth(t) == 4) { uint32_t v; memcpy(&v, cell, 4); got = v; }
        else got = cell[0];
        CHECK(got == c.value, "'%s' of type %d reads %lld, not %lld", c.field, t.tag, got, c.value);
        agree(t, c.field);
    }
    static const CanonText texts[] = {
        {5, "A", "A"}, {5, "", ""}, {5, "toolong", "t"}, {6, "abc", "abc"}, {6, "toolongvalue", "toolo"}, {6, "a b", "a b"}, {6, "\t", "\t"},
        {7, "hello", "hello"}, {7, "toolongvalue", "toolongv"}, {7, "hello\r", "hello\r"}, {7, "  ", "  "},
    };
    for (const CanonText& c : texts) {
        uint8_t cell[16] = {0}, want[16] = {0};
        const Type& t = kTypes[(size_t)c.type];
        memcpy(want, c.cell, strlen(c.cell));
        CHECK(plain(t, c.field, cell), "text '%s' is not plain", c.field);
        CHECK(memcmp(cell, want, 16) == 0, "text '%s' at width %d", c.field, columnWidth(t));
        agree(t, c.field);
    }
    { uint8_t cell[16] = {0}; CHECK(!plain(kTypes[7], std::string("ab\0cd", 5), cell), "a field with a NUL is odd"); }

    // ... and the forms that are odd on purpose
    static const struct { int type; const char* field; } odd[] = {
        {0, "1000000000"}, {0, "2147483647"}, {0, " 7"}, {0, "+8"}, {0, "9abc"}, {0, ""}, {0, "-"}, {0, "1 "}, {0, "x"},
        {1, "1234567890123456789"}, {1, "+8"}, {1, "10xyz"}, {1, ""},
        {2, "."}, {2, "-."}, {2, "-"}, {2, "1.2.3"}, {2, ""}, {2, "1234567890123456789"}, {2, "+1.5"}, {2, " 1.5"},
        {3, "1995-3-15"}, {3, "1995/3/5"}, {3, "1995-03/15"}, {3, "19950-3-15"}, {3, "1995-03-15x"}, {3, "1998-12-31trailing"}, {3, "15.03.1995"}, {3, ""},
        {4, "true "}, {4, "yes"}, {4, ""}, {4, "TRUE"},
    };
    for (const auto& o : odd) { uint8_t cell[16] = {0}; CHECK(!plain(kTypes[(size_t)o.type], o.field, cell), "'%s' of type %d must be odd", o.field, kTypes[(size_t)o.type].tag); }

    // field splitting: as many fields as the host finds (the k for which a line of k VARCHAR columns is neither short nor long)
    for (const char* l : {"a|b", "a|b|", "a||b|", "|", "", "||", "a", "a|\r", "|a"}) {
        const std::string line = l;
        int hostFields = -1;
        for (int k = 0; k <= 6 && hostFields < 0; k++) {
            std::vector<Type> types((size_t)k, typeOf(RSQ_VARCHAR, 8));
            std::vector<std::vector<uint8_t>> store((size_t)k, std::vector<uint8_t>(8, 0));
            std::vector<uint8_t*> cells;
            for (auto& s : store) cells.push_back(s.data());
            std::vector<char> buf(line.begin(), line.end());
            buf.push_back('\0');
            std::string what;
            if (!tblParseLine(types, buf.data(), line.size(), '|', cells.data(), what)) hostFields = k;
        }
        const int got = tblf::countFields((const unsigned char*)line.data(), (int)line.size(), '|');
        CHECK(got == hostFields, "'%s' splits into %d fields, the host finds %d", shown(line).c_str(), got, hostFields);
    }
    // the three messages of the line function, as parseTblFile reported them
    {
        std::vector<Type> types{typeOf(RSQ_INT), typeOf(RSQ_BOOL)};
        uint8_t a[4] = {0}, b[1] = {0};
        uint8_t* cells[2] = {a, b};
        std::string what;
        auto run = [&](const char* l) { std::string s = l; std::vector<char> buf(s.begin(), s.end()); buf.push_back('\0'); const char* r = tblParseLine(types, buf.data(), s.size(), '|', cells, what); return std::string(r ? r : "(ok)"); };
        CHECK(run("1|true|") == "(ok)", "%s", what.c_str());
        CHECK(run("1|") == "is missing attributes.", "%s", what.c_str());
        CHECK(run("1|true|x|") == "contains extra attributes.", "%s", what.c_str());
        CHECK(run("1|yes|") == "field 2: Couldnt parse BOOL constant.", "%s", what.c_str());
        CHECK(run("x|true|") == "field 1: stoi: no conversion", "%s", what.c_str());
    }
    if (failures) { fprintf(stderr, "tbl_fields_test: %d check(s) failed\n", failures); return 1; }
    printf("tbl_fields_test ok (%zu listed fields)\n", fields.size());
    return 0;
}
