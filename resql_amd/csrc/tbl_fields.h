// tbl_fields.h — the PLAIN field forms of '.tbl' text: what the device parser (tbl_device.hip) reads itself.  Everything else is
// ODD and goes, with its whole line, to the host's line function (tbl.h tblParseLine), which is the definition of BULK INSERT.
// The forms were chosen so that each of them means the same under strtol, strtoll and sscanf - the routines tbl.cpp reaches:
//   INT              -?[0-9]{1,9} to the end of the field          (cannot overflow)
//   BIGINT           -?[0-9]{1,18}                                  -> (int64)(int32)value, as tbl.cpp stores it
//   DECIMAL          -? then digits with at most one '.' anywhere among them, 1..18 digits in all -> the digits without the point
//   DATE             dddd-dd-dd or dddd/dd/dd, the same separator twice -> y * 10000 + m * 100 + d, not validated
//   BOOL             true / false
//   CHAR / VARCHAR   any bytes without NUL -> the first min(n, len) bytes; the rest of the cell stays 0
// Leading blanks, '+', trailing garbage, 10-digit INTs, 1995/3/5 and 1.2.3 are odd on purpose.  Compiled by hipcc for both sides
// and by g++ for the host alone (tests/cpp/tbl_fields_test.cpp).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define TBL_FN __host__ __device__ __forceinline__
#else
#define TBL_FN inline
#endif

namespace rsq {
namespace tblf {

// type categories of the kernel's schema (tbl_device.hip TblSchema)
enum Category { CAT_INT = 0, CAT_BIGINT = 1, CAT_DECIMAL = 2, CAT_DATE = 3, CAT_BOOL = 4, CAT_STRING = 5 };

TBL_FN bool isDigit(unsigned char c) { return (unsigned)(c - '0') <= 9u; }

// -?[0-9]{1,maxDigits} to the end of the field
TBL_FN bool plainInteger(const unsigned char* f, int len, int maxDigits, long long* out) {
    int i = 0;
    const bool neg = len > 0 && f[0] == '-';
    if (neg) i = 1;
    const int digits = len - i;
    if (digits < 1 || digits > maxDigits) return false;
    long long v = 0;
    for (; i < len; i++) {
        if (!isDigit(f[i])) return false;
        v = v * 10 + (long long)(f[i] - '0');
    }
    *out = neg ? -v : v;
    return true;
}

TBL_FN bool plainInt(const unsigned char* f, int len, int32_t* cell) {
    long long v;
    if (!plainInteger(f, len, 9, &v)) return false;
    *cell = (int32_t)v;
    return true;
}

TBL_FN bool plainBigint(const unsigned char* f, int len, int64_t* cell) {
    long long v;
    if (!plainInteger(f, len, 18, &v)) return false;
    *cell = (int64_t)(int32_t)v;
    return true;
}

TBL_FN bool plainDecimal(const unsigned char* f, int len, int64_t* cell) {
    int i = 0, digits = 0, points = 0;
    const bool neg = len > 0 && f[0] == '-';
    if (neg) i = 1;
    long long v = 0;
    for (; i < len; i++) {
        if (f[i] == '.') { if (++points > 1) return false; continue; }
        if (!isDigit(f[i]) || ++digits > 18) return false;
        v = v * 10 + (long long)(f[i] - '0');
    }
    if (digits < 1) return false;
    *cell = neg ? -v : v;
    return true;
}

TBL_FN bool plainDate(const unsigned char* f, int len, uint32_t* cell) {
    if (len != 10 || (f[4] != '-' && f[4] != '/') || f[7] != f[4]) return false;
    unsigned v[3] = {0, 0, 0};
    for (int i = 0; i < 10; i++) {
        if (i == 4 || i == 7) continue;
        if (!isDigit(f[i])) return false;
        const int part = i < 4 ? 0 : i < 7 ? 1 : 2;
        v[part] = v[part] * 10 + (unsigned)(f[i] - '0');
    }
    *cell = v[0] * 10000u + v[1] * 100u + v[2];
    return true;
}

TBL_FN bool plainBool(const unsigned char* f, int len, uint8_t* cell) {
    if (len == 4 && f[0] == 't' && f[1] == 'r' && f[2] == 'u' && f[3] == 'e') { *cell = 1; return true; }
    if (len == 5 && f[0] == 'f' && f[1] == 'a' && f[2] == 'l' && f[3] == 's' && f[4] == 'e') { *cell = 0; return true; }
    return false;
}

// (the cell is `width` bytes, zero before the call; a NUL anywhere in the field makes it odd, also behind the bytes that are kept)
TBL_FN bool plainString(const unsigned char* f, int len, uint8_t* cell, int width) {
    for (int i = 0; i < len; i++) if (f[i] == 0) return false;
    const int n = len < width ? len : width;
    for (int i = 0; i < n; i++) cell[i] = f[i];
    return true;
}

// Field splitting, the way std::getline(line, token, terminator) splits: fields end at the terminator, a terminator as the line's last
// byte yields no further field, an empty line has no fields, a '\r' is an ordinary byte.  *pos: where the next field starts (0 at
// first); false: the line has no further field.
TBL_FN bool nextField(const unsigned char* line, int len, unsigned char terminator, int* pos, int* begin, int* fieldLen) {
    const int b = *pos;
    if (b >= len) return false;
    int e = b;
    while (e < len && line[e] != terminator) e++;
    *begin = b; *fieldLen = e - b;
    *pos = e < len ? e + 1 : len;
    return true;
}

TBL_FN int countFields(const unsigned char* line, int len, unsigned char terminator) {
    int pos = 0, b, l, n = 0;
    while (nextField(line, len, terminator, &pos, &b, &l)) n++;
    return n;
}

}  // namespace tblf
}  // namespace rsq
