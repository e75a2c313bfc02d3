// result_text.h — the text of one result cell, for both sides: what serializeSqlValue (expr.cpp) prints for loadValue (hostref.cpp) of
// the cell, byte for byte, quirks included.  Those two stay the definition; this header is checked against them
// (tests/cpp/result_text_test.cpp) and is what the device path (result_text.hip) writes:
//   INT / BIGINT     std::to_string of the signed value
//   DECIMAL(p, s)    '-' when raw < 0, then the digits of the magnitude formed as a SIGNED negation (INT64_MIN keeps its own '-': the
//                    text starts with two), zeros in front up to s + 1 digits, the point s places from the right (none when s <= 0)
//   DATE             the cell as uint32: to_string(v / 10000) '/' two digits of v / 100 % 100 '/' two digits of v % 100, not validated
//   BOOL             true / false
//   CHAR(n), n > 1   the bytes up to the first NUL, then blanks up to n; no byte at or beyond n is read (the host's strlen stops at
//                    byte n of a well-formed field, which has n + 1 bytes)
//   CHAR(n), n <= 1  the byte, or nothing when it is NUL, then blanks up to n
//   VARCHAR(n)       the bytes up to the first NUL, the same bound
// len_or_scale is the scale of a DECIMAL and n of a CHAR / VARCHAR.  No std::string, no libc.  Compiled by hipcc for both sides and by
// g++ for the host alone.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define RTXT_FN __host__ __device__ __forceinline__
#else
#define RTXT_FN inline
#endif

namespace rsq {
namespace rtxt {

enum Category { CAT_INT = 0, CAT_BIGINT = 1, CAT_DECIMAL = 2, CAT_DATE = 3, CAT_BOOL = 4, CAT_CHAR = 5, CAT_VARCHAR = 6 };

// cells lie at any byte offset of a packed tuple
RTXT_FN uint32_t load32(const unsigned char* p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
RTXT_FN uint64_t load64(const unsigned char* p) { uint64_t v; __builtin_memcpy(&v, p, 8); return v; }

// decimal digits of v (1 for 0): one comparison per power of ten, no branch
RTXT_FN int countDigits(uint64_t v) {
    int n = 1;
    uint64_t p = 10;
    for (int i = 1; i < 20; i++) { n += v >= p ? 1 : 0; p *= 10; }          // (the last product wraps and is not used)
    return n;
}

// the digits of v, two at a time, so that the last one lands on end[-1]; exactly countDigits(v) bytes are written
RTXT_FN void writeDigitsBackwards(uint64_t v, unsigned char* end) {
    while (v >= 100) {
        const uint64_t q = v / 100;
        const unsigned r = (unsigned)(v - q * 100), t = r / 10;
        *--end = (unsigned char)('0' + (r - t * 10));
        *--end = (unsigned char)('0' + t);
        v = q;
    }
    const unsigned r = (unsigned)v, t = r / 10;
    *--end = (unsigned char)('0' + (r - t * 10));
    if (t) *--end = (unsigned char)('0' + t);
}

// std::to_string(long long)
RTXT_FN uint64_t magnitude(int64_t v) { return v < 0 ? 0 - (uint64_t)v : (uint64_t)v; }
RTXT_FN int signedLength(int64_t v) { return (v < 0 ? 1 : 0) + countDigits(magnitude(v)); }
RTXT_FN int writeSigned(int64_t v, unsigned char* out) {
    const int n = signedLength(v);
    if (v < 0) out[0] = '-';
    writeDigitsBackwards(magnitude(v), out + n);
    return n;
}

// the digit string of a DECIMAL: to_string of the signed magnitude (raw < 0 ? -raw : raw, which wraps for INT64_MIN alone)
RTXT_FN int64_t decimalMagnitude(int64_t raw) { return raw < 0 ? (int64_t)(0 - (uint64_t)raw) : raw; }
RTXT_FN int decimalLength(int64_t raw, int scale) {
    const int places = scale > 0 ? scale : 0;
    int digits = signedLength(decimalMagnitude(raw));
    if (digits <= places) digits = places + 1;
    return (raw < 0 ? 1 : 0) + digits + (places > 0 ? 1 : 0);
}
RTXT_FN int writeDecimal(int64_t raw, int scale, unsigned char* out) {
    const int places = scale > 0 ? scale : 0;
    const int64_t m = decimalMagnitude(raw);
    const int have = signedLength(m);
    const int digits = have <= places ? places + 1 : have;
    unsigned char* p = out;
    if (raw < 0) *p++ = '-';
    // zeros in front, the digit string behind them, then the last `places` characters move one to the right for the point
    for (int i = 0; i < digits - have; i++) p[i] = '0';
    writeSigned(m, p + (digits - have));
    if (places > 0) {
        for (int k = 0; k < places; k++) p[digits - k] = p[digits - k - 1];
        p[digits - places] = '.';
    }
    return (int)(p - out) + digits + (places > 0 ? 1 : 0);
}

// bytes of a string cell in front of its first NUL, never reading at or beyond byte n
RTXT_FN int boundedLength(const unsigned char* cell, int n) {
    int have = 0;
    while (have < n && cell[have] != 0) have++;
    return have;
}

RTXT_FN int cellTextLength(int category, int lenOrScale, const unsigned char* cell) {
    switch (category) {
        case CAT_INT: return signedLength((int64_t)(int32_t)load32(cell));
        case CAT_BIGINT: return signedLength((int64_t)load64(cell));
        case CAT_DECIMAL: return decimalLength((int64_t)load64(cell), lenOrScale);
        case CAT_DATE: return countDigits(load32(cell) / 10000u) + 6;
        case CAT_BOOL: return cell[0] ? 4 : 5;
        case CAT_CHAR: {
            if (lenOrScale > 1) return lenOrScale;                        // (whatever it holds, it is padded to n)
            const int have = cell[0] ? 1 : 0, n = lenOrScale > 0 ? lenOrScale : 0;
            return have < n ? n : have;
        }
        default: return boundedLength(cell, lenOrScale);
    }
}

// writes exactly cellTextLength bytes and returns their number
RTXT_FN int writeCellText(int category, int lenOrScale, const unsigned char* cell, unsigned char* out) {
    switch (category) {
        case CAT_INT: return writeSigned((int64_t)(int32_t)load32(cell), out);
        case CAT_BIGINT: return writeSigned((int64_t)load64(cell), out);
        case CAT_DECIMAL: return writeDecimal((int64_t)load64(cell), lenOrScale, out);
        case CAT_DATE: {
            const uint32_t v = load32(cell);
            const unsigned day = v % 100u, month = v / 100u % 100u;
            const int n = countDigits(v / 10000u);
            writeDigitsBackwards(v / 10000u, out + n);
            out[n] = '/'; out[n + 1] = (unsigned char)('0' + month / 10); out[n + 2] = (unsigned char)('0' + month % 10);
            out[n + 3] = '/'; out[n + 4] = (unsigned char)('0' + day / 10); out[n + 5] = (unsigned char)('0' + day % 10);
            return n + 6;
        }
        case CAT_BOOL:
            if (cell[0]) { out[0] = 't'; out[1] = 'r'; out[2] = 'u'; out[3] = 'e'; return 4; }
            out[0] = 'f'; out[1] = 'a'; out[2] = 'l'; out[3] = 's'; out[4] = 'e';
            return 5;
        case CAT_CHAR: {
            const int n = lenOrScale > 0 ? lenOrScale : 0;
            int have;
            if (lenOrScale > 1) { have = 0; while (have < n && cell[have] != 0) { out[have] = cell[have]; have++; } }
            else { have = cell[0] ? 1 : 0; if (have) out[0] = cell[0]; }
            for (int i = have; i < n; i++) out[i] = ' ';
            return have < n ? n : have;
        }
        default: {
            int have = 0;
            while (have < lenOrScale && cell[have] != 0) { out[have] = cell[have]; have++; }
            return have;
        }
    }
}

// an upper bound of cellTextLength from the type alone (a DECIMAL's scale is at most 18 wherever this bound is relied on)
RTXT_FN int maxCellTextLength(int category, int lenOrScale) {
    switch (category) {
        case CAT_INT: return 11;                                          // -2147483648
        case CAT_BIGINT: return 20;                                       // -9223372036854775808
        case CAT_DECIMAL: {                                               // '-', the smallest value's own '-' + 19 digits (or s + 1 digits), the point
            const int places = lenOrScale > 0 ? lenOrScale : 0;
            return 1 + (places + 1 > 20 ? places + 1 : 20) + (places > 0 ? 1 : 0);
        }
        case CAT_DATE: return 12;                                         // 429496/72/95
        case CAT_BOOL: return 5;
        case CAT_CHAR: return lenOrScale > 1 ? lenOrScale : 1;
        default: return lenOrScale > 0 ? lenOrScale : 0;
    }
}

}  // namespace rtxt
}  // namespace rsq
