// Exercises what resql_amd/csrc/dense_groups.h gives the device tail for a dictionary-coded key, on the host: the entries' terms of
// Values::hash (codedKeyHashTerms) against sums computed by hand for CHAR and VARCHAR, and the map from a rank to the smallest rank
// whose entry is equal up to trailing spaces (codedKeyClasses).  Built with the address and undefined-behaviour sanitizers and run by
// tests/test_dict_tail_host.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dense_groups.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "dense_tail_keys_test: %s failed at line %d\n", #c, __LINE__); return 1; } } while (0)

using namespace rsq;

static DenseKey codedKey(int tag, int width, const std::vector<std::string>& entries) {
    DenseKey k;
    k.type = Type(tag); k.type.len = width;
    k.coded = true; k.scanCol = 0; k.card = (int64_t)entries.size();
    k.dict.assign(entries.size() * (size_t)width, 0);                    // as stored: NUL padded to the width, a full-width entry has no NUL
    for (size_t e = 0; e < entries.size(); e++) memcpy(&k.dict[e * (size_t)width], entries[e].data(), entries[e].size());
    return k;
}

// One character's part of hashChar / hashVarchar: (int32)(c * 31636373) + c with c a signed char, both sign-extended to 64 bits.
// By hand: 97 * 31636373 = 3068728181 = 2^32 - 1226239115, so 'a' gives -1226239115 + 97; 32 * 31636373 = 1012363936 stays positive;
// the byte 0xE9 is the character -23: -23 * 31636373 = -727636579, and -23 more.
static const int64_t T_SPACE = 1012363968ll, T_a = -1226239018ll, T_b = -1194602644ll, T_c = -1162966270ll, T_x = -498602416ll, T_z = -435329668ll,
                     T_E9 = -727636602ll;
static uint64_t u(int64_t v) { return (uint64_t)v; }

static int hashTerms() {
    // width 4: the empty entry, 'ab' and 'ab ', two anagrams, a byte >= 0x80, a full-width entry (no NUL behind it: the next entry follows)
    const std::vector<std::string> entries = {"", "ab", "ab ", "abc", "cab", "a\xe9", "zzzz", "x"};
    std::vector<uint64_t> t;
    DenseKey ch = codedKey(RSQ_CHAR, 4, entries);
    codedKeyHashTerms(ch, t);
    CHECK(t.size() == entries.size());
    CHECK(t[0] == u(4 * T_SPACE));                                       // CHAR: the declared length, missing characters count as ' '
    CHECK(t[1] == u(T_a + T_b + 2 * T_SPACE));
    CHECK(t[2] == t[1]);                                                 // 'ab ' = 'ab' to CHAR
    CHECK(t[3] == u(T_a + T_b + T_c + T_SPACE) && t[4] == t[3]);         // anagrams collide
    CHECK(t[5] == u(T_a + T_E9 + 2 * T_SPACE));
    CHECK(t[6] == u(4 * T_z));
    CHECK(t[7] == u(T_x + 3 * T_SPACE));
    CHECK(t[1] == 18446744073313437890ull);                              // ... and one of them as the plain number: -396113726 mod 2^64
    DenseKey vc = codedKey(RSQ_VARCHAR, 4, entries);
    codedKeyHashTerms(vc, t);
    CHECK(t.size() == entries.size());
    CHECK(t[0] == 0);                                                    // VARCHAR: the characters up to the first NUL
    CHECK(t[1] == u(T_a + T_b));
    CHECK(t[2] == u(T_a + T_b + T_SPACE) && t[2] != t[1]);               // two values to VARCHAR
    CHECK(t[3] == u(T_a + T_b + T_c) && t[4] == t[3]);
    CHECK(t[5] == u(T_a + T_E9));
    CHECK(t[6] == u(4 * T_z));                                           // full width: stops at len, not at a NUL
    CHECK(t[7] == u(T_x));
    // the last entry of a dictionary at its full width: nothing is read behind the dictionary's bytes (the sanitizer watches)
    DenseKey last = codedKey(RSQ_CHAR, 2, {"a", "zz"});
    codedKeyHashTerms(last, t);
    CHECK(t.size() == 2 && t[0] == u(T_a + T_SPACE) && t[1] == u(2 * T_z));
    last = codedKey(RSQ_VARCHAR, 2, {"a", "zz"});
    codedKeyHashTerms(last, t);
    CHECK(t.size() == 2 && t[0] == u(T_a) && t[1] == u(2 * T_z));
    return 0;
}

static int classMaps() {
    std::vector<uint32_t> cls;
    // a class of three between other entries (memcmp order, as a dictionary is stored)
    DenseKey three = codedKey(RSQ_CHAR, 3, {"", "a", "x", "x ", "x  ", "xy"});
    CHECK(codedKeyClasses(three, cls));
    CHECK(cls == (std::vector<uint32_t>{0, 1, 2, 2, 2, 5}));
    // the empty value and spaces alone are one value as well
    DenseKey blank = codedKey(RSQ_CHAR, 3, {"", " ", "a ", "a  "});
    CHECK(codedKeyClasses(blank, cls));
    CHECK(cls == (std::vector<uint32_t>{0, 0, 2, 2}));
    // no classes: every rank is its own; leading and inner spaces do not count
    DenseKey none = codedKey(RSQ_CHAR, 3, {"", " a", "a", "a b", "ab"});
    CHECK(!codedKeyClasses(none, cls));
    CHECK(cls == (std::vector<uint32_t>{0, 1, 2, 3, 4}));
    // VARCHAR: trailing spaces are part of the value
    DenseKey vc = codedKey(RSQ_VARCHAR, 3, {"x", "x ", "x  "});
    CHECK(!codedKeyClasses(vc, cls));
    CHECK(cls == (std::vector<uint32_t>{0, 1, 2}));
    // one entry
    DenseKey one = codedKey(RSQ_CHAR, 3, {"x "});
    CHECK(!codedKeyClasses(one, cls));
    CHECK(cls == (std::vector<uint32_t>{0}));
    // a full-width entry ending in spaces, the dictionary's last
    DenseKey full = codedKey(RSQ_CHAR, 2, {"x", "x "});
    CHECK(codedKeyClasses(full, cls));
    CHECK(cls == (std::vector<uint32_t>{0, 0}));
    return 0;
}

int main() {
    if (hashTerms()) return 1;
    if (classMaps()) return 1;
    printf("dense_tail_keys_test ok\n");
    return 0;
}
