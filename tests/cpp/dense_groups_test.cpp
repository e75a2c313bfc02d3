// Exercises resql_amd/csrc/dense_groups.h on the host: a dense aggregate table whose key is a dictionary code becomes groups whose key
// value is dictionary entry `rank`, NUL-terminated at len + 1, for CHAR and VARCHAR at widths 2, 9 and 25 - alone, mixed with a numeric
// range key and a byte-set key, from the whole table (groupsFromDense) and from candidate rows (groupsFromDenseRows).  Built with the
// address and undefined-behaviour sanitizers and run by tests/test_dict_group_codegen.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dense_groups.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "dense_groups_test: %s failed at line %d\n", #c, __LINE__); return 1; } } while (0)

using namespace rsq;

static DenseKey codedKey(int tag, int width, const std::vector<std::string>& entries) {
    DenseKey k;
    k.type = Type(tag); k.type.len = width;
    k.coded = true; k.scanCol = 0; k.card = (int64_t)entries.size();
    k.dict.assign(entries.size() * (size_t)width, 0);                    // as stored: NUL padded to the width, a full-width entry has no NUL
    for (size_t e = 0; e < entries.size(); e++) memcpy(&k.dict[e * (size_t)width], entries[e].data(), entries[e].size());
    return k;
}

static void setStrides(std::vector<DenseKey>& keys) {
    int64_t stride = 1;
    for (size_t i = keys.size(); i-- > 0;) { keys[i].stride = stride; stride *= keys[i].card; }
}

static int oneCodedKey(int tag, int width) {
    // entries in memcmp order; the empty value, a one-byte value, 'ab' against 'ab ' where they fit, a value of the full width
    std::vector<std::string> entries = {"", "a", "ab"};
    if (width >= 3) entries.push_back("ab ");
    entries.push_back(std::string((size_t)width, 'z'));
    std::vector<DenseKey> keys = {codedKey(tag, width, entries)};
    setStrides(keys);
    const int64_t D = keys[0].card;
    const std::vector<int> accumSlot = {0, 1};                             // [first row | count]
    std::vector<uint64_t> table((size_t)(2 * D));
    for (int64_t g = 0; g < D; g++) { table[(size_t)g] = (uint64_t)INT64_MAX; table[(size_t)(D + g)] = 0; }
    for (int64_t g = 0; g < D; g++) if (g != 1) { table[(size_t)g] = (uint64_t)(100 - g); table[(size_t)(D + g)] = (uint64_t)(10 + g); }      // entry 1 has no rows
    Groups G;
    groupsFromDense(keys, D, accumSlot, table.data(), G);
    CHECK(G.n == (size_t)D - 1 && G.nKeys == 1 && G.nAcc == 2);
    CHECK(G.strings.size() == G.n * (size_t)(width + 1));
    size_t o = 0;
    for (int64_t g = 0; g < D; g++) {
        if (g == 1) continue;
        const char* s = G.keys(o)[0].s;
        const std::string& want = entries[(size_t)g];
        CHECK(s >= G.strings.data() && s + width + 1 <= G.strings.data() + G.strings.size());
        CHECK(memcmp(s, &keys[0].dict[(size_t)g * (size_t)width], (size_t)width) == 0);      // rank -> the entry's bytes as stored
        CHECK(s[width] == 0);                                                                  // the terminator at len + 1
        CHECK(strlen(s) == want.size() && want == s);
        CHECK(G.firstRow[o] == 100 - g && G.acc(o)[0] == 100 - g && G.acc(o)[1] == 10 + g);
        o++;
    }
    // the same groups as candidate rows [first row | group id | blocks], in another order
    std::vector<int64_t> rows;
    for (int64_t g = D - 1; g >= 0; g--) if (g != 1) { rows.push_back(100 - g); rows.push_back(g); rows.push_back(100 - g); rows.push_back(10 + g); }
    Groups R;
    groupsFromDenseRows(keys, accumSlot, rows.data(), rows.size() / 4, 4, R);
    CHECK(R.n == G.n);
    for (size_t i = 0; i < R.n; i++) {
        const int64_t g = rows[i * 4 + 1];
        CHECK(entries[(size_t)g] == R.keys(i)[0].s && R.keys(i)[0].s[width] == 0 && R.acc(i)[1] == 10 + g);
    }
    return 0;
}

static int mixedKeys() {
    // [numeric 5..7] x [coded VARCHAR(9), 3 entries] x [byte set {A, N, R}] x [coded CHAR(2), 2 entries]: id = ranks in mixed radix
    std::vector<DenseKey> keys(4);
    keys[0].type = Type(RSQ_BIGINT); keys[0].min = 5; keys[0].card = 3;
    keys[1] = codedKey(RSQ_VARCHAR, 9, {"", "MAIL", "full9byte"});
    keys[2].type = Type(RSQ_CHAR); keys[2].type.len = 1; keys[2].byteSet = true; keys[2].values = {'A', 'N', 'R'}; keys[2].card = 3;
    keys[3] = codedKey(RSQ_CHAR, 2, {"a", "zz"});
    setStrides(keys);
    const int64_t D = 3 * 3 * 3 * 2;
    CHECK(keys[0].stride == 18 && keys[1].stride == 6 && keys[2].stride == 2 && keys[3].stride == 1);
    const std::vector<int> accumSlot = {1, 0};                             // (the first-row block is not the first one)
    std::vector<uint64_t> table((size_t)(2 * D));
    for (int64_t g = 0; g < D; g++) { table[(size_t)(D + g)] = g % 5 == 0 ? (uint64_t)INT64_MAX : (uint64_t)g; table[(size_t)g] = (uint64_t)(g * 3); }
    Groups G;
    groupsFromDense(keys, D, accumSlot, table.data(), G);
    CHECK(G.strings.size() == G.n * (size_t)(10 + 3));
    size_t o = 0;
    const char* v9[] = {"", "MAIL", "full9byte"};
    const char* v2[] = {"a", "zz"};
    for (int64_t g = 0; g < D; g++) {
        if (g % 5 == 0) continue;
        const Val* k = G.keys(o);
        CHECK(k[0].i == 5 + g / 18);
        CHECK(strcmp(k[1].s, v9[(g / 6) % 3]) == 0 && k[1].s[9] == 0);
        CHECK(k[2].i == "ANR"[(g / 2) % 3]);
        CHECK(strcmp(k[3].s, v2[g % 2]) == 0 && k[3].s[2] == 0);
        CHECK(k[3].s == k[1].s + 10);                                      // a group's strings stand one behind the other
        CHECK(G.firstRow[o] == g && G.acc(o)[1] == g * 3);
        o++;
    }
    CHECK(o == G.n);
    return 0;
}

static int manyGroups() {
    // enough groups for several host threads (hostpar.h partsFor): every part fills its own slice of the strings
    std::vector<std::string> entries;
    for (int e = 0; e < 256; e++) { char b[8]; snprintf(b, sizeof b, "v%03d", e); entries.push_back(b); }
    std::vector<DenseKey> keys(2);
    keys[0] = codedKey(RSQ_VARCHAR, 25, entries);
    keys[1].type = Type(RSQ_BIGINT); keys[1].min = -3; keys[1].card = 1000;
    setStrides(keys);
    const int64_t D = 256 * 1000;
    const std::vector<int> accumSlot = {0};
    std::vector<uint64_t> table((size_t)D);
    for (int64_t g = 0; g < D; g++) table[(size_t)g] = g % 3 ? (uint64_t)g : (uint64_t)INT64_MAX;
    Groups G;
    groupsFromDense(keys, D, accumSlot, table.data(), G);
    CHECK(G.n == (size_t)(D - (D + 2) / 3));
    for (size_t o = 0; o < G.n; o++) {
        const int64_t g = G.firstRow[o];
        CHECK(entries[(size_t)(g / 1000)] == G.keys(o)[0].s && G.keys(o)[0].s[25] == 0 && G.keys(o)[1].i == -3 + g % 1000);
    }
    return 0;
}

int main() {
    for (int tag : {RSQ_CHAR, RSQ_VARCHAR})
        for (int width : {2, 9, 25})
            if (oneCodedKey(tag, width)) return 1;
    if (mixedKeys() || manyGroups()) return 1;
    printf("dense_groups_test ok\n");
    return 0;
}
