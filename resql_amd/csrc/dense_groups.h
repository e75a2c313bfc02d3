// dense_groups.h — the keys of a dense aggregation and the step from its [block][group] table to the groups the host tail works on.
//
// Kept apart from tail.cpp so that it stands on expr.h and hostpar.h alone: tests/cpp/dense_groups_test.cpp feeds it hand-made tables
// under the address and undefined-behaviour sanitizers, without a device or the rest of the engine.
#pragma once

#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "expr.h"
#include "hostpar.h"

namespace rsq {

struct Table;

struct DenseKey {
    Expr* expr = nullptr;
    Type type;
    bool byteSet = false;
    std::vector<uint8_t> values;     // byteSet: sorted distinct values
    int64_t min = 0;
    int64_t card = 1;
    int64_t stride = 1;
    // coded: a dictionary-coded string column of the pipeline's scan (engine.h TableColumn::dict) - the rank is the row's u8 code, card
    // the dictionary's entry count.  `dict` is the statement's own copy of the card x width entry bytes, for its tail; scanCol is the
    // column's place among the pipeline's scanned columns (the code is the row-function parameter vc_<scanCol>).
    // ... or, with scanCol -1, a string carried from a join's build side whose address points into the dictionary of column originCol of
    // originTable (engine_internal.h HashTable::DictOrigin): the rank is (address - dictionary) / width, card and dict are that column's.
    // The tails read card, dict and type alone and do not tell the two apart.
    bool coded = false;
    int scanCol = -1;
    const Table* originTable = nullptr;
    int originCol = -1;
    std::vector<uint8_t> dict;
    bool shared = false;             // ... and every shard holds that dictionary (engine.h TableColumn::dictShared): the table merges with the shards'
    bool spaceEquivalent = false;    // coded CHAR(n): two entries are equal up to trailing spaces - one group to the reference (tail.cpp mergeEqualGroups)
};
inline bool anyCodedKey(const std::vector<DenseKey>& keys) { for (auto& k : keys) if (k.coded) return true; return false; }

// ---- the groups the device produced ---------------------------------------------------------------
struct Groups {
    size_t n = 0, nKeys = 0, nAcc = 0;
    std::vector<int64_t> firstRow;                 // [n]
    std::vector<Val> keyData;                      // [n][nKeys], flat
    std::vector<int64_t> accData;                  // [n][nAcc], flat (index = accums index)
    std::vector<char> strings;                     // NUL-terminated bytes of string key values (Val::s points in here)
    const Val* keys(size_t i) const { return keyData.data() + i * nKeys; }
    const int64_t* acc(size_t i) const { return accData.data() + i * nAcc; }
};

// A dictionary-coded key's value is entry `rank` of the statement's copy of the dictionary (DenseKey::dict), handed on as the hash
// aggregation hands on a string group value: its bytes in Groups::strings, NUL-terminated at len + 1 (tail.cpp groupsFromJoinEntries).
// Everything downstream - Values::hash for the emission order, ORDER BY, projections, the tuple writer - then reads it as before.
inline size_t codedKeyBytes(const std::vector<DenseKey>& keys) {
    size_t b = 0;
    for (auto& dk : keys) if (dk.coded) b += (size_t)dk.type.len + 1;
    return b;
}
inline Val denseKeyValue(const DenseKey& dk, int64_t rank, char* strings, size_t& sp) {
    Val v;
    if (dk.coded) {
        const size_t w = (size_t)dk.type.len;
        memcpy(strings + sp, dk.dict.data() + (size_t)rank * w, w);
        strings[sp + w] = 0;
        v.s = strings + sp;
        sp += w + 1;
    } else v.i = dk.byteSet ? (int64_t)dk.values[(size_t)rank] : dk.min + rank;
    return v;
}

// ---- a coded key in the device tail (devtail.hip) -------------------------------------------------
// Values::hash adds a string value's contribution to the running sum (hostref.cpp refHashValue, the CHAR(n > 1) and VARCHAR cases), so a
// coded key's part of a group's hash depends on its rank alone: term[rank] = refHashValue(0, entry, type).  The two loops are restated
// here (this header does not see hostref.h) with the same character arithmetic: a signed char, a 32-bit multiply, sign extension.
inline uint64_t codedEntryHashTerm(const uint8_t* entry, const Type& t) {
    const char* s = (const char*)entry;
    uint64_t h = 0;
    if (t.tag == RSQ_CHAR) {       // hashChar: the declared length, missing characters count as ' '
        bool ended = false;
        for (int i = 0; i < t.len; i++) {
            char c;
            if (!ended && s[i] != '\0') c = s[i]; else { ended = true; c = ' '; }
            const int32_t m = (int32_t)((uint32_t)(int)c * 31636373u);
            h = h + (uint64_t)(int64_t)m + (uint64_t)(int64_t)c;
        }
        return h;
    }
    for (int i = 0; i < t.len && s[i] != '\0'; i++) {      // hashVarchar: the characters up to the first NUL
        const int c = s[i];
        const int32_t m = (int32_t)((uint32_t)c * 31636373u);
        h = h + (uint64_t)(int64_t)m + (uint64_t)(int64_t)c;
    }
    return h;
}
inline void codedKeyHashTerms(const DenseKey& dk, std::vector<uint64_t>& terms) {
    const size_t w = (size_t)dk.type.len;
    terms.resize((size_t)dk.card);
    for (size_t e = 0; e < (size_t)dk.card; e++) terms[e] = codedEntryHashTerm(dk.dict.data() + e * w, dk.type);
}
// rank -> the smallest rank whose entry is the same value to the reference: CHAR(n) entries are equal up to trailing spaces (the rule of
// codegen_agg.cpp tryDenseKeys and tail.cpp mergeEqualGroups), VARCHAR entries only when they are the same entry.  true: some rank moved.
inline bool codedKeyClasses(const DenseKey& dk, std::vector<uint32_t>& cls) {
    const size_t w = (size_t)dk.type.len;
    cls.resize((size_t)dk.card);
    bool any = false;
    std::map<std::string, uint32_t> first;
    for (size_t e = 0; e < (size_t)dk.card; e++) {
        cls[e] = (uint32_t)e;
        if (dk.type.tag != RSQ_CHAR) continue;
        const char* v = (const char*)dk.dict.data() + e * w;
        size_t n = strnlen(v, w);
        while (n > 0 && v[n - 1] == ' ') n--;
        auto at = first.emplace(std::string(v, n), (uint32_t)e);
        if (!at.second) { cls[e] = at.first->second; any = true; }
    }
    return any;
}

// table: [block][group] words, accumulator w in block accumSlot[w]; a group is present when its first-row word is not INT64_MAX
inline void groupsFromDense(const std::vector<DenseKey>& keys, int64_t D, const std::vector<int>& accumSlot, const uint64_t* table, Groups& G) {
    const size_t W = accumSlot.size();
    auto word = [&](size_t w, int64_t g) { return (int64_t)table[(size_t)(accumSlot[w] * D + g)]; };
    G.nKeys = keys.size(); G.nAcc = W;
    // two passes over the dense table, both split over the host threads: count the groups present per part, then
    // fill each part's slice (group order = dense id order, as before)
    const int parts = partsFor((size_t)D);
    std::vector<size_t> cnt((size_t)parts + 1, 0);
    parallelRanges((size_t)D, parts, [&](size_t b, size_t e, int p) {
        size_t c = 0;
        for (size_t g = b; g < e; g++) if (word(0, (int64_t)g) != INT64_MAX) c++;
        cnt[(size_t)p + 1] = c;
    });
    for (int p = 0; p < parts; p++) cnt[(size_t)p + 1] += cnt[(size_t)p];
    const size_t present = cnt[(size_t)parts];
    G.n = present;
    G.firstRow.resize(present); G.keyData.resize(present * G.nKeys); G.accData.resize(present * W);
    const size_t strBytes = codedKeyBytes(keys);
    G.strings.assign(present * strBytes, 0);
    parallelRanges((size_t)D, parts, [&](size_t b, size_t e, int p) {
        size_t o = cnt[(size_t)p];
        for (size_t gi = b; gi < e; gi++) {
            const int64_t g = (int64_t)gi;
            if (word(0, g) == INT64_MAX) continue;
            G.firstRow[o] = word(0, g);
            size_t k = 0, sp = o * strBytes;
            for (auto& dk : keys) {
                int64_t rank = (g / dk.stride) % dk.card;
                G.keyData[o * G.nKeys + k++] = denseKeyValue(dk, rank, G.strings.data(), sp);
            }
            for (size_t w = 0; w < W; w++) G.accData[o * W + w] = word(w, g);
            o++;
        }
    });
}

// rows: n candidate rows of `stride` words, [first row | group id | accumulator blocks]
inline void groupsFromDenseRows(const std::vector<DenseKey>& keys, const std::vector<int>& accumSlot, const int64_t* rows, size_t n, size_t stride, Groups& G) {
    const size_t W = accumSlot.size();
    G.n = n; G.nKeys = keys.size(); G.nAcc = W;
    G.firstRow.resize(G.n); G.keyData.resize(G.n * G.nKeys); G.accData.resize(G.n * W);
    const size_t strBytes = codedKeyBytes(keys);
    G.strings.assign(G.n * strBytes, 0);
    for (size_t i = 0; i < G.n; i++) {
        const int64_t* r = &rows[i * stride];
        const int64_t g = r[1];
        G.firstRow[i] = r[0];
        size_t k = 0, sp = i * strBytes;
        for (auto& dk : keys) {
            const int64_t rank = (g / dk.stride) % dk.card;
            G.keyData[i * G.nKeys + k++] = denseKeyValue(dk, rank, G.strings.data(), sp);
        }
        for (size_t w = 0; w < W; w++) G.accData[i * W + w] = r[2 + (size_t)accumSlot[w]];
    }
}

}  // namespace rsq
