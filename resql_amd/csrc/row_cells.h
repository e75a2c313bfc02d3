// row_cells.h - the second form of the register aggregation (codegen_agg.cpp, RSQ_ROW_CELLS 1): every row adds its inputs straight into its
// lane's words of the workgroup's LDS image, one LDS atomic per word.  Plain C++, shared by the code generator (which accumulators share a
// word), the engine (whether a launch may run the form) and tests/cpp/row_cells_test.cpp.
//
// Packing.  A sum that takes 32-bit partial sums in form 0 and whose input is never negative and at most kMaxEnvelopeBits wide shares a u64
// word with up to two others, in fixed fields of kFieldBits bits: the row adds in_a | in_b << 21 | in_c << 42 once.  The word is the cell
// of the FIRST accumulator of the three; the epilogue takes the fields apart per lane, before the wave reduction (a sum over 64 lanes
// could carry into the next field).  A field never carries while the rows one lane's word receives, times the largest input, stay below
// 2^21: maxRowsPerLaneWord() is the bound on those rows for a launch, fieldFits() the test, launchFits() both over all fields.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace rsq {
namespace rowcells {

constexpr int kFieldBits = 21, kFieldsPerWord = 3, kMaxEnvelopeBits = 8;
constexpr uint64_t kFieldMask = (1ull << kFieldBits) - 1ull;

struct Accumulator {
    bool partialSum;      // a sum that takes 32-bit partial sums in form 0
    bool negative;        // its input's envelope reaches below zero
    int envelopeBits;     // width of max |input| (a count: 1)
};
struct Field {
    int host = -1;        // the accumulator whose cell holds the word; -1: not packed (a word of its own)
    int shift = 0;        // first bit of the field
};

inline bool packs(const Accumulator& a) { return a.partialSum && !a.negative && a.envelopeBits >= 0 && a.envelopeBits <= kMaxEnvelopeBits; }

// fields in accumulator order, three to a word; a word with a single member is no packing at all
inline std::vector<Field> assignFields(const std::vector<Accumulator>& accs) {
    std::vector<Field> f(accs.size());
    std::vector<int> members;
    auto close = [&]() {
        if (members.size() >= 2)
            for (size_t j = 0; j < members.size(); j++) { f[(size_t)members[j]].host = members[0]; f[(size_t)members[j]].shift = (int)j * kFieldBits; }
        members.clear();
    };
    for (size_t w = 0; w < accs.size(); w++) {
        if (!packs(accs[w])) continue;
        members.push_back((int)w);
        if ((int)members.size() == kFieldsPerWord) close();
    }
    close();
    return f;
}

// The rows one lane's word can receive in a launch of `grid` workgroups of `blockThreads` threads over nRows rows: tiles of 128 rows are
// dealt to the waves round-robin, two rows a lane; the rows behind the last whole tile go one to a thread, round-robin over the grid; all
// waves of a workgroup add into the same 64 words of a cell.
inline uint64_t maxRowsPerLaneWord(uint64_t nRows, uint64_t grid, uint64_t blockThreads) {
    if (grid == 0 || blockThreads < 64) return ~0ull;
    const uint64_t wavesPerGroup = blockThreads / 64, nwaves = grid * wavesPerGroup, threads = grid * blockThreads;
    const uint64_t tiles = nRows >> 7, tailRows = nRows & 127;
    const uint64_t tilesPerWave = (tiles + nwaves - 1) / nwaves, tailPerThread = (tailRows + threads - 1) / threads;
    return wavesPerGroup * (tilesPerWave * 2 + tailPerThread);
}
inline bool fieldFits(uint64_t rows, int envelopeBits) {
    if (envelopeBits < 0 || envelopeBits > kMaxEnvelopeBits) return false;
    const uint64_t top = (1ull << envelopeBits) - 1ull;
    return rows <= (~0ull >> 8) && rows * top < (1ull << kFieldBits);
}
// every packed field of a statement (their envelope widths) under one launch
inline bool launchFits(const std::vector<int>& packedEnvelopeBits, uint64_t nRows, uint64_t grid, uint64_t blockThreads) {
    const uint64_t rows = maxRowsPerLaneWord(nRows, grid, blockThreads);
    for (int b : packedEnvelopeBits) if (!fieldFits(rows, b)) return false;
    return true;
}

}  // namespace rowcells
}  // namespace rsq
