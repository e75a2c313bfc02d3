// The packing rule of the register aggregation's second form (resql_amd/csrc/row_cells.h) on the host: fields of a word are disjoint, the
// largest sum the bound allows fits its field with every neighbour at its own largest, and one row more is refused.
#include "row_cells.h"
#include <cstdio>
#include <cstdlib>
#include <random>

using namespace rsq::rowcells;

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

// the rows the kernel's loops really give the busiest lane word, counted (the bound must cover it)
static uint64_t countedRows(uint64_t nRows, uint64_t grid, uint64_t block) {
    const uint64_t wavesPerGroup = block / 64, nwaves = grid * wavesPerGroup, tiles = nRows >> 7;
    uint64_t most = 0;
    for (uint64_t wg = 0; wg < grid; wg++) {
        for (uint64_t lane = 0; lane < 64; lane++) {
            uint64_t rows = 0;
            for (uint64_t w = 0; w < wavesPerGroup; w++) {
                const uint64_t wave = wg * wavesPerGroup + w;
                if (wave < tiles) rows += 2 * ((tiles - wave + nwaves - 1) / nwaves);
                for (uint64_t r = (tiles << 7) + wg * block + w * 64 + lane; r < nRows; r += grid * block) rows++;
            }
            if (rows > most) most = rows;
        }
    }
    return most;
}

int main() {
    std::mt19937_64 rng(20240607);
    // ---- which accumulators pack, and where -------------------------------------------------------------------------------------------
    for (int round = 0; round < 2000; round++) {
        std::vector<Accumulator> accs(1 + rng() % 12);
        for (auto& a : accs) { a.partialSum = rng() % 4 != 0; a.negative = rng() % 5 == 0; a.envelopeBits = (int)(rng() % 26) - 1; }
        const std::vector<Field> f = assignFields(accs);
        CHECK(f.size() == accs.size());
        for (size_t w = 0; w < accs.size(); w++) {
            if (f[w].host < 0) continue;
            CHECK(packs(accs[w]) && packs(accs[(size_t)f[w].host]) && f[w].host <= (int)w && f[(size_t)f[w].host].host == f[w].host);
            CHECK(f[w].shift % kFieldBits == 0 && f[w].shift + kFieldBits <= 64 && (f[w].host != (int)w || f[w].shift == 0));
            int members = 0;
            for (size_t v = 0; v < accs.size(); v++) {
                if (f[v].host != f[w].host) continue;
                members++;
                CHECK(v == w || f[v].shift != f[w].shift);              // disjoint fields
            }
            CHECK(members >= 2 && members <= kFieldsPerWord);
        }
        int packing = 0, packed = 0;
        for (size_t w = 0; w < accs.size(); w++) { packing += packs(accs[w]); packed += f[w].host >= 0; }
        CHECK(packed == packing || packed == packing - 1);              // at most one left over: a word of a single member is no packing
    }
    // TPC-H Q1: first row, sum(quantity) 6 bits, sum(extendedprice) 24 bits, two wide sums, the count, sum(discount) 4 bits
    {
        const std::vector<Field> f = assignFields({{false, false, -1}, {true, false, 6}, {true, false, 24}, {false, false, -1}, {false, false, -1}, {true, false, 1}, {true, false, 4}});
        CHECK(f[1].host == 1 && f[1].shift == 0 && f[5].host == 1 && f[5].shift == 21 && f[6].host == 1 && f[6].shift == 42);
        CHECK(f[0].host < 0 && f[2].host < 0 && f[3].host < 0 && f[4].host < 0);
    }
    // ---- the bound on the rows of a lane word covers what the loops deal out ----------------------------------------------------------------
    for (int round = 0; round < 300; round++) {
        const uint64_t block = 64ull << (rng() % 4), grid = 1 + rng() % 12, nRows = rng() % 40000;
        const uint64_t bound = maxRowsPerLaneWord(nRows, grid, block), counted = countedRows(nRows, grid, block);
        CHECK(counted <= bound);
        CHECK(bound <= counted + 3 * (block / 64));                     // ... and is not far off: a rounded-up tile and a tail row per wave
    }
    CHECK(maxRowsPerLaneWord(1000, 0, 512) == ~0ull);
    // ---- the largest sums the bound allows fit their fields; one row more is refused ------------------------------------------------------
    for (int round = 0; round < 5000; round++) {
        int env[3];
        for (int& e : env) e = 1 + (int)(rng() % kMaxEnvelopeBits);
        uint64_t rows = ~0ull;          // the most rows all three fields take
        for (int e : env) { const uint64_t top = (1ull << e) - 1ull, r = ((1ull << kFieldBits) - 1ull) / top; rows = r < rows ? r : rows; }
        for (int e : env) CHECK(fieldFits(rows, e));
        bool refused = false;
        for (int e : env) refused = refused || !fieldFits(rows + 1, e);
        CHECK(refused);
        // every row at the top of every envelope: the word's fields hold exactly their sums
        uint64_t word = 0;
        for (int j = 0; j < 3; j++) word += (rows * ((1ull << env[j]) - 1ull)) << (j * kFieldBits);
        for (int j = 0; j < 3; j++) CHECK(((word >> (j * kFieldBits)) & kFieldMask) == rows * ((1ull << env[j]) - 1ull));
    }
    CHECK(!fieldFits(1, kMaxEnvelopeBits + 1) && !fieldFits(1, -1) && fieldFits(0, 8) && !fieldFits(~0ull, 1));
    // a launch: 8-bit inputs at 255 in one workgroup of 512 threads
    {
        const std::vector<int> env = {8, 1, 4};
        // 8 waves x 2 rows x tiles-per-wave x 255 < 2^21  <=>  tiles per wave <= 514: 8 x 514 tiles of 128 rows fit, one tile more does not
        const uint64_t fits = 8ull * 514 * 128, past = fits + 128;
        CHECK(launchFits(env, fits, 1, 512) && !launchFits(env, past, 1, 512));
        CHECK(launchFits(env, 59986052, 512, 512));                      // TPC-H lineitem at SF10 on its full grid
        CHECK(!launchFits(env, 59986052, 1, 512));
        CHECK(launchFits({}, ~0ull >> 1, 1, 512));                       // nothing packed: nothing to carry
    }
    printf("row_cells_test ok\n");
    return 0;
}
