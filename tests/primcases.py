"""Inputs and exact references for tests/test_primitives_host.py and tests/test_gpu_primitives.py: the offset scan of a materialisation
(aot_kernels.hip k_scan_chunks / k_scan_chunk_totals / k_scan_add_base and the one-launch k_scan_chained), the rank index of a key bitmap
(k_rank_blocks / k_rank_absolute and the one-launch k_rank_blocks_chained) and the placement of build records at the rank of their keys
(k_rank_place<1..4>, k_rank_place<0>, k_rank_place_wide), called on the test's own data through rsq_prim_* (include/resql_hip.h).

The kernels are exact integer kernels, so the references are too: a numpy cumulative sum, a popcount per block and its cumulative sum, a
sort of the distinct keys.  The sizes put the kernels' own boundaries inside a run - the scalar tail of a four-count load, the four
sub-blocks of a chunk, the chunk, 64 and 128 predecessors of a wave's look-back, more than 1024 chunks for the carry of the
single-workgroup scan of the chunk totals; a bitmap block's first and last word and a word's first and last bit.  The host test holds
every vectorised reference against a plain loop before a kernel is involved."""
import numpy as np

# The kernels' geometry, in one place.  The host test reads the three definitions in the source and compares.
SCAN_CHUNK = 4096             # counts per workgroup of the scan:                            aot_kernels.hip  #define SCAN_CHUNK 4096
SCAN_BATCH = 1024             # counts per sub-block of a chunk (k_scan_chunks: sb * 1024), and chunk totals per batch of
#                               k_scan_chunk_totals (base += 1024):                          aot_kernels.hip, literals in both kernels
RANK_CHUNK_BLOCKS = 1024      # 32-byte bitmap blocks per workgroup of the rank index:       engine.h  #define RSQ_RANK_CHUNK_BLOCKS 1024
BLOCK_WORDS = 8               # a bitmap block: [rank word | 7 bitmap words]
BLOCK_BITS = 32 * (BLOCK_WORDS - 1)

# bits of the device error word the primitives may raise (include/resql_hip.h, "device primitives exposed for tests")
NOTE_PLACE_COUNT, NOTE_RANK_LOOKBACK, NOTE_SCAN_LOOKBACK = 64, 128, 512
NOTE_NAMES = {NOTE_PLACE_COUNT: "64: record count is not the number of distinct keys (or exceeds the capacity)",
              NOTE_RANK_LOOKBACK: "128: a look-back of the one-launch rank index timed out",
              NOTE_SCAN_LOOKBACK: "512: a look-back of the one-launch scan timed out"}


def notes_text(notes):
    """the bits of `notes` by name, for assertion messages"""
    return "; ".join(NOTE_NAMES.get(1 << b, f"{1 << b}: unknown") for b in range(32) if notes >> b & 1) or "none"


# ---- scan -------------------------------------------------------------------------------------------------------------------------
SCAN_SIZES = [1, 2, 3, 4, 5, 255, SCAN_BATCH - 1, SCAN_BATCH, SCAN_BATCH + 1, SCAN_BATCH + 3,
              SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 1, 2 * SCAN_CHUNK - 1, 2 * SCAN_CHUNK + 1,
              64 * SCAN_CHUNK - 1, 64 * SCAN_CHUNK, 64 * SCAN_CHUNK + 1, 65 * SCAN_CHUNK + 3, 129 * SCAN_CHUNK + 2,
              (SCAN_BATCH + 2) * SCAN_CHUNK + 5]       # the largest: 4.2 M counts, 17 MB in and 34 MB out; 1027 chunks
SCAN_PATTERNS = ["zeros", "ones", "random", "last_only", "first_only", "max32", "empty_chunks"]


def scan_counts(n, pattern, seed=0):
    """`n` uint32 counts.  max32: every count 0xffffffff - every carry (lane, wave, sub-block, chunk, chain) crosses 32 bits.
    empty_chunks: whole chunks of zeros between non-empty ones, the first chunk empty where there is more than one (chain words whose
    value is 0, own totals and inclusive ones)."""
    rng = np.random.default_rng(n * 7 + seed)
    if pattern == "zeros":
        return np.zeros(n, dtype=np.uint32)
    if pattern == "ones":
        return np.ones(n, dtype=np.uint32)
    if pattern == "random":
        return rng.integers(0, 128, n, dtype=np.uint32)
    if pattern in ("last_only", "first_only"):
        c = np.zeros(n, dtype=np.uint32)
        c[-1 if pattern == "last_only" else 0] = 77
        return c
    if pattern == "max32":
        return np.full(n, 0xffffffff, dtype=np.uint32)
    if pattern == "empty_chunks":
        c = rng.integers(0, 128, n, dtype=np.uint32)
        n_chunks = (n + SCAN_CHUNK - 1) // SCAN_CHUNK
        empty = rng.random(n_chunks) < 0.6
        empty[0] = n_chunks > 1
        c[np.repeat(empty, SCAN_CHUNK)[:n]] = 0
        return c
    raise AssertionError(pattern)


def scan_reference(counts):
    """offsets[i] = counts[0] + ... + counts[i - 1] in 64 bits"""
    out = np.zeros(len(counts), dtype=np.uint64)
    np.cumsum(counts[:-1], dtype=np.uint64, out=out[1:])
    return out


def scan_reference_loop(counts):
    out, run = [], 0
    for c in counts:
        out.append(run)
        run += int(c)
    return out


# ---- rank index ---------------------------------------------------------------------------------------------------------------------
RANK_BLOCKS = [1, 3, 4, 5, RANK_CHUNK_BLOCKS - 1, RANK_CHUNK_BLOCKS, RANK_CHUNK_BLOCKS + 1, 2 * RANK_CHUNK_BLOCKS + 1,
               64 * RANK_CHUNK_BLOCKS, 64 * RANK_CHUNK_BLOCKS + 1, 65 * RANK_CHUNK_BLOCKS + 7, 130 * RANK_CHUNK_BLOCKS + 3]
RANK_DENSITIES = ["empty", "full", "one_percent", "last_block_one_bit"]
_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint32)


def rank_blocks(n_blocks, density, seed=0):
    """a key bitmap [n_blocks, 8] of uint32: words 1..7 by `density`, word 0 junk (the index must ignore what it finds there)"""
    rng = np.random.default_rng(n_blocks * 13 + seed)
    b = np.zeros((n_blocks, BLOCK_WORDS), dtype=np.uint32)
    if density == "full":
        b[:, 1:] = 0xffffffff
    elif density == "one_percent":
        bits = rng.random((n_blocks, BLOCK_BITS)) < 0.01
        b[:, 1:] = np.packbits(bits, axis=1, bitorder="little").view(np.uint32).reshape(n_blocks, BLOCK_WORDS - 1)
    elif density == "last_block_one_bit":
        b[-1, 1 + int(rng.integers(0, BLOCK_WORDS - 1))] = np.uint32(1) << np.uint32(rng.integers(0, 32))
    elif density != "empty":
        raise AssertionError(density)
    b[:, 0] = rng.integers(0, 1 << 32, n_blocks, dtype=np.uint32)
    return b


def rank_reference(blocks):
    """(rank of every block: the bits set in words 1..7 of the blocks before it; chunk_base: the rank at every RANK_CHUNK_BLOCKS-th block,
    then the number of bits set)"""
    n = len(blocks)
    per_block = _POP8[np.ascontiguousarray(blocks[:, 1:]).view(np.uint8)].reshape(n, -1).sum(axis=1, dtype=np.uint64)
    incl = np.cumsum(per_block, dtype=np.uint64)
    rank = (incl - per_block).astype(np.uint32)
    chunk_base = np.append(rank[::RANK_CHUNK_BLOCKS], np.uint32(incl[-1] if n else 0)).astype(np.uint32)
    return rank, chunk_base


def rank_reference_loop(blocks):
    rank, chunk_base, run = [], [], 0
    for i, blk in enumerate(blocks):
        if i % RANK_CHUNK_BLOCKS == 0:
            chunk_base.append(run)
        rank.append(run)
        for w in range(1, BLOCK_WORDS):
            for bit in range(32):
                run += int(blk[w]) >> bit & 1
    return rank, chunk_base + [run]


# ---- placement ----------------------------------------------------------------------------------------------------------------------
PLACE_BITS = 3 * RANK_CHUNK_BLOCKS * BLOCK_BITS + 100        # three whole chunks of the index and a little of a fourth
PLACE_MIN = -(1 << 40) - 12345
PLACE_WORDS = [1, 2, 3, 4, 5, 8, 9, 12]                      # k_rank_place<1>..<4>, <0> with 5 and 8 words, k_rank_place_wide
PLACE_WAVES = [1, 3, 70]
PLACE_USED = [0, 1, 255, 256, 257, 511, 512, 513]            # around one and two passes of the two-records-per-thread loop of 256 threads
_CHUNK_BITS = RANK_CHUNK_BLOCKS * BLOCK_BITS
# key offsets every case holds (as many as it has records for): both ends of the domain, bits 0 and 31 of a word, words 1 and 7 of a
# block, the last key of each chunk of the index with the first of the next
PLACE_EDGES = [0, PLACE_BITS - 1, 31, 32, 63, BLOCK_BITS - 32, BLOCK_BITS - 1, BLOCK_BITS, _CHUNK_BITS - 1, _CHUNK_BITS, 2 * _CHUNK_BITS - 1,
               2 * _CHUNK_BITS, 3 * _CHUNK_BITS - 1, 3 * _CHUNK_BITS, 3 * _CHUNK_BITS + 31, 3 * _CHUNK_BITS + 32]


def bit_position(d):
    """(block, word, bit) of key offset d: bit d & 31 of word 1 + (d >> 5) % 7 of block (d >> 5) / 7 (kernels/rsq_device.h rank_of)"""
    return (d >> 5) // 7, 1 + (d >> 5) % 7, d & 31


def blocks_of_offsets(offsets, bm_bits=PLACE_BITS):
    """the key bitmap with the bit of every offset set; rank words 0 (the entry point indexes it)"""
    d = np.asarray(offsets, dtype=np.int64)
    b = np.zeros(((bm_bits + BLOCK_BITS - 1) // BLOCK_BITS, BLOCK_WORDS), dtype=np.uint32)
    blk, word, bit = bit_position(d)
    np.bitwise_or.at(b, (blk, word), np.uint32(1) << bit.astype(np.uint32))
    return b


def blocks_of_offsets_loop(offsets, bm_bits=PLACE_BITS):
    b = [[0] * BLOCK_WORDS for _ in range((bm_bits + BLOCK_BITS - 1) // BLOCK_BITS)]
    for d in offsets:
        blk, word, bit = bit_position(int(d))
        b[blk][word] |= 1 << bit
    return b


class PlaceCase:
    """records of `n_words` words in `n_waves` regions (used[w] of them in region w, the rest of a region junk the kernel must not read),
    their keys distinct offsets of the domain in random arrival order; `blocks` holds exactly their bits"""

    def __init__(self, n_words, n_waves, used_shift=0, seed=0):
        rng = np.random.default_rng(seed * 1000 + n_words * 100 + n_waves)
        self.n_words, self.n_waves = n_words, n_waves
        self.bm_min, self.bm_bits = PLACE_MIN, PLACE_BITS
        self.used = np.array([PLACE_USED[(w + used_shift) % len(PLACE_USED)] for w in range(n_waves)], dtype=np.uint32)
        self.region = max(64, (int(self.used.max()) + 63) // 64 * 64)
        n = int(self.used.sum())
        edges = PLACE_EDGES[:n]
        rest = np.setdiff1d(rng.permutation(self.bm_bits)[:n + len(edges)], edges)
        offsets = np.concatenate([np.array(edges, dtype=np.int64), rng.permutation(rest)[:n - len(edges)].astype(np.int64)])
        assert len(offsets) == n and len(np.unique(offsets)) == n
        self.rec = rng.integers(-(1 << 63), (1 << 63) - 1, (n, n_words), dtype=np.int64)      # word 0: the key, the others random
        self.rec[:, 0] = self.bm_min + rng.permutation(offsets)
        self.capacity = n + 7

    def offsets(self):
        return self.rec[:, 0] - self.bm_min

    def blocks(self):
        d = self.offsets()
        return blocks_of_offsets(np.unique(d[(d >= 0) & (d < self.bm_bits)]), self.bm_bits)

    def records(self):
        """the arrival-order buffer [n_waves, region, n_words]; a slot behind used[w] holds a key of the domain and random words: a
        kernel that read it would place it over a real entry (or, its key having no bit, at some entry's rank)"""
        buf = np.random.default_rng(int(self.used.sum()) + self.n_words).integers(-(1 << 62), 1 << 62, (self.n_waves, self.region, self.n_words), dtype=np.int64)
        buf[:, :, 0] = self.bm_min + buf[:, :, 0] % self.bm_bits
        at = 0
        for w, u in enumerate(self.used):
            buf[w, :u] = self.rec[at:at + u]
            at += int(u)
        return buf.reshape(-1)

    def expected(self):
        """words_out[rank(key)] = record, rank = the key's position among the sorted distinct keys of the domain; every other entry
        0xff bytes.  (Two records with one key: the later one here - callers compare that entry on their own.)"""
        d = self.offsets()
        ok = (d >= 0) & (d < self.bm_bits)
        keys = np.unique(self.rec[ok, 0])
        out = np.full((self.capacity, self.n_words), -1, dtype=np.int64)
        out[np.searchsorted(keys, self.rec[ok, 0])] = self.rec[ok]
        return out, len(keys)


def place_reference_loop(rec, n_words, bm_min, bm_bits, capacity):
    """the same by a plain loop over a Python set"""
    keys = sorted({int(r[0]) for r in rec if 0 <= int(r[0]) - bm_min < bm_bits})
    out = [[-1] * n_words for _ in range(capacity)]
    for r in rec:
        if 0 <= int(r[0]) - bm_min < bm_bits:
            out[keys.index(int(r[0]))] = [int(x) for x in r]
    return out, len(keys)


def place_cases():
    """(id, PlaceCase) over every record width and wave count; the used[] pattern starts at another value for every width, so that each
    of PLACE_USED is also the only region of a one-wave case once"""
    out = []
    for i, n_words in enumerate(PLACE_WORDS):
        for n_waves in PLACE_WAVES:
            out.append((f"words{n_words}_waves{n_waves}", PlaceCase(n_words, n_waves, used_shift=i)))
    return out
