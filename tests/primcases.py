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

# The kernels' geometry, in one place.  The host test reads the definitions in the source and compares.
SCAN_CHUNK = 4096             # counts per workgroup of the scan:                            scan_device.h  #define SCAN_CHUNK 4096
SCAN_BATCH = 1024             # counts per sub-block of a chunk (k_scan_chunks), and values per batch of the single-workgroup scans
#                               (batched_exclusive_scan: k_scan_chunk_totals, k_scanmin_totals):  scan_device.h  #define SCAN_BATCH 1024
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


# =====================================================================================================================================
# The kernels that finish an aggregation: the radix sort of the device tail, the running minimum of the replay, the merge of several
# shards' group rows (devtail.hip) and the ORDER BY ... LIMIT pre-selection (aot_kernels.hip), through rsq_prim_radix_sort_pairs,
# rsq_prim_running_min, rsq_prim_merge_group_rows and rsq_prim_topk_select.  Integer operations all four: every reference is exact.
# =====================================================================================================================================
RS_TILE = 2048                # pairs per workgroup of a sort pass, taken in rounds of 256:   devtail.hip  #define RS_TILE 2048
SM_CHUNK = 4096               # values per workgroup of the running minimum:                  scan_device.h  #define SM_CHUNK 4096
SM_PER_THREAD = 16            # ... consecutive ones per thread:                              scan_device.h  #define SM_PER_THREAD 16
SM_BATCH = SCAN_BATCH         # chunk minima per batch of k_scanmin_totals: the one batch size of batched_exclusive_scan (scan_device.h)
TOPK_BINS = 2048              # bins of one histogram (an 11-bit digit):                      aot_kernels.hip  enum { TOPK_PASSES = 6, TOPK_BINS = 2048 }
TOPK_PASSES = 6               # five 11-bit digits and a last one of 9 bits (topk_shift / topk_bits)
NOTE_MERGE_FULL = 2           # k_gm_insert: "Hash table full" (a table of >= 2 n slots: not reached)
NOTE_NAMES[NOTE_MERGE_FULL] = "2: the merge's hash table is full"
NOTE_NAMES[256] = "256: a meeting point of the one-launch top-k selection timed out"
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
U64 = (1 << 64) - 1
# rsq_type_tag (include/resql_plan.h)
T_VARCHAR, T_CHAR, T_BOOL, T_INT, T_BIGINT, T_DECIMAL, T_DATE = 0, 1, 2, 3, 4, 5, 7


# ---- sort ---------------------------------------------------------------------------------------------------------------------------
SORT_SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, RS_TILE - 1, RS_TILE, RS_TILE + 1, 2 * RS_TILE - 1, 2 * RS_TILE + 1, 3 * RS_TILE + 1, 600_001]
SORT_KEY_BITS = [1, 8, 9, 16, 17, 24, 32, 33, 41, 63, 64]          # 1, 1, 2, 2, 3, 3, 4, 5, 6, 8, 8 passes
SORT_PATTERNS = ["equal", "digits_0_255", "lane_digits", "ascending", "descending", "copies50", "top_byte", "above_mask"]


def sort_passes(key_bits):
    return (key_bits + 7) // 8


def sort_mask(key_bits):
    """the bits radixSortPairs sorts by: whole 8-bit digits, 8 * ceil(key_bits / 8) of them"""
    return (1 << 8 * sort_passes(key_bits)) - 1


def sort_keys(n, key_bits, pattern, seed=0):
    """`n` uint64 keys.  equal: a tile's 2048 pairs share every digit.  digits_0_255: every digit is the first or the last bin.
    lane_digits: digit d of key i is i % 256 in every pass - the 256 lanes of a round hold 256 different digits.  copies50: about 50
    copies of every key (stability decides their order).  top_byte: only the last pass sees a difference.  above_mask: copies50 with
    random bits above the sorted ones, which must travel with the key and not matter."""
    rng = np.random.default_rng(n * 11 + key_bits * 1000 + seed)
    passes, mask = sort_passes(key_bits), np.uint64(sort_mask(key_bits))
    i = np.arange(n, dtype=np.uint64)
    if pattern == "equal":
        return np.full(n, 0x5a5a5a5a5a5a5a5a, dtype=np.uint64) & mask
    if pattern == "digits_0_255":
        k = np.zeros(n, dtype=np.uint64)
        for d in range(passes):
            k |= rng.integers(0, 2, n, dtype=np.uint64) * np.uint64(255) << np.uint64(8 * d)
        return k
    if pattern == "lane_digits":
        return (i % np.uint64(256)) * np.uint64(0x0101010101010101) & mask
    if pattern in ("ascending", "descending"):
        up = i * np.uint64(int(mask) // max(n, 1)) if n <= int(mask) else i * (mask + np.uint64(1)) // np.uint64(max(n, 1))      # sorted, over the whole range
        return up if pattern == "ascending" else up[::-1].copy()
    distinct = rng.integers(0, 1 << 63, n // 50 + 1, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n // 50 + 1, dtype=np.uint64) & mask
    k = distinct[rng.integers(0, len(distinct), n)]
    if pattern == "copies50":
        return k
    if pattern == "top_byte":
        return (k & np.uint64(0xff)) << np.uint64(8 * (passes - 1)) | np.uint64(0x0123456789abcdef) & (mask >> np.uint64(8))
    if pattern == "above_mask":
        above = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64) & ~mask
        return k | above
    raise AssertionError(pattern)


def sort_vals(n, kind, seed=0):
    """arange: the input position, which makes stability visible; random: any 32 bits, 0xffffffff among them"""
    if kind == "arange":
        return np.arange(n, dtype=np.uint32)
    v = np.random.default_rng(n + seed).integers(0, 1 << 32, n, dtype=np.uint32)
    v[::7] = 0xffffffff
    return v


def sort_reference(keys, vals, key_bits):
    order = np.argsort(keys & np.uint64(sort_mask(key_bits)), kind="stable")
    return keys[order], vals[order]


def sort_reference_loop(keys, vals, key_bits):
    mask = sort_mask(key_bits)
    order = sorted(range(len(keys)), key=lambda i: (int(keys[i]) & mask, i))
    return [int(keys[i]) for i in order], [int(vals[i]) for i in order]


def sort_cases():
    """(n, key_bits, pattern, vals kind).  Every key_bits with 2049 (every pattern) and 600 001 (copies50 and one more pattern, all of
    them over the list); every other size with an odd and an even number of passes - the result in either buffer pair - and every
    pattern; three cases whose values are not the input positions."""
    out = []
    odd = [b for b in SORT_KEY_BITS if sort_passes(b) % 2 == 1]
    even = [b for b in SORT_KEY_BITS if sort_passes(b) % 2 == 0]
    for j, n in enumerate(SORT_SIZES):
        for b in SORT_KEY_BITS if n == RS_TILE + 1 else (odd[j % len(odd)], even[j % len(even)]) if n != 600_001 else ():
            out += [(n, b, p, "arange") for p in SORT_PATTERNS]
    for j, b in enumerate(SORT_KEY_BITS):
        out += [(600_001, b, p, "arange") for p in sorted({"copies50", SORT_PATTERNS[j % len(SORT_PATTERNS)]})]
    out += [(257, 17, "copies50", "random"), (RS_TILE + 1, 16, "copies50", "random"), (3 * RS_TILE + 1, 41, "digits_0_255", "random")]
    return out


# ---- running minimum ------------------------------------------------------------------------------------------------------------------
RUNMIN_SIZES = [1, 15, 16, 17, 1023, 1024, 1025, SM_CHUNK - 1, SM_CHUNK, SM_CHUNK + 1, 2 * SM_CHUNK + 1,
                SM_BATCH * SM_CHUNK - 1, SM_BATCH * SM_CHUNK, SM_BATCH * SM_CHUNK + 1, (SM_BATCH + 1) * SM_CHUNK + 17]      # the last four: a second
#                 batch of k_scanmin_totals, 34 MB each way
RUNMIN_PATTERNS = ["increasing", "decreasing", "random", "holds_max"]
# (n, index of the one INT64_MIN among INT64_MAX): both sides of a thread's 16 values, of a wave's 1024, of a chunk, of the first batch
# of chunk minima, and the very last value
RUNMIN_SINGLE = [(2 * SM_CHUNK + 1, at) for at in (0, 15, 16, 1023, 1024, SM_CHUNK - 1, SM_CHUNK, 2 * SM_CHUNK)] + \
                [((SM_BATCH + 1) * SM_CHUNK + 17, at) for at in (SM_CHUNK - 1, SM_CHUNK, (SM_BATCH - 1) * SM_CHUNK + SM_CHUNK - 1, SM_BATCH * SM_CHUNK,
                                                                 (SM_BATCH + 1) * SM_CHUNK + 16)]


def runmin_values(n, pattern, seed=0, at=None):
    """`n` int64 values.  increasing: the first value is the minimum of every prefix - it must cross every boundary.  decreasing: every
    value is a new minimum.  holds_max: INT64_MAX - the kernels' padding value - as data, a few other values in between.  single: one
    INT64_MIN at `at`, INT64_MAX everywhere else."""
    rng = np.random.default_rng(n * 3 + seed)
    i = np.arange(n, dtype=np.int64)
    if pattern == "increasing":
        return i - 5
    if pattern == "decreasing":
        return (1 << 62) - 3 * i
    if pattern == "random":
        return rng.integers(INT64_MIN, INT64_MAX, n, dtype=np.int64, endpoint=True)
    v = np.full(n, INT64_MAX, dtype=np.int64)
    if pattern == "holds_max":
        where = rng.random(n) < 0.002
        where[0] = False
        v[where] = rng.integers(INT64_MIN, INT64_MAX, int(where.sum()), dtype=np.int64, endpoint=True)
        return v
    if pattern == "single":
        v[at] = INT64_MIN
        return v
    raise AssertionError(pattern)


def runmin_reference(v):
    return np.minimum.accumulate(v)


def runmin_reference_loop(v):
    out, m = [], None
    for x in v:
        m = int(x) if m is None or int(x) < m else m
        out.append(m)
    return out


def runmin_cases():
    return [(n, p, None) for n in RUNMIN_SIZES for p in RUNMIN_PATTERNS] + [(n, "single", at) for n, at in RUNMIN_SINGLE]


# ---- merge of group rows ----------------------------------------------------------------------------------------------------------------
MERGE_SIZES = [1, 2, 255, 256, 257, 100_003]
MERGE_GROUPINGS = ["one", "distinct", "three", "random"]
MERGE_KEYSETS = ["bigint", "int_date", "bool_char1", "char12", "varchar12", "char11_varchar20", "composite"]
MERGE_ACCSETS = ["small", "wrap", "extremes"]
_MERGE_KEYS = {      # (type tag, len) of every key; a string takes ceil(len / 8) table words
    "bigint": [(T_BIGINT, 0)], "int_date": [(T_INT, 0), (T_DATE, 0)], "bool_char1": [(T_BOOL, 0), (T_CHAR, 1)], "char12": [(T_CHAR, 12)],
    "varchar12": [(T_VARCHAR, 12)], "char11_varchar20": [(T_CHAR, 11), (T_VARCHAR, 20)], "composite": [(T_BIGINT, 0), (T_INT, 0), (T_CHAR, 11)]}
_MERGE_ACCS = {"small": [0], "wrap": [0, 0, 2, 3], "extremes": [2, 3, 0]}      # merge kinds: 0 wrapping sum, 2 min, 3 max


def _key_words(length):
    return (length + 7) // 8 if length > 1 else 1


def _string_words(rng, g, length, is_char):
    """[n, words] int64 holding one spelling per row of group g's string: the group's text, then - row by row - some trailing spaces, a
    NUL and random bytes behind it (equal for CHAR, different strings for VARCHAR unless the spaces agree), or the text padded with
    spaces to the full length (CHAR only); every fourth group's text fills the whole length (not group 0: "one group" keeps its spellings).  The bytes behind `length` in the last
    word are random in every row."""
    n, words = len(g), _key_words(length)
    b = rng.integers(0, 256, (n, words * 8), dtype=np.uint8)
    spaces = rng.integers(0, length + 1, n)
    for r in range(n):
        text = b"k%d" % g[r]
        if g[r] % 4 == 3:
            text = (text + b"x" * length)[:length]
        end = min(length, len(text) + int(spaces[r]))
        b[r, :len(text)] = np.frombuffer(text, dtype=np.uint8)
        b[r, len(text):end] = 32
        if end < length and not (is_char and spaces[r] % 3 == 0):
            b[r, end] = 0
        elif end < length:
            b[r, end:length] = 32
    return b.view(np.int64).reshape(n, words)


class MergeCase:
    """group rows [first row | table words | accumulators] of `n` rows "of several shards, back to back".  grouping: one - all rows one
    group; distinct - as many groups as the key set has values for; three - every group has exactly three members, one in each third
    of the rows, the smallest first row in the first, second, third member in turn; random - about four members per group."""

    def __init__(self, n, grouping, keyset, accset, seed=0):
        rng = np.random.default_rng(n * 17 + MERGE_GROUPINGS.index(grouping) * 5 + MERGE_KEYSETS.index(keyset) + seed * 1000)
        self.n, self.grouping, self.keyset, self.accset = n, grouping, keyset, accset
        third = n // 3
        if grouping == "one":
            g = np.zeros(n, dtype=np.int64)
        elif grouping == "distinct" or (grouping == "three" and third == 0):
            g = rng.permutation(n).astype(np.int64)
        elif grouping == "three":      # (the n % 3 rows behind the three shards are groups of their own)
            g = np.concatenate([rng.permutation(third), rng.permutation(third), rng.permutation(third), third + np.arange(n - 3 * third)]).astype(np.int64)
        else:
            g = rng.integers(0, n // 4 + 1, n).astype(np.int64)
        first = rng.permutation(n).astype(np.int64) * 3 + 1          # unique
        if grouping == "three" and third:      # member (g % 3) of group g gets the smallest of the group's three first rows
            shard = np.minimum(np.arange(n) // third, 3)
            members = np.argsort(g[:3 * third], kind="stable").reshape(third, 3)          # row indices of a group's members, shard by shard
            f = np.sort(first[members], axis=1)
            for grp in range(third):
                order = [1, 2, 2]
                order.insert(grp % 3, 0)
                first[members[grp]] = f[grp][order[:3]]
            assert (shard[members] == [0, 1, 2]).all()
        cols, self.keys, word = [first.reshape(n, 1)], [], 1
        for tag, length in _MERGE_KEYS[keyset]:
            self.keys.append((word, tag, length))
            junk = rng.integers(INT64_MIN, INT64_MAX, n, dtype=np.int64)
            if length > 1:
                cols.append(_string_words(rng, g, length, tag == T_CHAR))
            elif tag == T_BIGINT:
                cols.append(((g + 1) * np.int64(0x9E3779B97F4A7C15 - (1 << 64))).reshape(n, 1))          # (wraps; odd multiplier: injective)
            elif tag in (T_INT, T_DATE):      # the low 32 bits are the key, the upper 32 random
                low = (g * 40503 + (0 if tag == T_INT else g // 7)) & 0xffffffff
                cols.append(((junk & ~np.int64(0xffffffff)) | low).reshape(n, 1))
            else:                             # BOOL / CHAR(1): the low byte is the key, the upper seven random
                low = (g & 1) if tag == T_BOOL else 33 + (g >> 1) % 90
                cols.append(((junk & ~np.int64(0xff)) | low).reshape(n, 1))
            word += _key_words(length)
        self.n_tab = word - 1
        self.accs = []
        for kind in _MERGE_ACCS[accset]:
            self.accs.append((word, kind))
            if accset == "small":
                a = rng.integers(-1000, 1000, n, dtype=np.int64)
            elif accset == "wrap":            # two members are enough to pass INT64_MAX (or INT64_MIN)
                a = rng.choice(np.array([INT64_MAX, INT64_MAX // 2 + 1, INT64_MIN, INT64_MIN // 2 - 1, 1, -1], dtype=np.int64), n)
            else:
                a = rng.integers(INT64_MIN, INT64_MAX, n, dtype=np.int64, endpoint=True)
                a[rng.random(n) < 0.2] = INT64_MIN
                a[rng.random(n) < 0.2] = INT64_MAX
            cols.append(a.reshape(n, 1))
            word += 1
        self.stride = word
        self.rows = np.ascontiguousarray(np.concatenate(cols, axis=1), dtype=np.int64)
        assert self.rows.shape == (n, 1 + self.n_tab + len(self.accs))


def _merge_normalised(rows, keys):
    """[n, bytes] uint8: the key of every row as mergeGroupRows compares it - INT / DATE 4 bytes, BOOL / CHAR(1) one, other numbers 8; a
    string cut at its NUL, CHAR(n) without trailing spaces, as (length, bytes zeroed behind the length)"""
    n, parts = len(rows), []
    for word, tag, length in keys:
        if length > 1:
            b = np.ascontiguousarray(rows[:, word:word + _key_words(length)]).view(np.uint8).reshape(n, -1)[:, :length]
            nul = b == 0
            ln = np.where(nul.any(axis=1), nul.argmax(axis=1), length)
            if tag == T_CHAR:
                inside = np.arange(length)[None, :] < ln[:, None]
                keep = inside & (b != 32)
                ln = np.where(keep.any(axis=1), length - keep[:, ::-1].argmax(axis=1), 0)
            parts.append(np.where(np.arange(length)[None, :] < ln[:, None], b, 0).astype(np.uint8))
            parts.append(ln.astype(np.uint8).reshape(n, 1))
        else:
            width = 4 if tag in (T_INT, T_DATE) else 1 if tag in (T_BOOL, T_CHAR) else 8
            parts.append(np.ascontiguousarray(rows[:, word:word + 1]).view(np.uint8).reshape(n, 8)[:, :width])
    return np.ascontiguousarray(np.concatenate(parts, axis=1)) if parts else np.zeros((n, 1), dtype=np.uint8)


def merge_reference(rows, n_tab, keys, accs):
    """one row per group - [min of the first rows | table words of the member with that first row | accumulators merged] - sorted by
    word 0"""
    n, stride = rows.shape
    if n == 0:
        return rows.copy()
    norm = _merge_normalised(rows, keys)
    _, inv = np.unique(norm.view(np.dtype((np.void, norm.shape[1]))).reshape(n), return_inverse=True)
    inv = inv.reshape(n)
    groups = int(inv.max()) + 1
    first = np.full(groups, INT64_MAX, dtype=np.int64)
    np.minimum.at(first, inv, rows[:, 0])
    best = np.flatnonzero(rows[:, 0] == first[inv])
    assert len(best) == groups, "first rows must be unique"
    out = np.zeros((groups, stride), dtype=np.int64)
    out[inv[best], :1 + n_tab] = rows[best, :1 + n_tab]
    for word, kind in accs:
        if kind == 0:
            acc = np.zeros(groups, dtype=np.uint64)
            np.add.at(acc, inv, rows[:, word].view(np.uint64))          # (uint64: wraps like the engine's int64 sum)
            out[:, word] = acc.view(np.int64)
        else:
            acc = np.full(groups, INT64_MAX if kind == 2 else INT64_MIN, dtype=np.int64)
            (np.minimum if kind == 2 else np.maximum).at(acc, inv, rows[:, word])
            out[:, word] = acc
    return out[np.argsort(out[:, 0], kind="stable")]


def merge_reference_loop(rows, n_tab, keys, accs):
    """the same row by row: a dict from the normalised key tuple to [min first row, table words of that member, accumulators]"""
    def signed(x):
        x &= U64
        return x - (1 << 64) if x >> 63 else x
    table = {}
    for r in rows:
        r = [int(x) for x in r]
        key = []
        for word, tag, length in keys:
            if length > 1:
                raw = b"".join((r[word + w] & U64).to_bytes(8, "little") for w in range(_key_words(length)))[:length]
                s = raw.split(b"\0")[0]
                key.append(s.rstrip(b" ") if tag == T_CHAR else s)
            else:
                key.append(r[word] & (0xffffffff if tag in (T_INT, T_DATE) else 0xff if tag in (T_BOOL, T_CHAR) else U64))
        key = tuple(key)
        if key not in table:
            table[key] = list(r)
            continue
        g = table[key]
        if r[0] < g[0]:
            g[:1 + n_tab] = r[:1 + n_tab]
        for word, kind in accs:
            g[word] = signed(g[word] + r[word]) if kind == 0 else min(g[word], r[word]) if kind == 2 else max(g[word], r[word])
    return sorted(table.values())


def merge_cases():
    """(n, grouping, key set, accumulator set): every small size with every grouping and key set; 100 003 rows with every grouping of
    BIGINT keys and with three shards of every other key set.  The accumulator sets take turns."""
    out = []
    for n in MERGE_SIZES:
        for grouping in MERGE_GROUPINGS:
            for keyset in MERGE_KEYSETS:
                if n == 100_003 and keyset != "bigint" and grouping != "three":
                    continue
                out.append((n, grouping, keyset, MERGE_ACCSETS[len(out) % len(MERGE_ACCSETS)]))
    return out


# ---- ORDER BY ... LIMIT pre-selection -----------------------------------------------------------------------------------------------------
TOPK_SIZES = [1, 255, 256, 257, 2047, 2049, 600_001]          # 600 001: more than one sweep of a 256-workgroup grid (65 536 rows)
TOPK_KINDS = ["random64", "random32", "equal", "minmax", "low9", "top11", "ties"]
TOPK_ID_STEP, TOPK_ID_BASE = 7, 13                            # row i carries the id 13 + 7 i in the word behind its key


def topk_image(words, is32, desc):
    """aot_kernels.hip topk_image: the key (is32: its low 32 bits, sign-extended) with the sign bit flipped, complemented for ascending
    order - "earlier in the requested order" is "larger" """
    v = np.asarray(words, dtype=np.int64)
    if is32:
        v = v.astype(np.int32).astype(np.int64)
    u = v.view(np.uint64) ^ np.uint64(1 << 63)
    return u if desc else ~u


def topk_image_loop(w, is32, desc):
    w = int(w)
    if is32:
        w &= 0xffffffff
        w -= (w >> 31) << 32
    u = (w & U64) ^ (1 << 63)
    return u if desc else u ^ U64


def topk_range_shift(hi, lo):
    """k_topk_range_hist: hi > lo ? clz(hi - lo) : 0"""
    return 64 - (int(hi) - int(lo)).bit_length() if int(hi) > int(lo) else 0


def topk_range_digit(u, lo, shift):
    """aot_kernels.hip topk_range_digit: ((u - lo) << shift) >> 53 in 64 bits - below 2048 whatever the range"""
    with np.errstate(over="ignore"):
        return ((np.asarray(u, dtype=np.uint64) - np.uint64(lo)) << np.uint64(shift)) >> np.uint64(53)


def topk_range_digit_loop(u, lo, shift):
    return ((((int(u) - int(lo)) & U64) << shift) & U64) >> 53


def topk_exact_range(images):
    """(largest image, ~smallest image): what compactEntries collects into the scratch"""
    return (int(images.max()), int(images.min()) ^ U64) if len(images) else (0, 0)


def topk_wider_range(rng2):
    """a range that reaches half way to both ends of the 64 bits beyond the data's"""
    hi, lo = rng2[0], rng2[1] ^ U64
    return hi + (U64 - hi) // 2, (lo - lo // 2) ^ U64


def topk_reference(images, want):
    """form 0: the indices of the rows whose image is at or above the want-th largest - every row when there are fewer than `want`"""
    if want > len(images):
        return np.arange(len(images))
    t = np.partition(images, len(images) - want)[len(images) - want]
    return np.flatnonzero(images >= t)


def topk_reference_loop(images, want):
    s = sorted((int(x) for x in images), reverse=True)
    return [i for i, x in enumerate(images) if want > len(s) or int(x) >= s[want - 1]]


def topk_range_reference(images, want, rng2):
    """form 1: the rows in the bin of the want-th largest image and in every bin above it (bins of topk_range_digit over the range given,
    rng2 = (hi, ~lo)); every row when there are fewer than `want`"""
    hi, lo = rng2[0], rng2[1] ^ U64
    d = topk_range_digit(images, lo, topk_range_shift(hi, lo))
    at_or_above = np.cumsum(np.bincount(d.astype(np.int64), minlength=TOPK_BINS)[::-1])[::-1]          # rows in bins >= b
    ok = np.flatnonzero(at_or_above >= want)
    return np.flatnonzero(d >= (ok[-1] if len(ok) else 0))


def topk_range_reference_loop(images, want, rng2):
    hi, lo = rng2[0], rng2[1] ^ U64
    shift = topk_range_shift(hi, lo)
    d = [topk_range_digit_loop(u, lo, shift) for u in images]
    assert all(0 <= x < TOPK_BINS for x in d)
    hist = [0] * TOPK_BINS
    for x in d:
        hist[x] += 1
    b, above = 0, 0
    for cand in range(TOPK_BINS - 1, -1, -1):          # the highest bin with `want` rows in it and above it
        above += hist[cand]
        if above >= want:
            b = cand
            break
    return [i for i, x in enumerate(d) if x >= b]


class TopkCase:
    """rows [n, stride] of random words with the sort key in word key_word and the row's id in the word behind it (cyclically).  kinds:
    random32 - the key is the low 32 bits, negative values among them, the upper 32 random; equal - one image (hi == lo); minmax - only
    INT64_MIN and INT64_MAX (a full 64-bit span: shift 0); low9 / top11 - keys that differ in their low 9 / top 11 bits only (the
    threshold is decided by the last / first digit of the radix select); ties - 5 rows above a value that 300 rows share."""

    def __init__(self, n, kind, want, stride=2, key_word=0, desc=True, capacity=None, rows_upper_bound=None, overflow=False, seed=0):
        rng = np.random.default_rng(n * 19 + TOPK_KINDS.index(kind) * 3 + stride + seed * 1000)
        self.n, self.kind, self.want, self.stride, self.key_word, self.desc = n, kind, want, stride, key_word, desc
        self.is32 = kind == "random32"
        self.capacity = n + 1 if capacity is None else capacity
        self.rows_upper_bound, self.overflow = rows_upper_bound, overflow
        if kind == "random64":
            k = rng.integers(INT64_MIN, INT64_MAX, n, dtype=np.int64, endpoint=True)
        elif kind == "random32":
            k = rng.integers(-(1 << 31), 1 << 31, n, dtype=np.int64) & 0xffffffff | rng.integers(INT64_MIN, INT64_MAX, n, dtype=np.int64) & ~np.int64(0xffffffff)
        elif kind == "equal":
            k = np.full(n, -123456789, dtype=np.int64)
        elif kind == "minmax":
            k = np.where(rng.integers(0, 2, n) == 1, INT64_MAX, INT64_MIN).astype(np.int64)
        elif kind == "low9":
            k = np.int64(0x1234567890abc000) + rng.integers(0, 512, n, dtype=np.int64)
        elif kind == "top11":
            k = (rng.integers(0, 2048, n, dtype=np.uint64) << np.uint64(53) | np.uint64(0x000fedcba9876543)).view(np.int64)
        elif kind == "ties":
            assert n >= 400
            k = rng.integers(-1000, 1000, n, dtype=np.int64)
            where = rng.permutation(n)
            k[where[:300]] = 5000 if desc else -5000
            k[where[300:305]] = (6000 if desc else -6000) + np.arange(5) * (1 if desc else -1)
        else:
            raise AssertionError(kind)
        self.rows = rng.integers(INT64_MIN, INT64_MAX, (n, stride), dtype=np.int64)
        self.rows[:, key_word] = k
        self.rows[:, (key_word + 1) % stride] = TOPK_ID_BASE + TOPK_ID_STEP * np.arange(n, dtype=np.int64)

    @property
    def id_word(self):
        return (self.key_word + 1) % self.stride

    def seen(self):
        """the rows the kernels take: min(n_rows, rows_upper_bound)"""
        return self.n if self.rows_upper_bound is None else min(self.n, self.rows_upper_bound)

    def images(self):
        return topk_image(self.rows[:self.seen(), self.key_word], self.is32, self.desc)

    def name(self):
        return (f"n{self.n}_{self.kind}_want{self.want}_s{self.stride}k{self.key_word}_{'desc' if self.desc else 'asc'}"
                + (f"_bound{self.rows_upper_bound}" if self.rows_upper_bound is not None else "") + ("_overflow" if self.overflow else ""))


def topk_cases():
    out = []
    for j, n in enumerate(TOPK_SIZES):          # every size with want = 1, n - 1, n, n + 1, ascending and descending in turn
        for i, want in enumerate(sorted({1, n - 1, n, n + 1} - {0})):
            out.append(TopkCase(n, "random64", want, stride=2, key_word=(i + j) % 2, desc=(i + j) % 2 == 0))
    for n in (257, 2049):                       # every kind of key in both orders, a few, some and all rows wanted
        for kind in TOPK_KINDS:
            if kind == "ties":
                continue
            for desc in (True, False):
                for want in (1, 100, n):
                    out.append(TopkCase(n, kind, want, stride=3, key_word=2, desc=desc))
    for stride, key_word in [(2, 0), (2, 1), (3, 1), (9, 0), (9, 4), (9, 8)]:          # the key in the first, a middle and the last word
        for kind in ("random64", "random32"):
            out.append(TopkCase(2049, kind, 40, stride=stride, key_word=key_word, desc=stride != 3))
    out.append(TopkCase(600_001, "random32", 1000, stride=3, key_word=1, desc=False))
    out.append(TopkCase(600_001, "low9", 50_000, stride=2, key_word=1, desc=True))
    for desc in (True, False):                  # the tie set at the threshold: inside the capacity, and larger than it
        out.append(TopkCase(2049, "ties", 10, stride=3, key_word=0, desc=desc))
        out.append(TopkCase(2049, "ties", 10, stride=3, key_word=0, desc=desc, capacity=100, overflow=True))
    out.append(TopkCase(600_001, "equal", 7, stride=2, key_word=0, capacity=1000, overflow=True))
    for n, bound in [(2049, 1000), (2049, 2048), (2049, 2050), (2049, 1 << 31), (600_001, 70_000), (257, 0)]:      # below and above n_rows
        out.append(TopkCase(n, "random64", 33, stride=2, key_word=1, desc=True, rows_upper_bound=bound))
    return out
