"""The references of tests/primcases.py are not taken on trust: each vectorised one is held against a plain Python loop, count by count
and bit by bit, over a few hundred random small inputs (and the forms the GPU test uses them in).  The constants it takes from the
source are read from the source.  The rsq_prim_* entry points refuse bad arguments without a launch, and a context without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from resql_amd import engine

import primcases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "resql_amd", "csrc")


def test_constants_are_the_sources():
    aot = open(os.path.join(SRC, "aot_kernels.hip")).read()
    scan = open(os.path.join(SRC, "scan_device.h")).read()
    define = lambda text, name: int(re.search(rf"^#define {name} (\d+)", text, re.M).group(1))
    assert define(scan, "SCAN_CHUNK") == pc.SCAN_CHUNK
    assert define(scan, "SCAN_BATCH") == pc.SCAN_BATCH == pc.SM_BATCH          # one batch size for every single-workgroup scan
    assert pc.SCAN_CHUNK == 4 * pc.SCAN_BATCH          # four sub-blocks per chunk
    eng = open(os.path.join(SRC, "engine.h")).read()
    assert define(eng, "RSQ_RANK_CHUNK_BLOCKS") == pc.RANK_CHUNK_BLOCKS == engine.RANK_CHUNK_BLOCKS
    tail = open(os.path.join(SRC, "devtail.hip")).read()
    assert define(tail, "RS_TILE") == pc.RS_TILE
    assert define(scan, "SM_CHUNK") == pc.SM_CHUNK
    assert define(scan, "SM_PER_THREAD") == pc.SM_PER_THREAD == 16 and pc.SM_CHUNK == 256 * 16          # 16 values per thread, 1024 per wave
    m = re.search(r"enum \{ TOPK_PASSES = (\d+), TOPK_BINS = (\d+) \}", aot)
    assert (int(m.group(1)), int(m.group(2))) == (pc.TOPK_PASSES, pc.TOPK_BINS)
    assert 5 * 11 + 9 == 64 and pc.TOPK_BINS == 1 << 11          # topk_shift / topk_bits: five 11-bit digits and one of 9
    plan = open(os.path.join(ROOT, "include", "resql_plan.h")).read()
    for name, tag in [("VARCHAR", pc.T_VARCHAR), ("CHAR", pc.T_CHAR), ("BOOL", pc.T_BOOL), ("INT", pc.T_INT), ("BIGINT", pc.T_BIGINT),
                      ("DECIMAL", pc.T_DECIMAL), ("DATE", pc.T_DATE)]:
        assert int(re.search(rf"RSQ_{name}\s*=\s*(\d+)", plan).group(1)) == tag


def test_case_lists_hold_the_boundaries():
    s = set(pc.SCAN_SIZES)
    assert {1, 2, 3, 4, 5, 255, 1023, 1024, 1025, 1027, 4095, 4096, 4097, 8191, 8193, 64 * 4096 - 1, 64 * 4096, 64 * 4096 + 1, 65 * 4096 + 3,
            129 * 4096 + 2, 1026 * 4096 + 5} == s
    assert max(s) // pc.SCAN_CHUNK > pc.SCAN_BATCH          # more chunk totals than one batch of their scan
    assert set(pc.RANK_BLOCKS) == {1, 3, 4, 5, 1023, 1024, 1025, 2 * 1024 + 1, 64 * 1024, 64 * 1024 + 1, 65 * 1024 + 7, 130 * 1024 + 3}
    assert (max(pc.RANK_BLOCKS) + pc.RANK_CHUNK_BLOCKS - 1) // pc.RANK_CHUNK_BLOCKS < 1171      # the one-launch index's grid limit
    assert pc.PLACE_BITS == 3 * 1024 * 224 + 100 and pc.PLACE_MIN < 0
    assert all(0 <= d < pc.PLACE_BITS for d in pc.PLACE_EDGES) and len(set(pc.PLACE_EDGES)) == len(pc.PLACE_EDGES)
    pos = [pc.bit_position(d) for d in pc.PLACE_EDGES]
    assert {0, 31} <= {b for _, _, b in pos} and {1, 7} <= {w for _, w, _ in pos}
    assert {(1023, 7, 31), (1024, 1, 0)} <= set(pos)          # last key of a chunk of the index, first of the next
    # the sort: tiles of 2048 in rounds of 256, waves of 64; every key_bits with 2049 and 600 001, every size with the result in either buffer
    sort = pc.sort_cases()
    assert set(pc.SORT_SIZES) == {0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4097, 3 * 2048 + 1, 600_001} == {c[0] for c in sort}
    assert pc.SORT_KEY_BITS == [1, 8, 9, 16, 17, 24, 32, 33, 41, 63, 64]
    assert [pc.sort_passes(b) for b in pc.SORT_KEY_BITS] == [1, 1, 2, 2, 3, 3, 4, 5, 6, 8, 8]
    assert (600_001 + pc.RS_TILE - 1) // pc.RS_TILE == 293
    for n in pc.SORT_SIZES:
        assert {pc.sort_passes(b) % 2 for m, b, _, _ in sort if m == n} == {0, 1}, n
    for b in pc.SORT_KEY_BITS:
        assert {2049, 600_001} <= {n for n, kb, _, _ in sort if kb == b}, b
        assert {p for n, kb, p, _ in sort if kb == b and n == 2049} == set(pc.SORT_PATTERNS)
    assert {p for n, _, p, _ in sort if n == 600_001} == set(pc.SORT_PATTERNS)
    for n in pc.SORT_SIZES:
        assert {p for m, _, p, _ in sort if m == n} == set(pc.SORT_PATTERNS)
    assert any(v == "random" for _, _, _, v in sort) and 0xffffffff in pc.sort_vals(100, "random")
    # the running minimum: a thread's 16 values, a wave's 1024, a chunk's 4096, 1024 chunk minima per batch
    assert set(pc.RUNMIN_SIZES) == {1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 2 * 4096 + 1, 1024 * 4096 - 1, 1024 * 4096, 1024 * 4096 + 1,
                                    1025 * 4096 + 17}
    assert sum((n + pc.SM_CHUNK - 1) // pc.SM_CHUNK > pc.SM_BATCH for n in pc.RUNMIN_SIZES) == 2          # two sizes put chunks into a second batch ...
    assert (1024 * 4096 + pc.SM_CHUNK - 1) // pc.SM_CHUNK == pc.SM_BATCH                                   # ... the two below fill the first to its end
    assert {(n, p) for n, p, _ in pc.runmin_cases() if p != "single"} == {(n, p) for n in pc.RUNMIN_SIZES for p in pc.RUNMIN_PATTERNS}
    single = {(n, at) for n, p, at in pc.runmin_cases() if p == "single"}
    big = 1025 * 4096 + 17
    assert {(big, 4095), (big, 4096), (big, 1023 * 4096 + 4095), (big, 1024 * 4096), (2 * 4096 + 1, 4095), (2 * 4096 + 1, 4096),
            (2 * 4096 + 1, 15), (2 * 4096 + 1, 16), (2 * 4096 + 1, 1023), (2 * 4096 + 1, 1024)} <= single
    assert all(0 <= at < n for n, at in single)
    # the merge
    merge = pc.merge_cases()
    assert set(pc.MERGE_SIZES) == {1, 2, 255, 256, 257, 100_003} == {c[0] for c in merge}
    for n in pc.MERGE_SIZES:
        assert {g for m, g, _, _ in merge if m == n} == set(pc.MERGE_GROUPINGS) and {k for m, _, k, _ in merge if m == n} == set(pc.MERGE_KEYSETS)
    assert {a for _, _, _, a in merge if a} == set(pc.MERGE_ACCSETS)
    for keyset in pc.MERGE_KEYSETS:
        assert {a for _, _, k, a in merge if k == keyset} == set(pc.MERGE_ACCSETS), keyset
    # the selection
    topk = pc.topk_cases()
    assert set(pc.TOPK_SIZES) == {1, 255, 256, 257, 2047, 2049, 600_001} and 600_001 > 256 * 256
    for n in pc.TOPK_SIZES:
        assert {1, n - 1, n, n + 1} - {0} <= {c.want for c in topk if c.n == n and c.kind == "random64"}, n
        assert {c.desc for c in topk if c.n == n} == {True, False}
    assert {c.kind for c in topk} == set(pc.TOPK_KINDS)
    assert {(2, 0), (2, 1), (3, 1), (9, 0), (9, 4), (9, 8)} <= {(c.stride, c.key_word) for c in topk}
    assert any(c.is32 and (c.rows[:, c.key_word] & 0x80000000 != 0).any() and (c.rows[:, c.key_word] >> 32 != 0).any() for c in topk)
    bounds = {(c.n, c.rows_upper_bound) for c in topk if c.rows_upper_bound is not None}
    assert any(b < n for n, b in bounds) and any(b > n for n, b in bounds)
    assert len({c.name() for c in topk}) == len(topk)


@pytest.mark.parametrize("pattern", pc.SCAN_PATTERNS)
def test_scan_reference_against_a_loop(pattern):
    rng = np.random.default_rng(1)
    sizes = [1, 2, 3, 4, 5, 255, 4095, 4096, 4097, 2 * 4096 + 1] + [int(x) for x in rng.integers(1, 3 * 4096, 40)]
    for n in sizes:
        c = pc.scan_counts(n, pattern, seed=n)
        assert c.dtype == np.uint32 and len(c) == n
        assert [int(x) for x in pc.scan_reference(c)] == pc.scan_reference_loop(c), (pattern, n)
    if pattern == "max32":
        assert int(pc.scan_reference(pc.scan_counts(3, pattern))[2]) == 2 * 0xffffffff          # 64-bit sums, no wrap at 32
    if pattern == "empty_chunks":
        c = pc.scan_counts(10 * 4096 + 5, pattern)
        per_chunk = [int(c[i:i + 4096].sum()) for i in range(0, len(c), 4096)]
        assert per_chunk[0] == 0 and 0 in per_chunk[1:] and any(per_chunk)


@pytest.mark.parametrize("density", pc.RANK_DENSITIES)
def test_rank_reference_against_a_loop(density):
    rng = np.random.default_rng(2)
    for n in [1, 3, 4, 5, 1023, 1024, 1025, 2049] + [int(x) for x in rng.integers(1, 300, 60)]:
        b = pc.rank_blocks(n, density, seed=n)
        assert b.shape == (n, 8) and b.dtype == np.uint32
        rank, base = pc.rank_reference(b)
        want_rank, want_base = pc.rank_reference_loop(b)
        assert [int(x) for x in rank] == want_rank and [int(x) for x in base] == want_base, (density, n)
        assert len(base) == (n + 1023) // 1024 + 1
    b = pc.rank_blocks(50, density)
    total = int(pc.rank_reference(b)[1][-1])
    assert total == {"empty": 0, "full": 50 * 224, "last_block_one_bit": 1}.get(density, total)
    if density == "one_percent":
        assert 0 < total < 50 * 224 // 20
    if density == "last_block_one_bit":
        assert not b[:-1, 1:].any()


def test_bitmap_of_offsets_against_a_loop():
    rng = np.random.default_rng(3)
    for trial in range(200):
        bits = int(rng.integers(1, 3000))
        d = np.unique(rng.integers(0, bits, int(rng.integers(0, 60))))
        if trial % 4 == 0:
            d = np.unique(np.append(d, [0, bits - 1]))
        got = pc.blocks_of_offsets(d, bits)
        assert got.tolist() == pc.blocks_of_offsets_loop(d, bits), (trial, bits)
        # the rank of offset d by the index's own arithmetic = its position among the sorted offsets
        rank, base = pc.rank_reference(got)
        for k, x in enumerate(d):
            blk, word, bit = pc.bit_position(int(x))
            below = sum(bin(int(got[blk, w])).count("1") for w in range(1, word)) + bin(int(got[blk, word]) & ((1 << bit) - 1)).count("1")
            assert int(rank[blk]) + below == k
        assert int(base[-1]) == len(d)


def test_placement_reference_against_a_loop():
    for seed in range(6):
        for n_words, n_waves, shift in [(1, 1, 1), (2, 3, 0), (3, 1, 2), (5, 3, 5), (9, 1, 4), (12, 3, 2)]:
            case = pc.PlaceCase(n_words, n_waves, used_shift=shift, seed=seed)
            n = int(case.used.sum())
            assert case.region % 64 == 0 and case.region >= int(case.used.max()) and (case.region == 64 or case.region - 64 < int(case.used.max()))
            assert len(case.rec) == n and len(set(case.rec[:, 0].tolist())) == n
            assert set(case.offsets().tolist()) >= set(pc.PLACE_EDGES[:n])
            want, distinct = case.expected()
            loop, loop_distinct = pc.place_reference_loop(case.rec, n_words, case.bm_min, case.bm_bits, case.capacity)
            assert want.tolist() == loop and distinct == loop_distinct == n
            assert (want[n:] == -1).all()
            assert int(pc.rank_reference(case.blocks())[1][-1]) == n
            # the arrival-order buffer holds the records region by region
            buf = case.records().reshape(n_waves, case.region, n_words)
            assert np.array_equal(np.concatenate([buf[w, :u] for w, u in enumerate(case.used)]), case.rec)
    # a key outside the domain has no bit and no entry; a key that occurs twice has one of each
    case = pc.PlaceCase(3, 3, used_shift=1, seed=9)
    case.rec[5, 0] = case.bm_min + case.bm_bits
    case.rec[7, 0] = case.rec[9, 0]
    want, distinct = case.expected()
    loop, loop_distinct = pc.place_reference_loop(case.rec, 3, case.bm_min, case.bm_bits, case.capacity)
    assert distinct == loop_distinct == len(case.rec) - 2 and int(pc.rank_reference(case.blocks())[1][-1]) == distinct
    assert want.tolist() == loop


def test_every_used_value_is_a_one_wave_case_and_every_width_has_every_wave_count():
    cases = pc.place_cases()
    assert sorted(int(c.used[0]) for _, c in cases if c.n_waves == 1) == sorted(pc.PLACE_USED)
    assert {(c.n_words, c.n_waves) for _, c in cases} == {(w, v) for w in pc.PLACE_WORDS for v in pc.PLACE_WAVES}
    for _, c in cases:
        if c.n_waves == 70:
            assert set(c.used.tolist()) == set(pc.PLACE_USED)


@pytest.mark.parametrize("pattern", pc.SORT_PATTERNS)
def test_sort_reference_against_a_loop(pattern):
    rng = np.random.default_rng(4)
    for trial, n in enumerate([0, 1, 2, 63, 64, 65, 255, 256, 257] + [int(x) for x in rng.integers(1, 700, 30)]):
        for key_bits in (pc.SORT_KEY_BITS[trial % len(pc.SORT_KEY_BITS)], pc.SORT_KEY_BITS[(trial + 5) % len(pc.SORT_KEY_BITS)]):
            keys = pc.sort_keys(n, key_bits, pattern, seed=trial)
            vals = pc.sort_vals(n, "random" if trial % 3 == 0 else "arange", seed=trial)
            assert keys.dtype == np.uint64 and vals.dtype == np.uint32 and len(keys) == len(vals) == n
            got_keys, got_vals = pc.sort_reference(keys, vals, key_bits)
            want_keys, want_vals = pc.sort_reference_loop(keys, vals, key_bits)
            assert got_keys.tolist() == want_keys and got_vals.tolist() == want_vals, (pattern, n, key_bits)
    # what the patterns promise
    assert pc.sort_mask(1) == 0xff and pc.sort_mask(9) == 0xffff and pc.sort_mask(41) == (1 << 48) - 1 and pc.sort_mask(64) == (1 << 64) - 1
    for key_bits in pc.SORT_KEY_BITS:
        k, mask, passes = pc.sort_keys(2049, key_bits, pattern), pc.sort_mask(key_bits), pc.sort_passes(key_bits)
        digits = np.stack([(k >> np.uint64(8 * d)) & np.uint64(255) for d in range(passes)])
        if pattern == "equal":
            assert len(np.unique(k)) == 1
        if pattern == "digits_0_255":
            assert set(np.unique(digits).tolist()) == {0, 255}
        if pattern == "lane_digits":
            assert all(len(np.unique(digits[d, r:r + 256])) == 256 for d in range(passes) for r in range(0, 2048, 256))
        if pattern == "ascending":
            assert (np.diff((k & np.uint64(mask)).astype(object)) >= 0).all()
        if pattern == "descending":
            assert (np.diff((k & np.uint64(mask)).astype(object)) <= 0).all() and (key_bits == 1 or k[0] > k[-1])
        if pattern == "copies50":
            assert len(np.unique(k)) <= 2049 // 50 + 1 and (int(k.max()) <= mask)
        if pattern == "top_byte":
            assert all(len(np.unique(digits[d])) == 1 for d in range(passes - 1)) and len(np.unique(digits[passes - 1])) > 1
        if pattern == "above_mask":
            assert key_bits > 56 or ((k & ~np.uint64(mask)) != 0).any()
            assert pc.sort_reference(k, np.arange(2049, dtype=np.uint32), key_bits)[1].tolist() == \
                pc.sort_reference(k & np.uint64(mask), np.arange(2049, dtype=np.uint32), key_bits)[1].tolist()


@pytest.mark.parametrize("pattern", pc.RUNMIN_PATTERNS + ["single"])
def test_running_minimum_reference_against_a_loop(pattern):
    rng = np.random.default_rng(5)
    for n in [1, 15, 16, 17, 1023, 1024, 1025] + [int(x) for x in rng.integers(1, 3000, 40)]:
        v = pc.runmin_values(n, pattern, seed=n, at=n // 2)
        assert v.dtype == np.int64 and len(v) == n
        assert pc.runmin_reference(v).tolist() == pc.runmin_reference_loop(v), (pattern, n)
    v = pc.runmin_values(5000, pattern, at=4095)
    if pattern == "increasing":
        assert (np.diff(v) > 0).all() and (pc.runmin_reference(v) == v[0]).all()
    if pattern == "decreasing":
        assert (np.diff(v) < 0).all() and np.array_equal(pc.runmin_reference(v), v)
    if pattern == "random":
        assert v.min() < 0 < v.max()
    if pattern == "holds_max":
        assert v[0] == pc.INT64_MAX and (v == pc.INT64_MAX).sum() > 4000 and (v != pc.INT64_MAX).any()
    if pattern == "single":
        want = np.full(5000, pc.INT64_MAX, dtype=np.int64)
        want[4095:] = pc.INT64_MIN
        assert np.array_equal(pc.runmin_reference(v), want)


@pytest.mark.parametrize("keyset", pc.MERGE_KEYSETS)
def test_merge_reference_against_a_loop(keyset):
    rng = np.random.default_rng(6)
    trial = 0
    for n in [1, 2, 3, 255, 256, 257] + [int(x) for x in rng.integers(1, 400, 12)]:
        for grouping in pc.MERGE_GROUPINGS:
            trial += 1
            case = pc.MergeCase(n, grouping, keyset, pc.MERGE_ACCSETS[trial % 3], seed=trial)
            assert case.stride == 1 + case.n_tab + len(case.accs) and len(set(case.rows[:, 0].tolist())) == n
            got = pc.merge_reference(case.rows, case.n_tab, case.keys, case.accs)
            want = pc.merge_reference_loop(case.rows, case.n_tab, case.keys, case.accs)
            assert got.tolist() == want, (keyset, n, grouping)
            varchar = any(tag == pc.T_VARCHAR for _, tag, _ in case.keys)
            if grouping == "one" and not varchar:
                assert len(got) == 1 and got[0, 0] == case.rows[:, 0].min()
            if grouping == "one" and varchar and n >= 255:
                assert 1 < len(got) <= 21          # the same text with 0..20 trailing spaces: different VARCHARs
            if grouping == "distinct" and keyset != "bool_char1":
                assert len(got) == n
            if grouping == "three" and keyset in ("bigint", "int_date", "char12", "composite") and n >= 255:
                # every group three members, one per shard, and the smallest first row in each position in turn
                third = n // 3
                assert len(got) == third + n % 3
                owner = {int(f): i for i, f in enumerate(case.rows[:, 0])}
                shard_of_best = np.array([owner[int(f)] // third for f in got[:, 0]])
                assert min((shard_of_best == s).sum() for s in range(3)) >= third // 3
    # the rules, one by one, on rows written out by hand: [first | key words | sum]
    word = lambda text: int.from_bytes(text.ljust(8, b"\0")[:8], "little", signed=True)
    rows = np.array([[10, word(b"abc     "), word(b"    \xff\xff\xff\xff"), 1], [4, word(b"abc\0zzzz"), word(b"zzzz\x01\x02\x03\x04"), 2],
                     [7, word(b"abc "), word(b"\0"), 4]], dtype=np.int64)
    one = pc.merge_reference(rows, 2, [(1, pc.T_CHAR, 12)], [(3, 0)])
    assert one.tolist() == [[4, word(b"abc\0zzzz"), word(b"zzzz\x01\x02\x03\x04"), 7]]          # the spelling of the member with first row 4
    assert len(pc.merge_reference(rows, 2, [(1, pc.T_VARCHAR, 12)], [(3, 0)])) == 3
    rows = np.array([[1, (5 << 32) | 77, pc.INT64_MAX], [2, (9 << 32) | 77, 1], [3, 77 | (1 << 31), 0]], dtype=np.int64)
    assert pc.merge_reference(rows, 1, [(1, pc.T_INT, 0)], [(2, 0)]).tolist() == [[1, (5 << 32) | 77, pc.INT64_MIN], [3, 77 | (1 << 31), 0]]
    assert len(pc.merge_reference(rows, 1, [(1, pc.T_BIGINT, 0)], [(2, 0)])) == 3
    assert len(pc.merge_reference(rows, 1, [(1, pc.T_BOOL, 0)], [(2, 2)])) == 1 and len(pc.merge_reference(rows, 1, [(1, pc.T_CHAR, 1)], [(2, 3)])) == 1
    # wrapping sums and extreme values occur in the cases that are named for them
    wrap = pc.MergeCase(257, "three", "bigint", "wrap")
    sums = [sum(int(x) for x in wrap.rows[wrap.rows[:, 1] == k, wrap.accs[0][0]]) for k in np.unique(wrap.rows[:, 1])]
    assert any(not pc.INT64_MIN <= s <= pc.INT64_MAX for s in sums)
    ext = pc.MergeCase(257, "three", "bigint", "extremes")
    assert all({pc.INT64_MIN, pc.INT64_MAX} <= set(ext.rows[:, w].tolist()) for w, _ in ext.accs)


def test_topk_references_against_loops():
    rng = np.random.default_rng(7)
    for trial in range(300):
        n = int(rng.integers(1, 200))
        kind = [k for k in pc.TOPK_KINDS if k != "ties"][trial % 6]
        want = [1, max(1, n - 1), n, n + 1, int(rng.integers(1, n + 1))][trial % 5]
        stride = int(rng.integers(2, 6))
        case = pc.TopkCase(n, kind, want, stride=stride, key_word=int(rng.integers(0, stride)), desc=trial % 2 == 0, seed=trial)
        images = case.images()
        assert images.dtype == np.uint64
        assert images.tolist() == [pc.topk_image_loop(w, case.is32, case.desc) for w in case.rows[:, case.key_word]]
        exact = pc.topk_reference(images, want)
        assert exact.tolist() == pc.topk_reference_loop(images, want), (trial, kind)
        assert len(exact) >= min(want, n)
        rng2 = pc.topk_exact_range(images)
        lo = int(images.min())
        ranges = [rng2, pc.topk_wider_range(rng2), (pc.U64, pc.U64), (int(rng.integers(0, 1 << 63)), int(rng.integers(0, 1 << 63)))]
        for k, r in enumerate(ranges):
            members = pc.topk_range_reference(images, want, r)
            assert members.tolist() == pc.topk_range_reference_loop(images, want, r), (trial, kind, r)
            if k < 3:          # a range that holds the data: a superset of the exact selection
                assert set(exact.tolist()) <= set(members.tolist())
        shift = pc.topk_range_shift(rng2[0], lo)
        assert pc.topk_range_digit(images, lo, shift).tolist() == [pc.topk_range_digit_loop(u, lo, shift) for u in images]
        if kind == "equal":
            assert rng2[0] == lo and shift == 0
        if kind == "minmax" and len(np.unique(images)) == 2:
            assert shift == 0 and rng2[0] - lo == pc.U64
    # order: descending takes the largest keys, ascending the smallest; is32 looks at the low half only
    assert pc.topk_reference(pc.topk_image(np.array([3, -5, 9]), False, True), 1).tolist() == [2]
    assert pc.topk_reference(pc.topk_image(np.array([3, -5, 9]), False, False), 1).tolist() == [1]
    assert pc.topk_reference(pc.topk_image(np.array([(7 << 32) | 3, 0xfffffffb, (1 << 40) | 9]), True, False), 1).tolist() == [1]


def test_topk_case_capacities_mean_what_they_say():
    """every case's candidate counts, by the references, stay inside its capacity - or exceed it where the case is the overflow case"""
    seen_overflow = 0
    for case in pc.topk_cases():
        images = case.images()
        assert len(images) == (case.n if case.rows_upper_bound is None else min(case.n, case.rows_upper_bound))
        rng2 = pc.topk_exact_range(images)
        counts = [len(pc.topk_reference(images, case.want)), len(pc.topk_range_reference(images, case.want, rng2)),
                  len(pc.topk_range_reference(images, case.want, pc.topk_wider_range(rng2)))]
        if case.overflow:
            assert min(counts) > case.capacity, case.name()
            seen_overflow += 1
        else:
            assert max(counts) < case.capacity, case.name()
        if case.kind == "ties":
            assert counts[0] == 305 and case.want < counts[0]
    assert seen_overflow >= 3


def test_notes_are_named():
    assert pc.notes_text(0) == "none"
    assert pc.notes_text(64 | 512).startswith("64:") and "512:" in pc.notes_text(64 | 512)


# ---- argument validation of the entry points (no device: nothing can be launched) ----
def _call(ctx, name, *args):
    return getattr(ctx._L, name)(ctx.h, *args)


def test_entry_points_refuse_bad_arguments_and_contexts_without_a_device(compile_ctx):
    ctx = compile_ctx
    notes = C.c_uint32(7)
    pn = C.addressof(notes)
    counts, offs = np.ones(8, np.uint32), np.zeros(8, np.uint64)
    blocks, base = np.zeros((4, 8), np.uint32), np.zeros(2, np.uint32)
    rec, used, out = np.zeros(64 * 2, np.int64), np.array([3], np.uint32), np.zeros((10, 2), np.int64)
    p = lambda a: a.ctypes.data
    INVALID, UNSUPPORTED = 1, 3
    # well-formed calls: no device
    assert _call(ctx, "rsq_prim_exclusive_scan", p(counts), 8, 0, p(offs), pn) == UNSUPPORTED
    assert _call(ctx, "rsq_prim_exclusive_scan", p(counts), 8, 1, p(offs), pn) == UNSUPPORTED
    assert _call(ctx, "rsq_prim_rank_index", p(blocks), 4, 0, p(base), pn) == UNSUPPORTED
    assert _call(ctx, "rsq_prim_rank_index", p(blocks), 4, 1, p(base), pn) == UNSUPPORTED
    place = lambda **kw: _call(ctx, "rsq_prim_rank_place", *[{**dict(blocks=p(blocks), n_blocks=4, bm_min=-5, bm_bits=4 * 224, records=p(rec), used=p(used),
                                                                      n_waves=1, region=64, n_words=2, capacity=10, out=p(out), notes=pn), **kw}[k]
                                                             for k in ("blocks", "n_blocks", "bm_min", "bm_bits", "records", "used", "n_waves", "region", "n_words",
                                                                       "capacity", "out", "notes")])
    assert place() == UNSUPPORTED
    assert notes.value == 0          # (set before anything else)
    with pytest.raises(engine.EngineError) as e:
        ctx.prim_scan(counts, 0)
    assert e.value.status == UNSUPPORTED
    # null pointers, negative sizes, forms that do not exist
    assert _call(ctx, "rsq_prim_exclusive_scan", None, 8, 0, p(offs), pn) == INVALID
    assert _call(ctx, "rsq_prim_exclusive_scan", p(counts), 8, 0, None, pn) == INVALID
    assert _call(ctx, "rsq_prim_exclusive_scan", p(counts), 8, 0, p(offs), None) == INVALID
    assert _call(ctx, "rsq_prim_exclusive_scan", p(counts), -1, 0, p(offs), pn) == INVALID
    assert _call(ctx, "rsq_prim_exclusive_scan", p(counts), 8, 2, p(offs), pn) == INVALID
    assert ctx._L.rsq_prim_exclusive_scan(None, p(counts), 8, 0, p(offs), pn) == INVALID
    assert _call(ctx, "rsq_prim_rank_index", None, 4, 0, p(base), pn) == INVALID
    assert _call(ctx, "rsq_prim_rank_index", p(blocks), 4, 0, None, pn) == INVALID
    assert _call(ctx, "rsq_prim_rank_index", p(blocks), 4, 0, p(base), None) == INVALID
    assert _call(ctx, "rsq_prim_rank_index", p(blocks), -4, 0, p(base), pn) == INVALID
    assert _call(ctx, "rsq_prim_rank_index", p(blocks), 4, -1, p(base), pn) == INVALID
    for kw in (dict(blocks=None), dict(records=None), dict(used=None), dict(out=None), dict(notes=None), dict(n_blocks=-1), dict(n_blocks=0),
               dict(n_waves=-1), dict(n_waves=0), dict(region=0), dict(n_words=0), dict(n_words=-3), dict(capacity=0), dict(capacity=-1),
               dict(bm_bits=0), dict(bm_bits=4 * 224 + 1),          # a key's block would lie behind the bitmap
               dict(region=2)):                                     # used[0] = 3 records do not fit the region
        assert place(**kw) == INVALID, kw


def test_tail_entry_points_refuse_bad_arguments_and_contexts_without_a_device(compile_ctx):
    """rsq_prim_radix_sort_pairs, rsq_prim_running_min, rsq_prim_merge_group_rows, rsq_prim_topk_select: every refused shape is
    RSQ_ERR_INVALID before anything is allocated or launched, a well-formed call on a compile-only context RSQ_ERR_UNSUPPORTED"""
    ctx = compile_ctx
    notes = C.c_uint32(7)
    pn = C.addressof(notes)
    p = lambda a: None if a is None else a.ctypes.data
    INVALID, UNSUPPORTED = 1, 3
    pick = lambda defaults, order, kw: [{**defaults, **kw}[k] for k in order]

    # ---- sort ----
    keys, vals, keys_out, vals_out = np.arange(8, dtype=np.uint64), np.arange(8, dtype=np.uint32), np.zeros(8, np.uint64), np.zeros(8, np.uint32)
    order = ("keys", "vals", "n", "key_bits", "keys_out", "vals_out", "notes")
    sort = lambda **kw: _call(ctx, "rsq_prim_radix_sort_pairs", *pick(dict(keys=p(keys), vals=p(vals), n=8, key_bits=24, keys_out=p(keys_out),
                                                                           vals_out=p(vals_out), notes=pn), order, kw))
    assert sort() == UNSUPPORTED and notes.value == 0
    assert sort(key_bits=1) == UNSUPPORTED and sort(key_bits=64) == UNSUPPORTED and sort(n=0) == UNSUPPORTED and sort(n=1) == UNSUPPORTED
    for kw in (dict(keys=None), dict(vals=None), dict(keys_out=None), dict(vals_out=None), dict(notes=None), dict(n=-1), dict(n=(1 << 31) + 1),
               dict(key_bits=0), dict(key_bits=-8), dict(key_bits=65)):
        assert sort(**kw) == INVALID, kw
    assert ctx._L.rsq_prim_radix_sort_pairs(None, p(keys), p(vals), 8, 24, p(keys_out), p(vals_out), pn) == INVALID
    with pytest.raises(engine.EngineError) as e:
        ctx.prim_radix_sort_pairs(keys, vals, 24)
    assert e.value.status == UNSUPPORTED

    # ---- running minimum ----
    v, out = np.arange(8, dtype=np.int64), np.zeros(8, np.int64)
    assert _call(ctx, "rsq_prim_running_min", p(v), 8, p(out), pn) == UNSUPPORTED
    assert _call(ctx, "rsq_prim_running_min", p(v), 0, p(out), pn) == UNSUPPORTED
    assert _call(ctx, "rsq_prim_running_min", None, 8, p(out), pn) == INVALID
    assert _call(ctx, "rsq_prim_running_min", p(v), 8, None, pn) == INVALID
    assert _call(ctx, "rsq_prim_running_min", p(v), 8, p(out), None) == INVALID
    assert _call(ctx, "rsq_prim_running_min", p(v), -1, p(out), pn) == INVALID
    assert ctx._L.rsq_prim_running_min(None, p(v), 8, p(out), pn) == INVALID
    with pytest.raises(engine.EngineError) as e:
        ctx.prim_running_min(v)
    assert e.value.status == UNSUPPORTED

    # ---- merge: rows [first | BIGINT | CHAR(12) in two words | INT | sum | min | max], stride 8, four table words ----
    rows, out_rows, count = np.zeros((5, 8), np.int64), np.zeros((5, 8), np.int64), C.c_uint64(0)
    i32 = lambda *x: np.array(x, dtype=np.int32)
    order = ("rows", "n", "stride", "n_tab", "key_word", "key_type", "key_len", "n_keys", "acc_word", "acc_kind", "n_acc", "out_rows", "out_count", "notes")
    good = dict(rows=p(rows), n=5, stride=8, n_tab=4, key_word=i32(1, 2, 4), key_type=i32(pc.T_BIGINT, pc.T_CHAR, pc.T_INT), key_len=i32(0, 12, 0), n_keys=3,
                acc_word=i32(5, 6, 7), acc_kind=i32(0, 2, 3), n_acc=3, out_rows=p(out_rows), out_count=C.addressof(count), notes=pn)

    def merge(**kw):
        a = {**good, **kw}
        return _call(ctx, "rsq_prim_merge_group_rows", *[p(a[k]) if isinstance(a[k], np.ndarray) else a[k] for k in order])
    assert merge() == UNSUPPORTED and notes.value == 0
    assert merge(key_len=i32(0, 16, 0)) == UNSUPPORTED          # (a string that fills its two words to the end)
    assert merge(key_word=i32(1, 2, 4), key_type=i32(pc.T_DATE, pc.T_VARCHAR, pc.T_BOOL), key_len=i32(0, 9, 0)) == UNSUPPORTED
    assert merge(key_type=i32(pc.T_DECIMAL, pc.T_CHAR, pc.T_CHAR), key_len=i32(0, 12, 1)) == UNSUPPORTED
    assert merge(n=0) == UNSUPPORTED and merge(n_keys=0, n_acc=0) == UNSUPPORTED
    many = np.ones(40, dtype=np.int32)
    for kw in (dict(rows=None), dict(out_rows=None), dict(out_count=None), dict(notes=None), dict(n=-1), dict(n=1 << 31),
               dict(stride=0), dict(stride=-8), dict(n_tab=-1), dict(n_tab=8),
               dict(key_word=None), dict(key_type=None), dict(key_len=None), dict(acc_word=None), dict(acc_kind=None),
               dict(n_keys=-1), dict(n_keys=17, key_word=many, key_type=many * pc.T_BIGINT, key_len=many * 0, n_tab=7, n_acc=0),
               dict(n_acc=-1), dict(n_acc=33, acc_word=many * 5, acc_kind=many * 0),
               dict(key_word=i32(0, 2, 4)),                 # the first-row word is no key
               dict(key_word=i32(5, 2, 4)),                 # a key among the accumulators
               dict(key_word=i32(1, 4, 4)),                 # CHAR(12) from word 4: its second word is an accumulator
               dict(key_len=i32(0, 25, 0)),                 # four words from word 2: one behind the table words
               dict(key_len=i32(0, -1, 0)), dict(key_len=i32(0, 0, 0)),          # a string has a length
               dict(key_len=i32(8, 12, 0)),                 # a number has none
               dict(key_type=i32(pc.T_BIGINT, pc.T_CHAR, 6)), dict(key_type=i32(8, pc.T_CHAR, pc.T_INT)), dict(key_type=i32(-1, pc.T_CHAR, pc.T_INT)),
               dict(key_type=i32(pc.T_BIGINT, pc.T_CHAR, 99)),
               dict(acc_word=i32(4, 6, 7)),                 # a table word
               dict(acc_word=i32(5, 6, 8)),                 # behind the row
               dict(acc_word=i32(0, 6, 7)), dict(acc_word=i32(-1, 6, 7)),
               dict(acc_kind=i32(1, 2, 3)), dict(acc_kind=i32(0, 2, 4)), dict(acc_kind=i32(0, -1, 3))):
        assert merge(**kw) == INVALID, kw
    assert ctx._L.rsq_prim_merge_group_rows(None, *[p(good[k]) if isinstance(good[k], np.ndarray) else good[k] for k in order]) == INVALID
    with pytest.raises(engine.EngineError) as e:
        ctx.prim_merge_group_rows(rows, 4, [(1, pc.T_BIGINT, 0)], [(5, 0)])
    assert e.value.status == UNSUPPORTED

    # ---- top-k ----
    rows, cand, count, rng2 = np.zeros((6, 3), np.int64), np.zeros((4, 3), np.int64), C.c_uint32(0), np.zeros(2, np.uint64)
    order = ("rows", "n_rows", "bound", "stride", "key_word", "is32", "desc", "want", "form", "range", "capacity", "cand", "count", "notes")
    topk = lambda **kw: _call(ctx, "rsq_prim_topk_select", *pick(dict(rows=p(rows), n_rows=6, bound=6, stride=3, key_word=1, is32=0, desc=1, want=2, form=0,
                                                                      range=p(rng2), capacity=4, cand=p(cand), count=C.addressof(count), notes=pn), order, kw))
    assert topk() == UNSUPPORTED and notes.value == 0
    assert topk(form=1) == UNSUPPORTED and topk(form=0, range=None) == UNSUPPORTED and topk(key_word=0) == UNSUPPORTED and topk(key_word=2) == UNSUPPORTED
    assert topk(bound=0) == UNSUPPORTED and topk(bound=1 << 31) == UNSUPPORTED and topk(want=7) == UNSUPPORTED and topk(n_rows=0) == UNSUPPORTED
    for kw in (dict(rows=None), dict(cand=None), dict(count=None), dict(notes=None), dict(form=1, range=None), dict(n_rows=-1), dict(n_rows=(1 << 31) + 1),
               dict(bound=-1), dict(bound=(1 << 31) + 1), dict(want=0), dict(want=-3), dict(want=1 << 32), dict(capacity=0), dict(capacity=-1),
               dict(stride=0), dict(stride=-3), dict(stride=65), dict(key_word=-1), dict(key_word=3), dict(form=2), dict(form=-1)):
        assert topk(**kw) == INVALID, kw
    assert ctx._L.rsq_prim_topk_select(None, p(rows), 6, 6, 3, 1, 0, 1, 2, 0, p(rng2), 4, p(cand), C.addressof(count), pn) == INVALID
    with pytest.raises(engine.EngineError) as e:
        ctx.prim_topk_select(rows, 1, False, True, 2, 0, 4)
    assert e.value.status == UNSUPPORTED
