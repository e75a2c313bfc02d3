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
    assert int(re.search(r"^#define SCAN_CHUNK (\d+)", aot, re.M).group(1)) == pc.SCAN_CHUNK
    assert f"(i64)sb * {pc.SCAN_BATCH} " in aot and f"base += {pc.SCAN_BATCH})" in aot
    assert pc.SCAN_CHUNK == 4 * pc.SCAN_BATCH          # four sub-blocks per chunk
    eng = open(os.path.join(SRC, "engine.h")).read()
    assert int(re.search(r"^#define RSQ_RANK_CHUNK_BLOCKS (\d+)", eng, re.M).group(1)) == pc.RANK_CHUNK_BLOCKS == engine.RANK_CHUNK_BLOCKS


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
