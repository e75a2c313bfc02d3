"""The offset scan, the rank index and the placement kernels (aot_kernels.hip) on the test's own data, through rsq_prim_*
(include/resql_hip.h): sizes that put a kernel's own boundaries inside the run and exact references (tests/primcases.py, proven against
plain loops by tests/test_primitives_host.py).  Every comparison is equality; every case expects no bit of the device error word - a
look-back that timed out is a failure here, nothing is repeated - except the two placement cases whose bit the code documents."""
import numpy as np
import pytest

import primcases as pc

pytestmark = pytest.mark.gpu


def _no_notes(notes, what):
    assert notes == 0, f"{what}: device error bits raised - {pc.notes_text(notes)}"


def _first_difference(got, want):
    bad = np.flatnonzero(got != want)
    return f"{len(bad)} differ, first at {int(bad[0])}: got {int(got[bad[0]])}, want {int(want[bad[0]])}" if len(bad) else "equal"


# ---- scan ----
@pytest.mark.parametrize("pattern", pc.SCAN_PATTERNS)
@pytest.mark.parametrize("n", pc.SCAN_SIZES)
def test_scan_offsets_in_both_forms(gpu_ctx, n, pattern):
    counts = pc.scan_counts(n, pattern)
    want = pc.scan_reference(counts)
    got = []
    for form in (0, 1):
        offs, notes = gpu_ctx.prim_scan(counts, form)
        _no_notes(notes, f"scan form {form}, n={n}, {pattern}")
        assert np.array_equal(offs, want), f"form {form}: {_first_difference(offs, want)}"
        got.append(offs)
    assert np.array_equal(got[0], got[1])


# ---- rank index ----
@pytest.mark.parametrize("density", pc.RANK_DENSITIES)
@pytest.mark.parametrize("n_blocks", pc.RANK_BLOCKS)
def test_rank_index_in_both_forms(gpu_ctx, n_blocks, density):
    blocks = pc.rank_blocks(n_blocks, density)
    rank, chunk_base = pc.rank_reference(blocks)
    for form in (0, 1):
        out, base, notes = gpu_ctx.prim_rank_index(blocks, form)
        _no_notes(notes, f"rank index form {form}, {n_blocks} blocks, {density}")
        assert np.array_equal(out[:, 1:], blocks[:, 1:]), f"form {form}: bitmap words changed"
        assert np.array_equal(out[:, 0], rank), f"form {form}: {_first_difference(out[:, 0], rank)}"
        assert np.array_equal(base, chunk_base), f"form {form}: {_first_difference(base, chunk_base)}"


# ---- placement ----
def _place(ctx, case):
    return ctx.prim_rank_place(case.blocks(), case.bm_min, case.bm_bits, case.records(), case.used, case.region, case.n_words, case.capacity)


_PLACE_CASES = pc.place_cases()


@pytest.mark.parametrize("case", [c for _, c in _PLACE_CASES], ids=[i for i, _ in _PLACE_CASES])
def test_records_land_at_the_rank_of_their_key(gpu_ctx, case):
    want, n = case.expected()
    assert n == int(case.used.sum())
    got, notes = _place(gpu_ctx, case)
    _no_notes(notes, f"placement of {n} records of {case.n_words} words in {case.n_waves} regions")
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, f"{len(bad)} entries differ, first {int(bad[0])}: got {got[bad[0]].tolist()}, want {want[bad[0]].tolist()}"
    assert (got[n:] == -1).all()          # entries nobody wrote are still 0xff bytes


@pytest.mark.parametrize("n_words", [2, 8, 9])
def test_a_key_that_occurs_twice_raises_bit_64_and_stays_inside_the_entries(gpu_ctx, n_words):
    """k_rank_place: "as many records as distinct keys ... anything else means the build side changed" - bit 64, on which the engine falls
    back to the hash table.  Both records go to the one rank their key has; the ranks behind the distinct keys stay unwritten (the
    entry array itself is all the call can see of "nothing outside")."""
    case = pc.PlaceCase(n_words, 3, used_shift=2, seed=5)          # used 255, 256, 257
    first, second = 100, 600                                        # (records of two different regions)
    case.rec[second, 0] = case.rec[first, 0]
    want, distinct = case.expected()
    assert distinct == len(case.rec) - 1
    got, notes = _place(gpu_ctx, case)
    assert notes == pc.NOTE_PLACE_COUNT, pc.notes_text(notes)
    r = int(np.searchsorted(np.unique(case.rec[:, 0]), case.rec[first, 0]))
    assert got[r].tolist() in (case.rec[first].tolist(), case.rec[second].tolist())
    others = np.arange(case.capacity) != r
    assert np.array_equal(got[others], want[others])
    assert (got[distinct:] == -1).all()
    # the context is usable and clean afterwards: the bit does not come back with the next call
    again, notes = _place(gpu_ctx, pc.PlaceCase(n_words, 1, used_shift=1))
    _no_notes(notes, "placement after a call that raised bit 64")


@pytest.mark.parametrize("n_words,where", [(1, "below"), (4, "above"), (5, "below"), (12, "above")])
def test_a_key_outside_the_domain_is_skipped(gpu_ctx, n_words, where):
    """k_rank_place: "a key outside the bitmap's domain: the build kernel has raised ERR_GROUP_OVERFLOW for it" - the record is skipped, the
    others are placed.  The record counter then exceeds the distinct keys of the bitmap by one, which is bit 64 as the kernel documents
    it: asserted, not tolerated."""
    case = pc.PlaceCase(n_words, 3, used_shift=5, seed=6)          # used 511, 512, 513
    case.rec[700, 0] = case.bm_min - 1 if where == "below" else case.bm_min + case.bm_bits
    want, distinct = case.expected()
    assert distinct == len(case.rec) - 1
    got, notes = _place(gpu_ctx, case)
    assert notes == pc.NOTE_PLACE_COUNT, pc.notes_text(notes)
    assert np.array_equal(got, want)
    assert (got[distinct:] == -1).all()
