"""The offset scan, the rank index and the placement kernels (aot_kernels.hip) on the test's own data, through rsq_prim_*
(include/resql_hip.h): sizes that put a kernel's own boundaries inside the run and exact references (tests/primcases.py, proven against
plain loops by tests/test_primitives_host.py).  Every comparison is equality; every case expects no bit of the device error word - a
look-back that timed out is a failure here, nothing is repeated - except the two placement cases whose bit the code documents.
The same for the kernels that finish an aggregation: the radix sort and the running minimum of the device tail, the merge of several
shards' group rows (devtail.hip) and the ORDER BY ... LIMIT pre-selection (aot_kernels.hip)."""
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


# ---- radix sort of the device tail ----
@pytest.mark.parametrize("n,key_bits,pattern,vals_kind", pc.sort_cases())
def test_pairs_are_sorted_stably_by_whole_digits(gpu_ctx, n, key_bits, pattern, vals_kind):
    keys, vals = pc.sort_keys(n, key_bits, pattern), pc.sort_vals(n, vals_kind)
    want_keys, want_vals = pc.sort_reference(keys, vals, key_bits)
    got_keys, got_vals, notes = gpu_ctx.prim_radix_sort_pairs(keys, vals, key_bits)
    _no_notes(notes, f"sort of {n} pairs by {key_bits} bits, {pattern}")
    assert np.array_equal(got_keys, want_keys), f"keys: {_first_difference(got_keys, want_keys)}"
    assert np.array_equal(got_vals, want_vals), f"values: {_first_difference(got_vals, want_vals)}"


# ---- running minimum of the replay ----
@pytest.mark.parametrize("n,pattern,at", pc.runmin_cases())
def test_running_minimum(gpu_ctx, n, pattern, at):
    v = pc.runmin_values(n, pattern, at=at)
    want = pc.runmin_reference(v)
    got, notes = gpu_ctx.prim_running_min(v)
    _no_notes(notes, f"running minimum of {n} values, {pattern}")
    assert np.array_equal(got, want), _first_difference(got, want)


# ---- merge of several shards' group rows ----
@pytest.mark.parametrize("n,grouping,keyset,accset", pc.merge_cases())
def test_group_rows_merge_by_normalised_key(gpu_ctx, n, grouping, keyset, accset):
    case = pc.MergeCase(n, grouping, keyset, accset)
    want = pc.merge_reference(case.rows, case.n_tab, case.keys, case.accs)
    got, notes = gpu_ctx.prim_merge_group_rows(case.rows, case.n_tab, case.keys, case.accs)
    _no_notes(notes, f"merge of {n} rows, {grouping}, {keyset}, {accset}")
    assert len(got) == len(want), f"{len(got)} groups, want {len(want)}"
    got = got[np.argsort(got[:, 0], kind="stable")]          # (a group's position follows whichever member claimed its slot)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, f"{len(bad)} groups differ, first {int(bad[0])}: got {got[bad[0]].tolist()}, want {want[bad[0]].tolist()}"


# ---- ORDER BY ... LIMIT pre-selection ----
def _candidates(case, cand, count, members, what):
    """`count` is the size of the reference's set; the first min(count, capacity) rows of `cand` are distinct members of it, copied
    whole; the rows behind them were not written.  Returns the row indices."""
    assert count == len(members), f"{what}: {count} candidates, want {len(members)}"
    assert (len(members) > case.capacity) == case.overflow
    n = min(count, case.capacity)
    ids = cand[:n, case.id_word] - pc.TOPK_ID_BASE
    idx = ids // pc.TOPK_ID_STEP
    assert (ids % pc.TOPK_ID_STEP == 0).all() and (idx >= 0).all() and (idx < case.n).all(), f"{what}: a candidate is no row"
    assert np.array_equal(cand[:n], case.rows[idx]), f"{what}: a candidate row is not a copy of its row"
    assert len(np.unique(idx)) == n, f"{what}: a row was taken twice"
    assert np.isin(idx, members).all(), f"{what}: first stray row {int(idx[~np.isin(idx, members)][0])}"
    assert (cand[n:] == -1).all(), f"{what}: rows behind the candidates were written"
    return idx


_TOPK_CASES = pc.topk_cases()


@pytest.mark.parametrize("case", _TOPK_CASES, ids=[c.name() for c in _TOPK_CASES])
def test_top_candidates_in_both_forms(gpu_ctx, case):
    images = case.images()
    exact = pc.topk_reference(images, case.want)
    select = lambda form, rng2=None: gpu_ctx.prim_topk_select(case.rows, case.key_word, case.is32, case.desc, case.want, form, case.capacity,
                                                              rows_upper_bound=case.rows_upper_bound, image_range=rng2)
    cand, count, notes = select(0)
    _no_notes(notes, f"exact selection, {case.name()}")
    _candidates(case, cand, count, exact, "exact selection")
    rng2 = pc.topk_exact_range(images)
    for what, r in (("range selection", rng2), ("range selection over a wider range", pc.topk_wider_range(rng2))):
        members = pc.topk_range_reference(images, case.want, r)
        assert np.isin(exact, members).all()          # the property the engine relies on: a superset of the exact selection
        cand, count, notes = select(1, r)
        _no_notes(notes, f"{what}, {case.name()}")
        _candidates(case, cand, count, members, what)
