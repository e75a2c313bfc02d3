"""The device selection of ORDER BY ... LIMIT over a materialisation (resql_amd/csrc/order_limit.hip) through rsq_prim_column_topk, against
numpy: T is the want-th largest image of the key column, the candidates are flatnonzero(image >= T) - in scan order, so positions and
payload rows compare as arrays - and the count is exact whatever the capacity.  Sizes sit on both sides of a wave (64), a workgroup's
256-row block and the scan's 4096-count chunk (66 000 rows are 258 blocks; the scan takes blocks + 1 counts); the keys hold the ends of
their types."""
import numpy as np
import pytest

from resql_amd import engine

import orderlimitcases as O

pytestmark = pytest.mark.gpu
FILL32 = 0xffffffff


def keys_of(n, dtype, seed=0):
    """scrambled keys with duplicates (about four rows a value) and the ends of the type among them"""
    lo, hi = (O.I32_MIN, O.I32_MAX) if dtype == np.int32 else (O.I64_MIN, O.I64_MAX)
    h = O.scramble(n, 2654435761 + 2 * seed, 3).astype(np.int64)
    k = ((h % max(1, n // 4)) * 7919 - 3 * n).astype(np.int64)
    if dtype == np.int64:
        k = k * 1_000_003_007
    edges = [lo, -1, 0, hi, lo + 1, hi - 1, hi, lo]
    for i, v in enumerate(edges):          # (scattered: row 0, the last row, rows on both sides of a block edge where there is one)
        k[(i * 97 + (n - 1) * (i & 1)) % n] = v
    return k.astype(dtype)


def payload_of(n, width):
    return ((np.arange(n * width, dtype=np.uint64) * np.uint64(2654435761) >> np.uint64(13)) % np.uint64(251)).astype(np.uint8).reshape(n, width)


def check(ctx, key, desc, want, capacity, payload):
    T, where = O.expected_selection(key, desc, want)
    pos, out, count, threshold, notes = ctx.prim_column_topk(key, desc, want, capacity, payload)
    assert notes == 0
    assert threshold == T, (len(key), want, desc)
    assert count == len(where), (len(key), want, desc)
    kept = min(count, capacity)
    assert np.array_equal(pos[:kept], where[:kept])
    assert np.array_equal(out[:kept], payload[where[:kept]])
    assert (pos[kept:] == FILL32).all() and (out[kept:] == 0xff).all()          # nothing behind the candidates was written
    return count


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000, 66_000])
def test_sizes_wants_widths_and_directions(gpu_ctx, n):
    payload = payload_of(n, 25)
    for dtype in (np.int32, np.int64):
        key = keys_of(n, dtype)
        for desc in (False, True):
            for want in sorted({1, 2, n, n + 1}):
                count = check(gpu_ctx, key, desc, want, n + 3, payload)
                assert count >= min(want, n)
                if want > n:
                    assert count == n          # fewer rows than wanted: every row is a candidate, T = 0


def test_all_candidates_inside_the_last_partial_block(gpu_ctx):
    n = 1000          # blocks of 256 rows: the last one holds rows 768..999
    key = (O.scramble(n) % np.uint64(500)).astype(np.int64)
    key[[990, 771, 999, 800, 768]] = [10_000, 10_001, 10_002, 10_003, 10_004]
    assert check(gpu_ctx, key, True, 5, 64, payload_of(n, 8)) == 5
    assert check(gpu_ctx, (-key).astype(np.int32), False, 5, 64, payload_of(n, 8)) == 5


def test_one_candidate_per_block(gpu_ctx):
    blocks = 41
    n = 256 * (blocks - 1) + 17
    key = (O.scramble(n) % np.uint64(1000)).astype(np.int32)
    for b in range(blocks):          # one leading value a block, at a lane that moves through the waves (the last block has 17 rows)
        key[256 * b + (b * 37) % (17 if b == blocks - 1 else 256)] = 5000 + ((b * 29) % blocks)
    assert check(gpu_ctx, key, True, blocks, blocks, payload_of(n, 4)) == blocks


def test_every_row_a_candidate(gpu_ctx):
    n = 66_000
    for key in (np.full(n, -7, dtype=np.int32), np.full(n, O.I64_MIN, dtype=np.int64)):
        for desc in (False, True):
            assert check(gpu_ctx, key, desc, 1, n, payload_of(n, 4)) == n


@pytest.mark.parametrize("width", [1, 4, 8, 25, 40])
def test_payload_widths(gpu_ctx, width):
    n = 1000
    assert check(gpu_ctx, keys_of(n, np.int64, seed=width), True, 10, 100, payload_of(n, width)) >= 10


@pytest.mark.parametrize("extra", [0, 1])
def test_a_tie_group_at_the_threshold_of_capacity_rows_and_one_more(gpu_ctx, extra):
    """want = 1 and `capacity + extra` rows share the leading value: with extra = 0 nothing is dropped; with one more the count is still
    exact and the first `capacity` candidates are the first in scan order"""
    n, capacity = 5000, 300
    key = (O.scramble(n) % np.uint64(900)).astype(np.int64)
    tied = np.sort(np.argsort(O.scramble(n, 40503, 0), kind="stable")[: capacity + extra])          # scattered over the blocks
    assert len(set(tied.tolist())) == capacity + extra
    key[tied] = 1_000_000
    payload = payload_of(n, 25)
    pos, out, count, threshold, notes = gpu_ctx.prim_column_topk(key, True, 1, capacity, payload)
    assert notes == 0 and count == capacity + extra and threshold == int(O.image(np.array([1_000_000]), True)[0])
    assert np.array_equal(pos, tied[:capacity].astype(np.uint32))
    assert np.array_equal(out, payload[tied[:capacity]])
    check(gpu_ctx, key, True, 1, capacity, payload)
    if extra:          # one row of capacity more, and the row that did not fit is the last in scan order
        pos2, out2, count2, _, _ = gpu_ctx.prim_column_topk(key, True, 1, capacity + 1, payload)
        assert count2 == capacity + 1 and np.array_equal(pos2, tied.astype(np.uint32)) and np.array_equal(out2, payload[tied])
