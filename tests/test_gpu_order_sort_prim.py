"""The device's order of column-wise rows and the gather of their tuples (resql_amd/csrc/order_sort.hip) through rsq_prim_sort_rows and
rsq_prim_gather_tuples, against numpy - never against the engine.

The order is held against numpy.lexsort over the keys' images (tests/ordersortcases.py image): lexsort is stable, so with ties it is
exactly the device's "keys, then scan order".  The tied-pair count among the leading `lead` rows, the bits per key and the words are numpy
restatements.  Row counts sit on both sides of a wave, a workgroup and a radix tile (2048 pairs), and 70 001 rows take 35 tiles.

The gather is held byte for byte: the device buffer is filled with 0xEE before the launch and carries 64 guard bytes behind the tuples. A
workgroup stages R = min(256, 48 KiB / tuple size) output rows in LDS; tuple sizes that are and are not multiples of 4 take the word and
the byte loads, spans start at every alignment, and one tuple is longer than the tile (R = 0: global to global)."""
import numpy as np
import pytest

from resql_amd import plan as P

import ordersortcases as S

pytestmark = pytest.mark.gpu
T = P.TypeInit
TILE = 49152          # order_sort.hip OS_TILE_BYTES
GUARD = 64
ROWS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097, 70_001]          # 2048: devtail.hip RS_TILE


def scrambled(n, mul, mod):
    """n values below mod in scrambled order, as int64"""
    return ((np.arange(n, dtype=np.uint64) * np.uint64(mul) + np.uint64(12345)) % np.uint64(mod)).astype(np.int64)


def with_ends(values, lo, hi):
    """the type's two ends among the values, away from the array's own ends"""
    if len(values) > 4:
        values[len(values) // 3] = lo
        values[len(values) // 2] = hi
    return values


def int_key(n, mul=2654435761, mod=1 << 40):
    return with_ends((scrambled(n, mul, mod) - (mod >> 1)).astype(np.int32), S.I32_MIN, S.I32_MAX)


def big_key(n, mul=0x9E3779B97F4A7C15):
    v = (np.arange(n, dtype=np.uint64) * np.uint64(mul) + np.uint64(77)).view(np.int64).copy()
    return with_ends(v, S.I64_MIN, S.I64_MAX)


def date_key(n):
    """DATEs, a few of them at and above 2^31: they sort as negative numbers"""
    d = (19920101 + scrambled(n, 40503, 3000)).astype(np.uint32)
    late = np.flatnonzero(np.arange(n) % 7 == 3)
    d[late] = (0x80000000 + late % 5).astype(np.uint32)
    return d


def held_against_lexsort(ctx, columns, types, key_columns, descending, lead=None):
    n = len(columns[0])
    lead = n if lead is None else lead
    keys = [columns[c].view(np.int32) if columns[c].dtype == np.uint32 else columns[c] for c in key_columns]
    want_perm, want_tied, want_bits, want_words = S.expected_order(keys, descending, lead)
    perm, tied, bits, words = ctx.prim_sort_rows(columns, types, key_columns, descending, lead)
    assert (bits, words) == (want_bits, want_words)
    assert np.array_equal(perm, want_perm), "first difference at %d" % int(np.flatnonzero(perm != want_perm)[0])
    assert tied == want_tied
    return perm, tied, bits, words


ONE_KEY = {"int": (T.INT(), int_key), "date": (T.DATE(), date_key), "bigint": (T.BIGINT(), big_key), "decimal": (T.DECIMAL(15, 2), big_key)}


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("kind", sorted(ONE_KEY))
@pytest.mark.parametrize("desc", [False, True], ids=["asc", "desc"])
def test_one_key_of_each_width_in_each_direction(gpu_ctx, kind, desc, n):
    t, make = ONE_KEY[kind]
    key = make(n)
    if n > 4 and kind != "date":          # the type's ends are among the values
        assert key.min() == (S.I32_MIN if t.width == 4 else S.I64_MIN) and key.max() == (S.I32_MAX if t.width == 4 else S.I64_MAX)
    held_against_lexsort(gpu_ctx, [key], [t], [0], [desc])


@pytest.mark.parametrize("n", ROWS)
def test_several_keys_with_ties_and_a_payload_column_between(gpu_ctx, n):
    """a DATE of few values descending, a constant key, an INT of few values: ties on all three remain, and the order among them is the
    scan order; the VARCHAR column between the keys is not the sort's business"""
    cols = [date_key(n), np.zeros(n, dtype="S7"), np.full(n, -5, dtype=np.int64), (scrambled(n, 2246822519, 11) - 5).astype(np.int32)]
    types = [T.DATE(), T.VARCHAR(7), T.BIGINT(), T.INT()]
    _, tied, bits, _ = held_against_lexsort(gpu_ctx, cols, types, [0, 2, 3], [True, False, False])
    assert bits[1] == 0 and (n < 70_001 or tied > 0)


def test_all_keys_constant(gpu_ctx):
    """no key varies: no bits, no word, nothing is sorted - every leading pair ties, and with lead 1 none does"""
    for n, lead in ((1, 1), (2, 2), (300, 300), (300, 1), (300, 0), (4097, 17)):
        cols = [np.full(n, S.I32_MIN, dtype=np.int32), np.full(n, S.I64_MAX, dtype=np.int64)]
        perm, tied, bits, words = held_against_lexsort(gpu_ctx, cols, [T.INT(), T.BIGINT()], [0, 1], [False, True], lead)
        assert bits == [0] * 8 and words == 0 and tied == max(lead - 1, 0) and np.array_equal(perm, np.arange(n, dtype=np.uint32))


@pytest.mark.parametrize("n", [257, 4097])
@pytest.mark.parametrize("total", [64, 65, 192])
def test_composites_at_the_word_boundaries(gpu_ctx, total, n):
    """exactly 64 bits: two keys of 32; 65: the first key takes 33 and straddles the boundary; 192: three full-range BIGINTs"""
    if total == 192:
        cols = [big_key(n, m) for m in (0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9)]
        cols[0] = (cols[0] >> np.int64(62)) << np.int64(62)          # (few values in front, so that the later words decide)
        cols[0] = with_ends(cols[0], S.I64_MIN, S.I64_MAX)
        types, desc = [T.BIGINT(), T.DECIMAL(15, 2), T.BIGINT()], [False, True, False]
    else:
        first = (scrambled(n, 2654435761, 7) * ((1 << (total - 32)) - 1) // 6).astype(np.int64)          # 0 .. 2^(total - 32) - 1, both ends present
        second = with_ends(int_key(n, 40503), S.I32_MIN, S.I32_MAX)
        cols, types, desc = [first, second], [T.BIGINT(), T.INT()], [True, False]
    _, _, bits, words = held_against_lexsort(gpu_ctx, cols, types, list(range(len(cols))), desc)
    assert sum(bits) == total and words == (total + 63) // 64


@pytest.mark.parametrize("n", [65, 2049, 70_001])
def test_eight_keys(gpu_ctx, n):
    cols = [(scrambled(n, 2654435761 + 2 * k, 5 + k) - 3).astype(np.int32 if k % 2 else np.int64) for k in range(7)] + [S.O.unique_ints(n)]
    types = [T.INT() if k % 2 else T.BIGINT() for k in range(7)] + [T.INT()]
    _, tied, _, _ = held_against_lexsort(gpu_ctx, cols, types, list(range(8)), [k % 3 == 0 for k in range(8)])
    assert tied == 0          # (the last key is unique)
    with pytest.raises(Exception):
        gpu_ctx.prim_sort_rows(cols + [cols[0]], types + [types[0]], list(range(9)), [False] * 9)


@pytest.mark.parametrize("n", [300, 4097])
def test_lead_bounds_the_tie_count(gpu_ctx, n):
    """key = row // 2 scrambled into pairs: sorted, positions (2 j, 2 j + 1) tie and (2 j + 1, 2 j + 2) do not.  A lead that puts a tied
    pair at (lead - 2, lead - 1) counts it; one that puts it at (lead - 1, lead) does not"""
    order = np.argsort(scrambled(n, 2654435761, 1 << 30), kind="stable")
    key = np.empty(n, dtype=np.int32)
    key[order] = np.arange(n, dtype=np.int32) // 2
    for lead, want in ((0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (100, 50), (101, 50), (n, n // 2)):
        _, tied, _, _ = held_against_lexsort(gpu_ctx, [key], [T.INT()], [0], [False], lead)
        assert tied == want, lead


# ---- the gather --------------------------------------------------------------------------------------------------------------------

TUPLE_SIZES = [4, 5, 34, 60, 64, 204, 309, 50_005]


def group_rows(ts):
    return min(256, TILE // ts) if ts <= TILE else 0


def row_counts(ts):
    R = group_rows(ts)
    return sorted({n for n in (1, R - 1, R, R + 1, 2 * R + 1, 1000) if n > 0}) if R else [1, 3, 1000]


def permutation(kind, n):
    if kind == "identity":
        return np.arange(n, dtype=np.uint32)
    if kind == "reversed":
        return np.arange(n, dtype=np.uint32)[::-1].copy()
    return np.argsort(scrambled(n, 2654435761, 1 << 30), kind="stable").astype(np.uint32)


GATHER = [(ts, n) for ts in TUPLE_SIZES for n in row_counts(ts)]


def test_the_tuple_sizes_tile_as_described():
    assert [group_rows(ts) for ts in TUPLE_SIZES] == [256, 256, 256, 256, 256, 240, 159, 0]


@pytest.mark.parametrize("ts,n", GATHER, ids=["%d-%d" % c for c in GATHER])
def test_every_byte_of_the_gathered_tuples(gpu_ctx, ts, n):
    if ts * n > (8 << 20):          # (the long tuple: a stride of the byte values, made without a multiplication of that size)
        tuples = np.resize(np.arange(251, dtype=np.uint8), n * ts).reshape(n, ts).copy()
    else:
        tuples = ((np.arange(n * ts, dtype=np.uint64) * np.uint64(2654435761) >> np.uint64(9)) % np.uint64(251)).astype(np.uint8).reshape(n, ts)
    tuples[:, 0] = np.arange(n) % 256          # (rows differ in their first bytes whatever the pattern's period)
    tuples[:, ts - 1] = (np.arange(n) // 256) % 256
    for kind in ("identity", "reversed", "scrambled"):
        perm = permutation(kind, n)
        for n_out in sorted({0, 1, n - 1, n}):
            got = gpu_ctx.prim_gather_tuples(tuples, ts, perm, n_out)
            assert got.shape == (n_out * ts + GUARD,)
            want = tuples[perm[:n_out]]
            out = got[:n_out * ts].reshape(n_out, ts)
            wrong = np.flatnonzero((out != want).any(axis=1))
            assert len(wrong) == 0, "%s, n_out %d: rows %s differ" % (kind, n_out, wrong[:8])
            assert (got[n_out * ts:] == 0xEE).all(), "%s, n_out %d: a byte behind the last tuple was written" % (kind, n_out)
