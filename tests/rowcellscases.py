"""Statements and tables for the register aggregation's second form, rows into per-lane LDS cells (tests/test_row_cells_codegen.py,
tests/test_gpu_row_cells.py): sums of small non-negative columns that share a word, a sum of a signed column that does not, min and max."""
import os
import sys

import numpy as np

from resql_amd import plan as P

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import narrowcases as N  # noqa: E402

T = P.TypeInit

# sum(a): 8 bits, never negative; sum(d): 4 bits; the count: the three share a word.  sum(s): small but signed, a word of its own.
PACKED = N.Statement([("sum", "a"), ("sum", "s"), ("count", None), ("sum", "d"), ("min", "c"), ("max", "c")], ["g"])
ROWS = [0, 1, 127, 128, 129, 4 * N.TILE + 77]          # one workgroup: a 512-thread workgroup takes 8 tiles, and these have at most 4
# two workgroups (RSQ_MAX_GRID=4: two 512-thread workgroups at the most): the fewest tiles that ask for a second one, with one tail row; and
# two tiles a wave with 77 tail rows, which the grid's 1024 threads deal out round-robin
ROWS_TWO_WORKGROUPS = [9 * N.TILE + 1, 16 * 2 * N.TILE + 77]
FIELD_TOP = 255
# one 512-thread workgroup (RSQ_MAX_GRID=1): 8 waves x 2 rows x tiles per wave x 255 stays below 2^21 up to 514 tiles a wave
EDGE_INSIDE = 8 * 514 * N.TILE
EDGE_PAST = EDGE_INSIDE + N.TILE
# ... and two of them (RSQ_MAX_GRID=4): 16 waves, the same 514 tiles a wave
EDGE_INSIDE_TWO = 16 * 514 * N.TILE
EDGE_PAST_TWO = EDGE_INSIDE_TWO + N.TILE


def packed_table(n, seed=23):
    """g: groups 0..5 - group 5 in row 0 only, group 0 in the last row only (a tail row unless n is a multiple of 128), group 3 never,
    1 / 2 / 4 share the rest; a: 0..255 with both ends present; d: 0..10; s: -100..100; c: the 24-bit envelope, both signs"""
    rng = np.random.default_rng(seed)
    g = rng.choice(np.array([1, 2, 4], dtype=np.int64), n)
    a = rng.integers(0, FIELD_TOP + 1, n).astype(np.int64)
    d = rng.integers(0, 11, n).astype(np.int64)
    s = rng.integers(-100, 101, n).astype(np.int64)
    c = rng.integers(-N.P32_MAX, N.P32_MAX + 1, n).astype(np.int64)
    if n:
        g[0], g[n - 1] = 5, 0
    if n > 4:
        a[1], a[2], s[1], s[2], d[1], d[2] = 0, FIELD_TOP, -100, 100, 0, 10
    return P.Table("t", [P.Column("g", T.BIGINT(), g), P.Column("a", T.BIGINT(), a), P.Column("d", T.BIGINT(), d),
                         P.Column("s", T.BIGINT(), s), P.Column("c", T.BIGINT(), c)], n)


def one_group_table(n):
    """every row in group 1 of 0..2 (rows 0 and 1 open the domain), a at 255 in every row of it: the fields at their largest"""
    g = np.ones(n, dtype=np.int64)
    a = np.full(n, FIELD_TOP, dtype=np.int64)
    g[0], g[1] = 0, 2
    a[0], a[1] = 0, 0
    d = np.full(n, 10, dtype=np.int64)
    s = np.full(n, -100, dtype=np.int64)
    c = np.arange(n, dtype=np.int64) % 1000 - 500
    return P.Table("t", [P.Column("g", T.BIGINT(), g), P.Column("a", T.BIGINT(), a), P.Column("d", T.BIGINT(), d),
                         P.Column("s", T.BIGINT(), s), P.Column("c", T.BIGINT(), c)], n)


def one_group_reference(n):
    """PACKED over one_group_table(n), in closed form"""
    m = n - 2
    c = np.arange(n, dtype=np.int64) % 1000 - 500
    return sorted([(0, 0, -100, 1, 10, int(c[0]), int(c[0])), (2, 0, -100, 1, 10, int(c[1]), int(c[1])),
                   (1, FIELD_TOP * m, -100 * m, m, 10 * m, int(c[2:].min()), int(c[2:].max()))])
