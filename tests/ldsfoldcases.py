"""Tables and statements for tests/test_lds_fold_codegen.py and tests/test_gpu_lds_fold.py: the register aggregation's 32-bit partial
sums folded into the workgroup's LDS image s_lane (codegen_agg.cpp) and its launch as two workgroups per CU (codegen_loop.cpp).  The
fold tables, their closed-form reference and the plan builder are tests/narrowcases.py's; this file adds the tile counts around the
fold period from no tile on, a min and a max next to two partial sums over groups seen once, never, and in the last tail row only,
and a statement at the register form's limit of 64 cells."""
import os
import sys

import numpy as np

from resql_amd import plan as P

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import narrowcases as N  # noqa: E402

T = P.TypeInit

FOLD_TILES = [0, 1, 31, 32, 33, 64, 65]                 # whole tiles per wave: none, one, around one fold period, around two
FOLD_TAILS = [0, 1, 77]
FOLD_KINDS = ["pos", "neg"]                             # (a negative partial sum must be sign-extended into the 64-bit cell)
GRID_WAVES = {"1": 8, "4": 16}                          # RSQ_MAX_GRID -> waves of the launch: one 512-thread workgroup, two
SMALL_N = [0, 1, 127]

MINMAX = N.Statement([("sum", "c"), ("count", None), ("min", "c"), ("max", "c")], ["g"])
MINMAX_N = 8 * 33 * N.TILE + 77                         # one workgroup (RSQ_MAX_GRID=1): every wave folds once in the loop, then tail rows
CELLS64 = N.Statement([("sum", "c"), ("count", None), ("min", "c")], ["b"])      # 16 groups x (first row + 3) = 64 cells
CELLS64_N = 8 * 3 * N.TILE + 77


def minmax_table(n, seed=17):
    """g: six dense groups 0..5 - group 5's only row is row 0 (the first-row tracker's), group 0's only row is the last row (a tail row
    unless n is a multiple of 128), group 3 is never seen, 1 / 2 / 4 share the rest; c: +-(2^24 - 1) and values between"""
    rng = np.random.default_rng(seed)
    g = rng.choice(np.array([1, 2, 4], dtype=np.int64), n)
    c = rng.integers(-N.P32_MAX, N.P32_MAX + 1, n).astype(np.int64)
    if n:
        g[0], c[0] = 5, N.P32_MAX
        g[n - 1], c[n - 1] = 0, -N.P32_MAX
    if n > 4:
        c[1], c[2] = -N.P32_MAX, N.P32_MAX
    return P.Table("t", [P.Column("g", T.BIGINT(), g.astype(np.int64)), P.Column("c", T.BIGINT(), c)], n)


def cells64_table(n=CELLS64_N, seed=19):
    """b: sixteen groups by row; c: both ends of the 24-bit envelope in every group's rows"""
    rng = np.random.default_rng(seed)
    c = rng.choice(np.array([-N.P32_MAX, N.P32_MAX, 1, -1], dtype=np.int64), n)
    return P.Table("t", [P.Column("b", T.BIGINT(), (np.arange(n, dtype=np.int64) % 16)), P.Column("c", T.BIGINT(), c)], n)


def fold_rows(max_grid, tiles, tail):
    return GRID_WAVES[max_grid] * tiles * N.TILE + tail


def warm_plans():
    """every plan shape of tests/test_gpu_lds_fold.py whose text tests/narrowcases.py's warm_plans do not already give, as (plan,
    environment) pairs for the build's code-object warm-up (each is compiled with narrow scans and without).  A kernel's text does
    not depend on the row count or on RSQ_MAX_GRID, but it does on the statistics: a table of one row has one group."""
    for kind in FOLD_KINDS:
        for tail in (0, 1):                               # (rows 0 and 1 alone: no statistics / one group)
            yield N.plan(N.FOLD, [N.fold_table(tail, kind, 1)]), {}
            yield N.plan(N.FOLD_GROUPED, [N.fold_table(tail, kind, 3)]), {}
    for n in SMALL_N + [300]:
        yield N.plan(MINMAX, [minmax_table(n)]), {}
    yield N.plan(CELLS64, [cells64_table(300)]), {}
