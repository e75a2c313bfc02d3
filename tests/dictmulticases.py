"""Tables of tests/test_dict_multi_codegen.py and tests/test_gpu_dict_multi.py: the shards of one table whose dictionaries of the coded
column s differ, as engine.unify_shard_dictionaries and a MultiContext with ENGINE_DICT_MULTI make them one.  Shard A holds every value,
shard B lacks the value that sorts first (every one of its codes moves when it receives the union), shard C holds a strict subset.  Built
on dictcases / dictgroupcases: the same columns, s filled value after value so that a shard of one row is decided too."""
import numpy as np

from resql_amd import engine, plan as P

import dictcases as D
import dictgroupcases as G

T = P.TypeInit

RECODE_ROWS = [1, 15, 16, 17, 255, 256, 257, G.ROWS]                      # around one 16-byte vector, one workgroup's 256 lanes, and many tiles
RECODE_TYPES = [("CHAR", 2), ("VARCHAR", 9), ("CHAR", 25)]


def shard_values(vals):
    """(A, B, C) of the values, each in descending bytewise order: a shard of one row holds its largest value, not the union's first"""
    s = np.sort(np.asarray(vals))[::-1]
    return s, (s[1:-1] if len(s) > 3 else s[:-1]), s[::2][:max(1, len(s) // 2)]


def table(n, s_type, vals, seed=1, name="t"):
    """dictgroupcases.table with s = the values in turn (row r holds vals[r % len(vals)])"""
    vals = np.asarray(vals)
    t = G.table(n, s_type, vals, seed=seed, name=name)
    if n:
        t.col("s").data[:] = vals[np.arange(n) % len(vals)]
    return t


def shards(s_type, vals, rows, seed=20):
    """the three shards as host tables; rows: one count, or one per shard"""
    rows = [rows] * 3 if isinstance(rows, int) else list(rows)
    return [table(n, s_type, v, seed=seed + i) for i, (n, v) in enumerate(zip(rows, shard_values(vals)))]


def random_shards(s_type, vals, rows=(2_000, 2_500, 2_100), seed=30):
    """the three shards with s drawn at random (every value of a shard occurs in it)"""
    return [G.table(n, s_type, v, seed=seed + i) for i, (n, v) in enumerate(zip(rows, shard_values(vals)))]


def concat(parts):
    first = parts[0]
    return P.Table(first.name, [P.Column(c.name, c.type, np.concatenate([p.columns[i].data for p in parts])) for i, c in enumerate(first.columns)],
                   sum(p.n_rows for p in parts))


def plan_over(sql, whole):
    """the statement's plan over the whole tables, made without a device"""
    cc = engine.Context(device=-1)
    try:
        tabs = [cc.table(t) for t in whole]
        return cc.sql_plan(sql, tabs, list(whole))
    finally:
        cc.close()


def unify_stats(tabs):
    blobs = [t.stats_blob() for t in tabs]
    for t in tabs:
        t.unify_shard_stats(blobs)


def place(contexts, parts):
    """the shards' device tables, each numbered over the whole table"""
    out, row0 = [], 0
    for ctx, p in zip(contexts, parts):
        tb = ctx.table(p)
        tb.set_row0(row0)
        row0 += p.n_rows
        out.append(tb)
    return out


def entries(tb, col="s"):
    w = tb.widths[col]
    return tb.read_image(col, 1).reshape(-1, w)


def sorted_union(parts, col="s"):
    """the bytes of the distinct values of all parts, padded to the width, in bytewise order"""
    w = parts[0].col(col).type.width
    vals = np.unique(np.concatenate([np.asarray(p.col(col).data, dtype=f"S{w}") for p in parts]))
    raw = np.zeros((len(vals), w), dtype=np.uint8)
    for i, v in enumerate(vals):
        raw[i, :len(v)] = np.frombuffer(v, dtype=np.uint8)
    order = sorted(range(len(vals)), key=lambda i: raw[i].tobytes())
    return raw[order]
