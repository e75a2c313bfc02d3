"""One dictionary for all shards of a coded column (engine.unify_shard_dictionaries, ENGINE_DICT_MULTI), checked without a GPU on
compile-only contexts: every instance receives the union of the shards' entries in bytewise order; what is not unified is left exactly as
it was; a shard with unified statistics and unified dictionaries plans GROUP BY over the column dense by the code, as one context does,
and shards whose dictionaries were not unified keep the hash form with the reasons they gave before."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from resql_amd import engine, plan as P

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dictcases as D  # noqa: E402
import dictgroupcases as G  # noqa: E402
import dictjoincases as J  # noqa: E402
import dictmulticases as M  # noqa: E402
import shardcases  # noqa: E402

T = P.TypeInit


@pytest.fixture(scope="module")
def ctx(tmp_path_factory):
    c = engine.Context(device=-1, cache_dir=str(tmp_path_factory.mktemp("kcache_dict_multi")))
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _dictionary_images_on(monkeypatch):
    monkeypatch.setenv("RSQ_DICT_SCANS", "1")                             # (read when a table is created and a statement compiled)


def _state(tb, cols=("s", "u")):
    return [(tb.image_info(c), tb.read_image(c, 1).tobytes()) for c in cols]


def _close(tabs):
    for t in tabs:
        t.close()


@pytest.mark.parametrize("n_shards", [2, 3])
@pytest.mark.parametrize("kind,w", M.RECODE_TYPES)
def test_every_instance_receives_the_sorted_union(ctx, tmp_path_factory, n_shards, kind, w):
    parts = M.shards(getattr(T, kind)(w), D.edge_values(w), 300)[-n_shards:]      # (two shards: B and C, neither holds every value)
    other = engine.Context(device=-1, cache_dir=str(tmp_path_factory.mktemp("kcache_other")))      # the instances may sit on different contexts
    tabs = [(other if i == 1 else ctx).table(p) for i, p in enumerate(parts)]
    try:
        want = M.sorted_union(parts)
        assert any(tb.image_info("s")[2] != len(want) for tb in tabs)     # the shards' own dictionaries differ
        engine.unify_shard_dictionaries(tabs)
        for tb in tabs:
            assert tb.image_info("s")[2] == len(want)
            assert np.array_equal(M.entries(tb), want)
        before = [_state(tb) for tb in tabs]
        engine.unify_shard_dictionaries(tabs)                             # a second call changes nothing
        assert [_state(tb) for tb in tabs] == before
    finally:
        _close(tabs)
        other.close()


def test_a_union_of_256_values_is_unified_and_one_of_257_is_not(ctx):
    for extra, unified in ((0, True), (1, False)):
        a = G.table(600, T.VARCHAR(9), G.values(128, 9, b"a"), seed=1)
        b = G.table(600, T.VARCHAR(9), G.values(128 + extra, 9, b"b"), seed=2)
        tabs = [ctx.table(a), ctx.table(b)]
        try:
            before = [_state(tb) for tb in tabs]
            assert [s[0][0][2] for s in before] == [128, 128 + extra]
            engine.unify_shard_dictionaries(tabs)
            if unified:
                for tb in tabs:
                    assert tb.image_info("s")[2] == 256 and np.array_equal(M.entries(tb), M.sorted_union([a, b]))
            else:
                assert [_state(tb) for tb in tabs] == before              # nothing changed on any instance
                q = ctx.sql_compile(G.SUMS, [tabs[0]])                    # ... and the instance is one table of its own, dense over its own dictionary
                assert "by dictionary code (128 entries)" in q.explain
                q.close()
        finally:
            _close(tabs)


def test_a_shard_without_a_dictionary_blocks_that_column_only(ctx):
    a = G.table(1_000, T.VARCHAR(9), G.values(7), seed=1)
    b = G.table(1_000, T.VARCHAR(9), G.values(300), seed=2)               # 300 values: no dictionary of s on this shard
    b.col("u").data[:] = np.resize(np.array([b"MAIL", b"SHIP", b"AIR"], dtype="S6"), 1_000)      # u: 3 of the 5 values here
    tabs = [ctx.table(a), ctx.table(b)]
    try:
        before = [_state(tb, ("s",)) for tb in tabs]
        assert [tb.image_info("s")[2] for tb in tabs] == [7, 0] and [tb.image_info("u")[2] for tb in tabs] == [5, 3]
        engine.unify_shard_dictionaries(tabs)
        assert [_state(tb, ("s",)) for tb in tabs] == before
        assert [tb.image_info("u")[2] for tb in tabs] == [5, 5]
        assert np.array_equal(M.entries(tabs[1], "u"), M.entries(tabs[0], "u"))
    finally:
        _close(tabs)


def test_a_shard_without_rows_blocks_nothing_and_takes_the_union(ctx):
    parts = M.shards(T.CHAR(9), D.edge_values(9, 12), [300, 0, 300])
    tabs = [ctx.table(p) for p in parts]
    try:
        assert tabs[1].image_info("s")[2] == 0
        engine.unify_shard_dictionaries(tabs)
        want = M.sorted_union(parts)
        for tb in tabs:
            assert tb.image_info("s")[2] == len(want) == 12 and np.array_equal(M.entries(tb), want)
    finally:
        _close(tabs)


def test_shards_of_different_schemas_are_refused(ctx):
    a = G.table(100, T.VARCHAR(9), G.values(7))
    b = G.table(100, T.VARCHAR(12), G.values(7, 12))
    tabs = [ctx.table(a), ctx.table(b)]
    try:
        with pytest.raises(engine.EngineError) as e:
            engine.unify_shard_dictionaries(tabs)
        assert e.value.status == 1 and "another schema" in str(e.value)
    finally:
        _close(tabs)


def _is_hash(ex):
    return "hash aggregation" in ex and "aggregation dense" not in ex and G.NOTE not in ex


def _compiled(ctx, sql, tabs):
    q = ctx.sql_compile(sql, tabs)
    try:
        return q.explain, q.source, shardcases.layout_line(q) if "partial table:" in q.explain else None
    finally:
        q.close()


def test_a_unified_shard_groups_dense_by_the_code_of_the_union(ctx):
    """fails without the feature: a shard of a larger table keeps the hash form there, whatever its dictionary holds"""
    def shards(vals):
        parts = M.random_shards(T.CHAR(9), vals)
        tabs = M.place([ctx] * 3, parts)
        M.unify_stats(tabs)
        return parts, tabs
    parts, tabs = shards(D.edge_values(9, 12))
    try:
        for tb in tabs:
            assert _is_hash(_compiled(ctx, G.SUMS, [tb])[0])              # statistics unified, dictionaries not: as before
        engine.unify_shard_dictionaries(tabs)
        got = [_compiled(ctx, G.SUMS, [tb]) for tb in tabs]
        for ex, src, layout in got:
            assert "aggregation dense groups=12 " in ex and "key s by dictionary code (12 entries)" in ex
            assert "const int gk0 = (int)(vc_0);" in src
            assert layout == got[0][2] and "keys=[s{dictionary code, 12 entries}]" in layout
        # the text holds the count and not the values: other values, as many of them in the union, one kernel
        _, others = shards(G.values(12, 9, b"zz"))
        try:
            engine.unify_shard_dictionaries(others)
            assert _compiled(ctx, G.SUMS, [others[0]])[1] == got[0][1]
        finally:
            _close(others)
        # the partial entry points follow: the table merges with the siblings'
        q = ctx.sql_compile(G.SUMS, [tabs[1]])
        assert q.partial_layout() == (12, 0, 24)
        q.close()
    finally:
        _close(tabs)


def test_a_build_side_key_is_dense_where_the_origins_copies_agree(ctx, monkeypatch):
    monkeypatch.setenv("RSQ_DICT_SCANS", "2")
    t, r = J.tables()
    parts = [G.table(2_000, T.CHAR(9), v, seed=40 + i) for i, v in enumerate(M.shard_values(D.edge_values(9, 12)))]
    tabs = M.place([ctx] * 3, parts)
    copies = [ctx.table(r) for _ in range(3)]
    try:
        M.unify_stats(tabs)
        line = [l for l in _compiled(ctx, J.JOIN_PAYLOAD, [tabs[0], copies[0]])[0].split("\n") if "aggregation" in l][-1]
        assert "key ru not by dictionary code: t is a shard of a larger table" in line      # the refusal of today
        engine.unify_shard_dictionaries(tabs)
        line = [l for l in _compiled(ctx, J.JOIN_PAYLOAD, [tabs[0], copies[0]])[0].split("\n") if "aggregation" in l][-1]
        assert "key ru not by dictionary code: t is a shard of a larger table" in line      # r's copies have not been compared
        engine.unify_shard_dictionaries(copies)
        for tb, rc in zip(tabs, copies):
            ex, src, layout = _compiled(ctx, J.JOIN_PAYLOAD, [tb, rc])
            assert "aggregation dense groups=4 " in ex and "key ru by dictionary code of r.ru (4 entries)" in ex and "dict_rank<6>" in src
    finally:
        _close(tabs + copies)


def test_a_single_context_refuses_the_flag_of_multi_gpu_handles():
    L = engine.lib()
    h = C.c_void_p()
    assert engine.ENGINE_DICT_MULTI == 16
    bad = engine.rsq_config.make(-1, engine_flags=16)
    assert L.rsq_ctx_create(C.byref(bad), C.byref(h)) == 1 and b"engine_flags" in L.rsq_last_error(None)
    assert b"RSQ_ENGINE_DICT_MULTI" in L.rsq_last_error(None)
    unknown = engine.rsq_config.make(-1, engine_flags=32)
    assert L.rsq_ctx_create(C.byref(unknown), C.byref(h)) == 1 and b"does not know" in L.rsq_last_error(None)
