"""GROUP BY over a dictionary-coded string that comes from a join's build side, as the code generator plans it (RSQ_DICT_SCANS=2),
checked without a GPU: the payload word holds an address inside the origin column's dictionary image in both forms of the join table,
the group's dense rank is (address - dictionary) / width, the text holds the width and the entry count and no address; what keeps the
hash form, with the reason in explain; and RSQ_DICT_SCANS=1 keeps every text it had."""
import os
import re
import sys

import numpy as np
import pytest

from resql_amd import engine, plan as P, tpch_full

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dictcases as D  # noqa: E402
import dictgroupcases as G  # noqa: E402
import dictjoincases as J  # noqa: E402

T = P.TypeInit


@pytest.fixture(scope="module")
def ctx(tmp_path_factory):
    c = engine.Context(device=-1, cache_dir=str(tmp_path_factory.mktemp("kcache_dict_join")))
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _join_keys_on(monkeypatch):
    monkeypatch.setenv("RSQ_DICT_SCANS", "2")                             # (read when a table is created and a statement compiled)


def _source(ctx, stmt, host_tables, prepare=None):
    tabs = [ctx.table(t) for t in host_tables]
    if prepare:
        prepare(tabs)
    q = ctx.sql_compile(stmt, tabs) if isinstance(stmt, str) else ctx.compile(stmt, tabs)
    try:
        return q.explain, q.source
    finally:
        q.close()
        for t in tabs:
            t.close()


def _agg_line(ex):
    return [l for l in ex.split("\n") if "aggregation" in l][-1]


def _is_hash(ex):
    return "hash aggregation" in ex and "aggregation dense" not in ex and J.NOTE + " of" not in ex


def test_a_build_side_payload_is_dense_over_its_origins_dictionary(ctx, monkeypatch):
    """fails without the feature: the statement is a hash aggregation there, whatever the switch says"""
    t, r = G.join_tables()
    ex, src = _source(ctx, J.JOIN_PAYLOAD, [t, r])
    assert "aggregation dense groups=4 " in ex and "in workgroup LDS table" in ex and "wave compaction" in ex
    assert "key ru by dictionary code of r.ru (4 entries)" in ex and "hash aggregation" not in ex
    assert "keys=[ru{dictionary code, 4 entries}]" in ex
    # the rank from the carried address: the dictionary's address is an argument, the text holds the width and the entry count
    assert "const char* gd0;" in src
    assert re.search(r"const u64 r = dict_rank<6>\(ht0_v\d+, a\.gd0\); if \(r < 4ull\) gk0 = \(int\)r; else atomicOr\(a\.err, \(u32\)rsq::ERR_GROUP_OVERFLOW\);", src)
    assert "return (u64)(v.p - dict) / (u64)W;" in src
    assert "0x" not in "".join(l for l in src.split("\n") if "gd0" in l)
    monkeypatch.setenv("RSQ_DICT_SCANS", "1")
    ex1, src1 = _source(ctx, J.JOIN_PAYLOAD, [t, r])
    assert _is_hash(ex1) and "dict_rank" not in src1 and "gd0" not in src1 and "not by dictionary code" not in ex1


def test_the_text_holds_no_value_and_no_address(ctx):
    a = _source(ctx, J.JOIN_PAYLOAD, list(J.tables()))[1]
    b = _source(ctx, J.JOIN_PAYLOAD, list(J.tables(vals=G.values(4, 6, b"z"))))[1]
    c = _source(ctx, J.JOIN_PAYLOAD, list(J.tables(vals=G.values(5, 6, b"z"))))[1]
    assert "dict_rank<6>" in a and a == b                                 # other values, as many of them: one kernel
    assert a != c and "r < 5ull" in c


def _statements():
    edge = G.table(G.ROWS, T.CHAR(9), D.edge_values(9, 12), seed=2)
    out = [(name, sql, [edge]) for name, sql in sorted(G.STATEMENTS.items())]
    t, r = G.join_tables()
    out += [("join_own", G.JOIN_OWN, [t, r]), ("join_own_hbm", G.JOIN_OWN_HBM, [t, r])]
    return out


@pytest.mark.parametrize("name,sql,host", _statements(), ids=[s[0] for s in _statements()])
def test_statements_without_a_build_side_key_keep_their_text(ctx, monkeypatch, name, sql, host):
    ex2, src2 = _source(ctx, sql, host)
    monkeypatch.setenv("RSQ_DICT_SCANS", "1")
    ex1, src1 = _source(ctx, sql, host)
    assert src2 == src1 and ex2 == ex1


def test_the_payload_join_alone_changes_under_the_switch(ctx, monkeypatch):
    t, r = G.join_tables()
    src2 = _source(ctx, J.JOIN_PAYLOAD, [t, r])[1]
    monkeypatch.setenv("RSQ_DICT_SCANS", "1")
    assert src2 != _source(ctx, J.JOIN_PAYLOAD, [t, r])[1]


def test_the_direct_and_the_built_form_both_yield_dictionary_addresses(ctx, monkeypatch):
    """one kernel, two forms behind a.ht0_direct: the direct branch reads the build table's code column and dictionary, the built
    branch loads the address the build pipeline stored - which that pipeline made from a.d<k> + code * width"""
    host = list(J.tables(keys=np.arange(600)))
    ex, src = _source(ctx, J.JOIN_PAYLOAD, host)
    assert "aggregation dense groups=4 " in ex and "of r.ru" in ex
    assert "const u8* ht0_code1;" in src and "const char* ht0_dict1;" in src and "ht0_src1" in src
    m = re.search(r"const i64 ht0_w1 = a\.ht0_direct \? (.*?) : (a\.ht0_words\[.*?\]);", src)
    assert m and m.group(1) == "(i64)(u64)(a.ht0_dict1 + (u32)a.ht0_code1[ht0_s] * 6u)"
    assert "const rsq::Str ht0_v1 = rsq::str_from_addr(ht0_w1, 6);" in src and "dict_rank<6>(ht0_v1, a.gd0)" in src
    build = src.split("scan t")[0] if "scan t" in src else src
    assert re.search(r"const rsq::Str v_\d+ = rsq::str\(a\.d\d+ \+ \(u32\)\(vc_\d+\) \* 6u, 6\);", build)
    assert re.search(r"rec\[1\] = rsq::str_addr\(v_\d+\);", build)         # the build stores the address inside the image
    monkeypatch.setenv("RSQ_DICT_SCANS", "1")
    src1 = _source(ctx, J.JOIN_PAYLOAD, host)[1]
    assert "ht0_code1" not in src1 and "(i64)(u64)(a.ht0_src1 + ht0_s * 6ull)" in src1      # the wide column, as before


def test_the_origin_is_carried_from_table_to_table(ctx):
    """m probes n's table (in place or built: both hand out dictionary addresses) and stores the name's address in its own; t finds it there"""
    plan = J.two_hop_plan()
    ex, src = _source(ctx, plan, plan.tables)
    assert re.search(r"scan m .* probe ht0 \(single match\) -> build hash table ht1", ex)
    assert "key nname by dictionary code of n.nname (25 entries)" in ex and re.search(r"dict_rank<25>\(ht1_v\d+, a\.gd0\)", src)
    assert "(i64)(u64)(a.ht0_dict1 + (u32)a.ht0_code1[ht0_s] * 25u)" in src


def test_a_probe_whose_build_keys_repeat_keeps_the_hash_form(ctx):
    keys = np.sort(np.concatenate([J.scattered_keys(599), [7]]))          # ascending, 7 twice: the statistics know
    ex, src = _source(ctx, J.JOIN_PAYLOAD, list(J.tables(keys=keys)))
    assert _is_hash(ex) and "probe ht0 (all matches)" in ex
    assert "key ru not by dictionary code: the build keys of ht0 repeat" in _agg_line(ex)
    ex, src = _source(ctx, J.JOIN_PAYLOAD, list(J.tables(keys=np.arange(1200) % 600)))      # more rows than values
    assert _is_hash(ex) and "the build keys of ht0 repeat" in _agg_line(ex)


def test_agg_mode_5_keeps_the_hash_form(ctx, monkeypatch):
    monkeypatch.setenv("RSQ_AGG_MODE", "5")
    ex, src = _source(ctx, J.JOIN_PAYLOAD, list(J.tables()))
    assert _is_hash(ex) and "RSQ_AGG_MODE=5" in _agg_line(ex) and "dict_rank" not in src


def test_a_257_value_build_column_keeps_the_hash_form(ctx):
    ex, src = _source(ctx, J.JOIN_PAYLOAD, list(J.tables(T.VARCHAR(9), G.values(257))))
    assert _is_hash(ex) and "key ru not by dictionary code: its bytes do not stand in a dictionary image" in _agg_line(ex)
    ex, src = _source(ctx, J.JOIN_PAYLOAD, list(J.tables(T.VARCHAR(9), G.values(256))))
    assert "aggregation dense groups=256 " in ex


def test_a_computed_string_key_keeps_the_hash_form(ctx):
    plan = J.computed_key_plan()
    ex, src = _source(ctx, plan, plan.tables)
    assert _is_hash(ex) and "not by dictionary code: a computed value" in _agg_line(ex)


def test_a_key_out_of_a_derived_table_keeps_the_hash_form(ctx):
    plan = J.derived_key_plan()
    ex, src = _source(ctx, plan, plan.tables)
    top = ex.split("derived table")[0]
    assert "derived table" in ex and _is_hash(top) and "key ru not by dictionary code: its bytes do not stand in a dictionary image" in top


@pytest.mark.parametrize("which", [0, 1], ids=["probe_side", "build_side"])
def test_a_shard_of_either_table_keeps_the_hash_form(ctx, which):
    """a table that plans as a range of a larger one (its siblings hold other dictionaries): the refusal of a scan-own coded key, for the
    scanned table and for the origin alike.  (A slice view, multi.cpp sliceOf, is such a table without images: no origin at all.)"""
    def shard(tabs):
        tabs[which].unify_shard_stats([tabs[which].stats_blob(), tabs[which].stats_blob()])
    ex, src = _source(ctx, J.JOIN_PAYLOAD, list(J.tables()), prepare=shard)
    assert _is_hash(ex) and " is a shard of a larger table" in _agg_line(ex) and ("key ru not by dictionary code: " + "tr"[which] + " is") in _agg_line(ex)


def test_q5_is_dense_over_n_name_behind_its_compaction(ctx, monkeypatch):
    db = tpch_full.database(0.01)
    host = [db[k] for k in sorted(db)]
    ex, src = _source(ctx, tpch_full.QUERIES["q5"], host)
    li = [l for l in ex.split("\n") if "scan lineitem" in l][0]
    assert "wave compaction" in li and "aggregation dense groups=25 accumulators=1" in li and "in workgroup LDS table" in li
    assert "key n_name by dictionary code of nation.n_name (25 entries)" in li and "hash aggregation" not in ex
    # the value crossed two tables on its way: nation's build, then the supplier's, whose entry the lineitem row finds
    assert re.search(r"scan supplier .* probe ht1 .* build hash table ht2", ex) and re.search(r"probe ht2 .* aggregation dense", li)
    assert re.search(r"dict_rank<25>\(ht2_v\d+, a\.gd0\)", src) and "r < 25ull" in src
    monkeypatch.setenv("RSQ_DICT_SCANS", "1")
    ex1, src1 = _source(ctx, tpch_full.QUERIES["q5"], host)
    assert _is_hash(ex1) and "dict_rank" not in src1
