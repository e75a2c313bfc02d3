"""GROUP BY over dictionary-coded string columns as the code generator plans it, checked without a GPU: the code the scan loads is the
dense rank of the group (RSQ_DICT_SCANS=1), so the aggregation takes the register / LDS / HBM forms instead of a hash table; the text
holds the entry count and not the values; what keeps the hash form; and the host tail's step from rank to bytes, in a stand-alone
program under the address and undefined-behaviour sanitizers."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from resql_amd import datagen, plan as P, tpch_full

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dictcases as D  # noqa: E402
import dictgroupcases as G  # noqa: E402

T = P.TypeInit
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx(tmp_path_factory):
    from resql_amd import engine
    c = engine.Context(device=-1, cache_dir=str(tmp_path_factory.mktemp("kcache_dict_group")))
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _dictionary_images_on(monkeypatch):
    monkeypatch.setenv("RSQ_DICT_SCANS", "1")                             # (read when a table is created and a statement compiled)


def _source(ctx, sql, host_tables):
    tabs = [ctx.table(t) for t in host_tables]
    q = ctx.sql_compile(sql, tabs)
    try:
        return q.explain, q.source
    finally:
        q.close()
        for t in tabs:
            t.close()


def _simple(s_type, vals, n=4096):
    return P.Table("t", [P.Column("s", s_type, np.resize(np.asarray(vals), n)), P.Column("a", T.BIGINT(), np.arange(n, dtype=np.int64) % 1000)], n)


def test_group_by_a_coded_column_is_dense_over_the_code(ctx):
    ex, src = _source(ctx, G.COUNT, [_simple(T.CHAR(10), G.SHIPMODES)])
    assert "aggregation dense groups=7" in ex and "in registers" in ex
    assert "key s by dictionary code (7 entries)" in ex
    assert "ht0" not in src and "hash aggregation" not in ex              # no hash table
    assert "const int gk0 = (int)(vc_0);" in src and "const int gid = 0 + gk0 * 1;" in src
    assert "const rsq::Str v_0 = rsq::str(a.d0 + (u32)(vc_0) * 10u, 10);" in src      # the decode line stays (nothing reads it)
    assert "keys=[s{dictionary code, 7 entries}]" in ex


def test_the_text_holds_the_entry_count_not_the_values(ctx):
    a = _source(ctx, G.COUNT, [_simple(T.CHAR(10), G.SHIPMODES)])[1]
    b = _source(ctx, G.COUNT, [_simple(T.CHAR(10), G.values(7, 10, b"zz"), n=777)])[1]
    c = _source(ctx, G.COUNT, [_simple(T.CHAR(10), G.values(8, 10, b"zz"))])[1]
    assert G.NOTE in a and a == b                                         # other values, as many of them: one kernel
    assert G.NOTE in c and a != c                                         # 8 entries: another card, another kernel


def _is_hash(ex):
    return "hash aggregation" in ex and "aggregation dense" not in ex and G.NOTE not in ex


def test_257_values_keep_the_hash_form(ctx):
    ex, src = _source(ctx, G.COUNT, [_simple(T.VARCHAR(12), G.values(257, 12))])
    assert _is_hash(ex) and "ht0" in src


def test_agg_mode_5_keeps_the_hash_form(ctx, monkeypatch):
    monkeypatch.setenv("RSQ_AGG_MODE", "5")
    ex, src = _source(ctx, G.COUNT, [_simple(T.CHAR(10), G.SHIPMODES)])
    assert _is_hash(ex) and "ht0" in src and "(u32)(vc_0)" in src         # (the scan still reads the codes)


def test_a_key_from_the_build_side_of_a_join_keeps_the_hash_form(ctx):
    t, r = D.join_tables("CHAR", n=4000)
    ex, src = _source(ctx, D.JOIN_GROUP_SQL, [t, r])
    assert "hash aggregation" in ex and G.NOTE not in ex


_SWITCH = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from resql_amd import engine, plan as P
T = P.TypeInit
ctx = engine.Context(device=-1, cache_dir=sys.argv[2])
vals = np.resize(np.array([b"MAIL", b"SHIP", b"AIR", b"RAIL", b"TRUCK", b"FOB", b"REG AIR"], dtype="S10"), 1000)
t = P.Table("t", [P.Column("s", T.CHAR(10), vals), P.Column("a", T.BIGINT(), np.arange(1000, dtype=np.int64))], 1000)
q = ctx.sql_compile("select s, count(*) from t group by s", [ctx.table(t)])
sys.stdout.write(q.explain + "\n=====\n" + q.source)
q.close()
ctx.close()
"""


def test_the_switches_keep_the_hash_form(tmp_path):
    def run(**env):
        e = {k: v for k, v in os.environ.items() if k not in ("RSQ_DICT_SCANS", "RSQ_NARROW_SCANS", "RSQ_AGG_MODE")}
        e.update(env)
        name = "kc" + "".join(env.values())
        return subprocess.run([sys.executable, "-c", _SWITCH, ROOT, str(tmp_path / name)], env=e, check=True, capture_output=True, text=True).stdout
    on, off, narrow_off = run(RSQ_DICT_SCANS="1"), run(RSQ_DICT_SCANS="0"), run(RSQ_DICT_SCANS="1", RSQ_NARROW_SCANS="0")
    assert run() == off                                                   # unset: off
    assert "aggregation dense groups=7" in on and G.NOTE in on
    for out in (off, narrow_off):
        assert _is_hash(out.split("=====")[0]) and "vc_0" not in out and "ht0" in out


def test_char1_keeps_its_byte_set(ctx):
    ex, src = _source(ctx, "select f, count(*) from t group by f", [G.table(2000, T.CHAR(9), G.values(7))])
    assert "aggregation dense groups=3" in ex and G.NOTE not in ex and "keys=[f{65,78,82}]" in ex
    assert "(u8)a.k0_1" in src                                            # the compare chain over the distinct bytes


def test_mixed_keys_multiply(ctx):
    ex, src = _source(ctx, G.MIXED, [G.table(G.ROWS, T.VARCHAR(9), G.values(7))])
    assert f"aggregation dense groups={7 * 5 * 3 * 1000}" in ex
    assert "key s by dictionary code (7 entries), key u by dictionary code (5 entries)" in ex
    assert "const int gk0 = (int)(vc_0);" in src and "const int gk1 = (int)(vc_1);" in src
    assert f"gk0 * {5 * 3 * 1000} + gk1 * 3000 + gk2 * 1000 + gk3 * 1" in src
    assert "keys=[s{dictionary code, 7 entries} x u{dictionary code, 5 entries} x f{65,78,82} x a[0..999]]" in ex


@pytest.mark.parametrize("count,sql,groups,form", [
    (7, "select s, sum(a), count(*) from t group by s", 7, "in registers"),                     # 7 x 3 cells
    (12, "select s, u, count(*) from t group by s, u", 60, "in workgroup LDS table"),           # 12 x 5 groups, 120 cells
    (256, G.HBM, 256_000, "in HBM table"),
])
def test_the_form_follows_the_cells_as_for_every_dense_key(ctx, count, sql, groups, form):
    ex, src = _source(ctx, sql, [G.table(G.ROWS, T.CHAR(9), G.values(count))])
    assert f"aggregation dense groups={groups} " in ex and form in ex and G.NOTE in ex
    assert "ht0" not in src


def test_check_stats_checks_the_code_against_the_entry_count(ctx, monkeypatch):
    monkeypatch.setenv("RSQ_CHECK_STATS", "1")
    ex, src = _source(ctx, G.COUNT, [_simple(T.CHAR(10), G.SHIPMODES)])
    assert "int gk0 = (int)(vc_0);" in src
    assert "if ((u32)gk0 >= 7u) { atomicOr(a.err, (u32)rsq::ERR_GROUP_OVERFLOW); gk0 = 0; }" in src


def test_late_loads_hand_the_code_to_the_row_function(ctx):
    ex, src = _source(ctx, G.LATE, [G.table(20_000, T.CHAR(9), G.values(7))])
    assert "late loads" in ex and "lead_pred" in src and G.NOTE in ex
    assert "const int gk0 = (int)(vc_0);" in src


def test_behind_a_wave_compaction_the_code_travels_not_the_string(ctx):
    t, r = G.join_tables()
    ex, src = _source(ctx, G.JOIN_OWN, [t, r])
    probe = [l for l in ex.split("\n") if "scan t " in l][0]
    assert "wave compaction" in probe and "key s by dictionary code (12 entries)" in probe
    m = re.search(r"const int gk0 = \(int\)\((q_\d+)\);", src)
    assert m, "the group id reads the carried code"
    assert re.search(r"const u8 %s = \(\(u8\)\(qw_\d+\)\);" % m.group(1), src)
    assert re.search(r"cq_\d+ = \(\(i64\)\(vc_0\)\);", src)               # stage 1 pushes the code ...
    assert "rsq::str_addr(v_0)" not in src                                # ... and no address of the decoded value
    ex, src = _source(ctx, G.JOIN_PAYLOAD, [t, r])
    assert "hash aggregation" in ex and G.NOTE not in ex                  # a build-side payload keeps the hash form


def _tpch(sf, monkeypatch, cut=None):
    """the tables of Q12: whole at a small scale factor, or the first `cut` rows of lineitem with the values of `sf` (and as many of
    orders as keep the tables' proportions, which the join order follows)"""
    if cut is not None:
        for mod, fn, share in ((datagen, "n_lineitem", 1), (datagen, "n_orders", 4)):
            real = getattr(mod, fn)
            monkeypatch.setattr(mod, fn, lambda s, real=real, share=share: min(real(s), cut // share))
    return {t.name: t for t in (tpch_full.lineitem(sf), tpch_full.orders(sf))}


def test_q12_is_dense_over_l_shipmode_with_one_source_from_sf001_and_sf10_values(ctx, monkeypatch):
    small = _tpch(0.01, monkeypatch)
    large = _tpch(10, monkeypatch, cut=400_000)
    assert large["lineitem"].n_rows == 400_000 and small["lineitem"].n_rows < 100_000
    ex_s, src_s = _source(ctx, tpch_full.QUERIES["q12"], [small[t] for t in ("orders", "lineitem")])
    ex_l, src_l = _source(ctx, tpch_full.QUERIES["q12"], [large[t] for t in ("orders", "lineitem")])
    assert src_s == src_l
    for ex in (ex_s, ex_l):
        assert "aggregation dense groups=7 accumulators=2" in ex and "in workgroup LDS table" in ex      # (behind the probe's compaction: 256 threads)
        assert "key l_shipmode by dictionary code (7 entries)" in ex and "hash aggregation" not in ex
    assert re.search(r"const int gk0 = \(int\)\(q_\d+\);", src_s)


def test_the_host_tail_turns_ranks_into_dictionary_entries(tmp_path):
    """resql_amd/csrc/dense_groups.h under the sanitizers, as a program of its own: rank -> bytes and the NUL terminator for CHAR and
    VARCHAR at widths 2, 9 and 25, mixed keys, candidate rows"""
    exe = str(tmp_path / "dense_groups_test")
    src = os.path.join(ROOT, "resql_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-I" + src, "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "dense_groups_test.cpp"), os.path.join(src, "hostpar.cpp"), "-lpthread", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "dense_groups_test ok" in out.stdout
