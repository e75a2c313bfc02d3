"""Dictionary images (one u8 code per row + the sorted distinct values) as the code generator sees them, checked without a GPU: which
string columns are coded, that the kernel text holds the width only (the dictionary's address and entry count are arguments), that
TPC-H Q12 / Q14 / Q19 generate one source at SF 0.01 and from SF 10's values, and that the two switches give scans without the decode."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from resql_amd import datagen, plan as P, tpch_full

T = P.TypeInit
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx(tmp_path_factory):
    from resql_amd import engine
    c = engine.Context(device=-1, cache_dir=str(tmp_path_factory.mktemp("kcache_dict")))
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _dictionary_images_on(monkeypatch):
    monkeypatch.setenv("RSQ_DICT_SCANS", "1")                             # (the images are opt-in: read when a table is created and a statement compiled)


def _values(count, width, salt=b""):
    """`count` distinct values of at most `width` bytes"""
    return np.array([salt + b"%x" % i for i in range(count)], dtype=f"S{width}")


def _table(s_type, values, n=4096):
    vals = np.resize(np.asarray(values), n)
    return P.Table("t", [P.Column("s", s_type, vals), P.Column("a", T.BIGINT(), np.arange(n, dtype=np.int64) % 1000)], n)


def _source(ctx, sql, host_tables):
    tabs = [ctx.table(t) for t in host_tables]
    q = ctx.sql_compile(sql, tabs)
    try:
        return q.explain, q.source
    finally:
        q.close()
        for t in tabs:
            t.close()


GROUPS = "select s, count(*) from t group by s"
WHERE = "select sum(a) from t where s = 'MAIL' or s like '%AIR'"
SHIPMODES = np.array([b"MAIL", b"SHIP", b"AIR", b"RAIL", b"TRUCK", b"FOB", b"REG AIR"], dtype="S10")


def _coded(src, k=0):
    return f"const u8* c{k};" in src and f"const char* d{k};" in src


def test_char10_with_seven_values_is_coded(ctx):
    ex, src = _source(ctx, GROUPS, [_table(T.CHAR(10), SHIPMODES)])
    assert "const u8* c0;" in src and "const char* d0;" in src and "i64 dn0;" in src
    assert "rsq::str(a.d0 + (u32)(vc_0) * 10u, 10)" in src               # the row's value points into the dictionary
    assert "rsq::ld2(a.c0 + b, t0_0);" in src                            # a one-byte tile column: no staging, no prefetched words
    assert "a.c0[r]" in src and "strt" not in src and "_w0" not in src
    assert "10 B/row, 1 B/row stored]" in ex


def test_predicate_over_one_coded_column_is_a_truth_table(ctx):
    ex, src = _source(ctx, WHERE, [_table(T.CHAR(10), SHIPMODES)])
    assert "__shared__ u64 s_dt[4];" in src and "dt0_eval(a, rsq::str(a.d0 + dt_e * 10u, 10))" in src
    assert "dt_e < (u32)a.dn0" in src                                     # entries past the dictionary's count evaluate to 0
    assert "rsq::dict_bit(s_dt + 0 * 4, vc_0)" in src
    assert "rsq::like(v_0" in src.split("dt0_eval")[1].split("\n")[0]     # the table is filled by the expression's own text
    assert "18 B/row, 3 B/row stored]" in ex                               # (a: two bytes of its narrow image)


@pytest.mark.parametrize("count,coded", [(1, True), (2, True), (256, True), (257, False), (4096, False)])
def test_at_most_256_distinct_values(ctx, count, coded):
    ex, src = _source(ctx, GROUPS, [_table(T.VARCHAR(12), _values(count, 12))])
    assert _coded(src) == coded
    assert ("B/row stored]" in ex) == coded


def test_values_that_differ_only_in_padding_are_two_entries(ctx):
    # all n stored bytes count: 'ab' and 'ab ' are two entries (that compare equal as CHAR)
    vals = np.array([b"k%03d" % i for i in range(255)] + [b"ab", b"ab "], dtype="S8")
    assert not _coded(_source(ctx, GROUPS, [_table(T.CHAR(8), vals)])[1])
    assert _coded(_source(ctx, GROUPS, [_table(T.CHAR(8), vals[1:])])[1])


def test_char1_is_untouched(ctx):
    ex, src = _source(ctx, GROUPS, [_table(T.CHAR(1), np.array([b"A", b"N", b"R"], dtype="S1"))])
    assert "d0;" not in src and "vc_0" not in src and "B/row stored]" not in ex


def test_the_text_holds_the_width_only(ctx):
    a = _source(ctx, WHERE, [_table(T.CHAR(10), SHIPMODES)])[1]
    b = _source(ctx, WHERE, [_table(T.CHAR(10), _values(200, 10, b"zz"), n=777)])[1]
    assert _coded(a) and a == b                                           # other entries, another count: one kernel
    c = _source(ctx, WHERE, [_table(T.CHAR(11), SHIPMODES.astype("S11"))])[1]
    assert _coded(c) and a != c


def test_columns_without_data_and_empty_tables_stay_wide(ctx):
    t = _table(T.CHAR(10), SHIPMODES, n=0)
    ex, src = _source(ctx, GROUPS, [t])
    assert not _coded(src)


_SWITCH = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from resql_amd import engine, plan as P
T = P.TypeInit
ctx = engine.Context(device=-1, cache_dir=sys.argv[2])
vals = np.resize(np.array([b"MAIL", b"SHIP", b"AIR"], dtype="S10"), 1000)
t = P.Table("t", [P.Column("s", T.CHAR(10), vals), P.Column("a", T.BIGINT(), np.arange(1000, dtype=np.int64))], 1000)
q = ctx.sql_compile("select sum(a) from t where s = 'MAIL' or s like '%AIR'", [ctx.table(t)])
sys.stdout.write(q.explain + "\n=====\n" + q.source)
q.close()
ctx.close()
"""


def test_the_switches_give_scans_without_the_decode(tmp_path):
    def run(**env):
        e = {k: v for k, v in os.environ.items() if k not in ("RSQ_DICT_SCANS", "RSQ_NARROW_SCANS")}
        e.update(env)
        name = "kc" + "".join(env.values())
        return subprocess.run([sys.executable, "-c", _SWITCH, ROOT, str(tmp_path / name)], env=e, check=True, capture_output=True, text=True).stdout
    on, off, narrow_off = run(RSQ_DICT_SCANS="1"), run(RSQ_DICT_SCANS="0"), run(RSQ_DICT_SCANS="1", RSQ_NARROW_SCANS="0")
    assert run() == off                                                   # unset: off
    assert "const char* d0;" in on and "dict_bit" in on and "18 B/row, 3 B/row stored]" in on
    for src in (off, narrow_off):
        assert "const char* c0;" in src and "d0;" not in src and "dict_bit" not in src and "s_dt" not in src and "vc_0" not in src
    assert "12 B/row stored]" in off                                      # (column a keeps its narrow image: only the dictionary is off)
    assert "B/row stored]" not in narrow_off


def _tpch(sf, monkeypatch, cut=None):
    """the tables of Q12 / Q14 / Q19: whole at a small scale factor, or the first `cut` rows of lineitem with the values of `sf` (and
    as many of orders and part as keep the tables' proportions, which the join order follows)"""
    if cut is not None:
        for mod, fn, share in ((datagen, "n_lineitem", 1), (datagen, "n_orders", 4), (tpch_full, "n_part", 30)):
            real = getattr(mod, fn)
            monkeypatch.setattr(mod, fn, lambda s, real=real, share=share: min(real(s), cut // share))
    return {t.name: t for t in (tpch_full.lineitem(sf), tpch_full.orders(sf), tpch_full.part(sf))}


def test_q12_q14_q19_same_source_from_sf001_and_sf10_values(ctx, monkeypatch):
    small = _tpch(0.01, monkeypatch)
    large = _tpch(10, monkeypatch, cut=400_000)
    assert large["lineitem"].n_rows == 400_000 and small["lineitem"].n_rows < 100_000
    for name, tables, decoded in (("q12", ("orders", "lineitem"), "l_shipmode"), ("q14", ("lineitem", "part"), "p_type"),
                                  ("q19", ("lineitem", "part"), "l_shipinstruct")):
        ex_s, src_s = _source(ctx, tpch_full.QUERIES[name], [small[t] for t in tables])
        ex_l, src_l = _source(ctx, tpch_full.QUERIES[name], [large[t] for t in tables])
        assert src_s == src_l, name
        assert re.search(r"rsq::str\(a\.d\d+ \+ \(u32\)\(vc_\d+\)", src_s), name
        assert "B/row stored]" in ex_s, name
    ex, src = _source(ctx, tpch_full.QUERIES["q19"], [small["lineitem"], small["part"]])
    assert "dict_bit" in src                                              # l_shipinstruct = ..., l_shipmode in (...): truth tables
