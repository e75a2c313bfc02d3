"""The device tail of dense aggregations keyed by dictionary-coded string columns (RSQ_DICT_SCANS=1; resql_amd/csrc/devtail.hip):
the key's part of Values::hash from a table of terms, the entry's bytes in the tuple, groups of CHAR(n) entries equal up to trailing
spaces merged on the device with the spelling of their first row.  Every statement is the oracle's answer, text and tuples, twice from
one compiled statement, and again with RSQ_DEVICE_TAIL=0; the path taken is read from RSQ_TRACE.  Shapes are the smallest at which a
piece can go wrong (tests/dicttailcases.py)."""
import os
import sys

import numpy as np
import pytest

from resql_amd import engine, plan as P
from oracle import orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dicttailcases as C  # noqa: E402
import dictgroupcases as G  # noqa: E402

pytestmark = pytest.mark.gpu
T = P.TypeInit
MERGED = "groups equal up to trailing spaces merged"
ON_DEVICE = "device tail"


@pytest.fixture(scope="module", autouse=True)
def _dictionary_images_on():
    """the images are opt-in (read when a table is created and when a statement is compiled): on for this module's tables"""
    old = os.environ.get("RSQ_DICT_SCANS")
    os.environ["RSQ_DICT_SCANS"] = "1"
    yield
    if old is None:
        os.environ.pop("RSQ_DICT_SCANS", None)
    else:
        os.environ["RSQ_DICT_SCANS"] = old


def _twice(ctx, stmt, tabs, want, multiset=False):
    q = ctx.sql_compile(stmt, tabs) if isinstance(stmt, str) else ctx.compile(stmt, tabs)
    try:
        assert G.NOTE in q.explain, q.explain                             # dense over the dictionary codes
        for _ in range(2):                                                # (the table is folded in place: the second execution starts clean)
            q.execute()
            got = q.result()
            if multiset:
                assert got.n_rows == want.n_rows and sorted(got.text.splitlines()) == sorted(want.text.splitlines()), stmt
            else:
                assert got.n_rows == want.n_rows and got.text == want.text and got.tuples == want.tuples, stmt
        return got
    finally:
        q.close()


def _check(ctx, monkeypatch, capfd, stmt, host, env=None, device=True, merged=False, multiset=False, replayed=None):
    """`stmt` (SQL text or a plan) under `env` with the trace on, then with RSQ_DEVICE_TAIL=0, both twice, all against the oracle; returns
    the answer and the first run's trace"""
    tabs = [ctx.table(t) for t in host]
    try:
        want = orc.execute(ctx.sql_plan(stmt, tabs, host) if isinstance(stmt, str) else stmt)
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        monkeypatch.setenv("RSQ_TRACE", "1")
        capfd.readouterr()
        got = _twice(ctx, stmt, tabs, want, multiset)
        err = capfd.readouterr().err
        assert (ON_DEVICE in err) == device, err[-3000:]
        assert (MERGED in err) == merged, err[-3000:]
        if replayed is not None:
            assert ("the reference's table replayed (device)" in err) == replayed, err[-3000:]
        monkeypatch.setenv("RSQ_DEVICE_TAIL", "0")
        _twice(ctx, stmt, tabs, want, multiset)
        assert ON_DEVICE not in capfd.readouterr().err
        monkeypatch.delenv("RSQ_DEVICE_TAIL")
        return got, err
    finally:
        for t in tabs:
            t.close()


FEW = dict(C.FEW, RSQ_DEVICE_TAIL_MIN="1")


@pytest.mark.parametrize("name", sorted(C.FEW_GROUPS))
def test_few_groups_host_replay(gpu_ctx, monkeypatch, capfd, name):
    """a handful of groups: ordered and hashed on the device, the reference's table replayed on the host.  Under VARCHAR 'ab' and 'ab '
    stay two groups and nothing is merged; under CHAR they are one where the width holds both"""
    kind, w, vals = C.FEW_GROUPS[name]
    got, err = _check(gpu_ctx, monkeypatch, capfd, C.SUMS, [C.few_groups_table(name)], FEW, merged=C.merges(kind, vals), replayed=False)
    if name == "varchar9_edge":
        assert got.n_rows == 12 and MERGED not in err
    if name == "char9_edge":
        assert got.n_rows == 11 and MERGED in err
    if name in ("one_entry", "two_entries", "256_entries"):
        assert got.n_rows == len(vals)


@pytest.mark.parametrize("first", [b"ab ", b"ab"], ids=["space_first", "space_later"])
def test_a_merged_group_shows_its_first_rows_spelling(gpu_ctx, monkeypatch, capfd, first):
    got, _ = _check(gpu_ctx, monkeypatch, capfd, C.ALL_AGGS, [C.spelling_table(first)], FEW, merged=True)
    assert got.n_rows == 2
    spelled = [got.value(r, 0) for r in range(2)]
    assert first in spelled and (b"ab" if first == b"ab " else b"ab ") not in spelled


def test_a_class_of_three_folds_concurrently(gpu_ctx, monkeypatch, capfd):
    """'x', 'x ' and 'x  ' with thousands of rows each, a as second key: two members fold into every representative at the same time;
    sum, min, max, avg and count"""
    got, _ = _check(gpu_ctx, monkeypatch, capfd, C.ALL_AGGS_BY_A, [C.class_of_three_table()], {"RSQ_DEVICE_TAIL_MIN": "1"}, merged=True)
    assert 1000 < got.n_rows <= 2000                                      # x (three spellings) and y, with nearly every a


@pytest.mark.parametrize("limit", [None, 1, 1234])
def test_device_replay_and_limit(gpu_ctx, monkeypatch, capfd, limit):
    sql = C.HBM + (f" limit {limit}" if limit else "")
    got, _ = _check(gpu_ctx, monkeypatch, capfd, sql, [C.replay_table()], {"RSQ_DEVICE_TAIL_MIN": "1"}, merged=True, replayed=True)
    assert got.n_rows == limit if limit else got.n_rows > 4096            # (beyond 4 096 groups the reference's table is replayed on the device)


def test_key_order_in_the_hash(gpu_ctx, monkeypatch, capfd):
    """coded, CHAR(1), coded, numeric: the CHAR(1) key doubles the sum of what stands in front of it, the coded keys add their terms at
    their places; output columns in another order than the keys"""
    got, _ = _check(gpu_ctx, monkeypatch, capfd, C.KEY_ORDER, [C.key_order_table()], {"RSQ_DEVICE_TAIL_MIN": "1"}, merged=True)
    assert got.n_rows > 4096


def test_no_group_and_one_group(gpu_ctx, monkeypatch, capfd):
    got, _ = _check(gpu_ctx, monkeypatch, capfd, C.NO_ROW, [C.few_groups_table("char9_edge")], FEW, merged=True)      # (the fold runs over an empty table)
    assert got.n_rows == 0
    one = G.table(1, T.CHAR(9), np.array([b"ab "], dtype="S9"), seed=29)
    got, _ = _check(gpu_ctx, monkeypatch, capfd, C.SUMS, [one], FEW)
    assert got.n_rows == 1


def test_taken_by_itself_at_the_default_threshold(gpu_ctx, monkeypatch, capfd):
    monkeypatch.delenv("RSQ_DEVICE_TAIL_MIN", raising=False)
    got, _ = _check(gpu_ctx, monkeypatch, capfd, C.HBM, [C.by_itself_table()])      # 256 000 groups
    assert got.n_rows > 4096


def test_emission_order_any_gives_the_same_rows(monkeypatch, capfd):
    ctx = engine.Context(device=0, emission_order=engine.EMIT_ANY)
    try:
        _check(ctx, monkeypatch, capfd, C.HBM, [C.replay_table()], {"RSQ_DEVICE_TAIL_MIN": "1"}, merged=True, multiset=True)
    finally:
        ctx.close()


@pytest.mark.parametrize("case", ["order_by", "computed_projection", "top_k_over_space_equivalent_keys"])
def test_still_on_the_host(gpu_ctx, monkeypatch, capfd, case):
    stmt, host, env = {"order_by": (C.ORDERED, C.replay_table(), {"RSQ_DEVICE_TAIL_MIN": "1"}),
                       "computed_projection": (C.COMPUTED, C.few_groups_table("char9_edge"), FEW),
                       "top_k_over_space_equivalent_keys": (C.TOP, C.top_table(), {})}[case]
    _check(gpu_ctx, monkeypatch, capfd, stmt, [host], env, device=False)


def test_derived_aggregation_reads_the_device_tails_tuples(gpu_ctx, monkeypatch, capfd):
    """HAVING over a sub-query grouped by a coded key: the derived table's columns are written from the tuples the device tail left"""
    t = C.replay_table()
    got, err = _check(gpu_ctx, monkeypatch, capfd, C.having_plan(t), [t], {"RSQ_DEVICE_TAIL_MIN": "1"}, merged=True)
    assert "from the device tail's tuples" in err
    assert got.n_rows > 0
