"""BULK INSERT parsed on the device (rsq_table_load_tbl_ex mode 2, rsq_config.tbl_ingest = 1) against the host path (mode 1), which is
the code tests/test_tbl_ingest.py pins to the reference: every column byte for byte, the statistics blobs, the error texts.  The
device path is never compared with itself."""
import pytest

from resql_amd import engine

import tblcases
import tbldevcases
from test_tbl_ingest import ACCEPTED, ODD, REJECTED

pytestmark = pytest.mark.gpu

HOST, DEVICE = engine.TBL_HOST, engine.TBL_DEVICE


def outcome(ctx, schema, path, mode, **kw):
    """what a load gives: ("error", status, message) or ("ok", rows, {column: bytes}, statistics blob); and its report (None after an error)"""
    try:
        t = ctx.load_tbl(schema, path, mode=mode, **kw)
    except engine.EngineError as e:
        return ("error", e.status, e.message), None
    try:
        cols = {c.name: t.read_column(c.name, c.type.np_dtype).tobytes() for c in schema.columns}
        return ("ok", t.n_rows, cols, t.stats_blob()), t.load_report
    finally:
        t.close()


@pytest.fixture(scope="module")
def host_loaded(gpu_ctx):
    """the fixtures through the host path, once: the yardstick of the tests below"""
    return {name: outcome(gpu_ctx, tblcases.schema_table(name), tblcases.FILES[name], HOST)[0] for name in ("customer", "orders")}


@pytest.mark.parametrize("chunk_bytes", [0, 1000])
@pytest.mark.parametrize("name", ["customer", "orders"])
def test_fixture_files_parse_on_the_device_without_the_host(gpu_ctx, host_loaded, name, chunk_bytes):
    got, rep = outcome(gpu_ctx, tblcases.schema_table(name), tblcases.FILES[name], DEVICE, chunk_bytes=chunk_bytes)
    assert rep["path"] == 1 and rep["fallback_reason"] == 0
    assert rep["lines_patched"] == 0          # every line of both files is plain: nothing came through the host's line function
    assert rep["rows"] == got[1] == {"customer": 600, "orders": 2500}[name] and rep["text_bytes"] == {"customer": 95421, "orders": 273105}[name]
    assert got == host_loaded[name]


@pytest.mark.parametrize("name", sorted(tblcases.QUERIES))
def test_queries_over_device_loaded_tables(gpu_ctx, name):
    needed, make = tblcases.QUERIES[name]
    schemas = {t: tblcases.schema_table(t) for t in needed}
    texts = []
    for mode in (HOST, DEVICE):
        dev = {t: gpu_ctx.load_tbl(schemas[t], tblcases.FILES[t], mode=mode) for t in needed}
        assert all(d.load_report["path"] == (1 if mode == DEVICE else 0) for d in dev.values())
        plan = make(schemas)
        q = gpu_ctx.compile(plan, [dev[t.name] for t in plan.tables])
        q.execute()
        texts.append(q.result().text)
        q.close()
        for d in dev.values():
            d.close()
    assert texts[0] == texts[1] and len(texts[0].splitlines()) > 1


def _write(tmp_path, lines, newline="\n", last_newline=True):
    p = tmp_path / "odd.tbl"
    p.write_bytes((newline.join(lines) + (newline if last_newline else "")).encode())
    return str(p)


def test_odd_but_accepted_lines_are_patched_by_the_host_function(gpu_ctx, tmp_path):
    path = _write(tmp_path, ACCEPTED)
    want, _ = outcome(gpu_ctx, ODD, path, HOST)
    got, rep = outcome(gpu_ctx, ODD, path, DEVICE)
    assert want[0] == "ok" and got == want
    assert rep["path"] == 1 and rep["lines_patched"] == 2          # by the grammar: lines 2 and 4 (blank / sign / short date; trailing garbage)


@pytest.mark.parametrize("bad", range(len(REJECTED)))
def test_malformed_lines_raise_the_host_paths_error(gpu_ctx, tmp_path, bad):
    path = _write(tmp_path, [ACCEPTED[0], ACCEPTED[1], REJECTED[bad], ACCEPTED[0]])
    want, _ = outcome(gpu_ctx, ODD, path, HOST)
    got, _ = outcome(gpu_ctx, ODD, path, DEVICE)
    assert want[0] == "error" and want[1] == 1 and "Line 2 " in want[2]
    assert got == want


def test_two_bad_lines_report_the_smaller_number(gpu_ctx, tmp_path):
    path = _write(tmp_path, [ACCEPTED[0], REJECTED[3], ACCEPTED[1], REJECTED[4], ACCEPTED[2]])
    want, _ = outcome(gpu_ctx, ODD, path, HOST)
    got, _ = outcome(gpu_ctx, ODD, path, DEVICE)
    assert want[0] == "error" and "Line 1 " in want[2] and got == want


@pytest.mark.parametrize("variant", ["joins_last_field", "ninth_field"])
def test_crlf_files_of_the_odd_schema(gpu_ctx, tmp_path, variant):
    """both CRLF variants of test_tbl_ingest.py: without a trailing terminator the '\\r' joins the last field, behind one it is a ninth field"""
    path = _write(tmp_path, [ACCEPTED[1] if variant == "joins_last_field" else ACCEPTED[0]], newline="\r\n")
    want, _ = outcome(gpu_ctx, ODD, path, HOST)
    got, _ = outcome(gpu_ctx, ODD, path, DEVICE)
    assert want[0] == ("ok" if variant == "joins_last_field" else "error") and got == want
    if variant == "joins_last_field":
        assert want[2]["v"] == b"hello\r\0\0"


@pytest.mark.parametrize("final_newline", [True, False], ids=["nl", "no_nl"])
@pytest.mark.parametrize("shape", tbldevcases.SHAPES)
@pytest.mark.parametrize("kind", ["s1", "s3"])
def test_seams(gpu_ctx, tmp_path, kind, shape, final_newline):
    p = tmp_path / "seam.tbl"
    body = tbldevcases.content(kind, shape, final_newline)
    p.write_bytes(body)
    schema = tbldevcases.SCHEMAS[kind]
    want, _ = outcome(gpu_ctx, schema, str(p), HOST)
    got, rep = outcome(gpu_ctx, schema, str(p), DEVICE)
    assert got == want
    if want[0] == "ok":
        assert rep["path"] == 1 and rep["rows"] == want[1] and rep["text_bytes"] == len(body)
        # by the grammar: a leading blank, a '\r' in a numeric field, an INT of more than nine digits
        odd = sum(1 for l in body.decode().split("\n") if l and (not l[0].isdigit() or l.endswith("\r") or (kind == "s1" and len(l) > 9)))
        assert rep["lines_patched"] == odd
    else:          # the shapes that both paths refuse: an empty line, a '\r' behind the trailing terminator
        assert (shape, final_newline) == ("empty", True) or shape == "crlf_after_terminator"


def test_text_that_does_not_fit_takes_the_host_path(gpu_ctx, host_loaded):
    got, rep = outcome(gpu_ctx, tblcases.schema_table("orders"), tblcases.FILES["orders"], DEVICE, max_device_text_bytes=1024)
    assert rep["path"] == 0 and rep["fallback_reason"] == engine.TBL_FALLBACK_DOES_NOT_FIT
    assert got == host_loaded["orders"]


def test_too_many_odd_lines_take_the_host_path(gpu_ctx, tmp_path):
    p = tmp_path / "blanks.tbl"
    p.write_bytes(b" 1\n" * 65537)
    want, _ = outcome(gpu_ctx, tbldevcases.S1, str(p), HOST)
    got, rep = outcome(gpu_ctx, tbldevcases.S1, str(p), DEVICE)
    assert rep["path"] == 0 and rep["fallback_reason"] == engine.TBL_FALLBACK_ODD_LINES
    assert want[0] == "ok" and want[1] == 65537 and got == want
    # ... and one line fewer is patched on the device path
    p.write_bytes(b" 1\n" * 65536)
    want, _ = outcome(gpu_ctx, tbldevcases.S1, str(p), HOST)
    got, rep = outcome(gpu_ctx, tbldevcases.S1, str(p), DEVICE)
    assert rep["path"] == 1 and rep["lines_patched"] == 65536 and got == want


def test_unusable_terminators_take_the_host_path(gpu_ctx, tmp_path):
    p = tmp_path / "t.tbl"
    p.write_bytes(b"1\n2\n")
    want, _ = outcome(gpu_ctx, tbldevcases.S1, str(p), HOST, terminator="\n")
    got, rep = outcome(gpu_ctx, tbldevcases.S1, str(p), DEVICE, terminator="\n")
    assert rep["path"] == 0 and rep["fallback_reason"] == engine.TBL_FALLBACK_TERMINATOR and got == want and want[1] == 2
    with pytest.raises(engine.EngineError, match="Could not open file"):
        gpu_ctx.load_tbl(tbldevcases.S1, str(tmp_path / "nope.tbl"), mode=DEVICE)


def test_statement_loop_follows_the_contexts_setting(tmp_path):
    """create table, two bulk inserts (the second appends), a select: the same messages and result text with tbl_ingest 1 as with 0"""
    body = tbldevcases.content("s3", "lines_513", True)
    (tmp_path / "a.tbl").write_bytes(body)
    (tmp_path / "b.tbl").write_bytes(tbldevcases.content("s3", "odd_first", False))
    seen = []
    for setting in (0, 1):
        ctx = engine.Context(device=0, tbl_ingest=setting, arena_reserve_bytes=-1)
        try:
            db = engine.Database(ctx)
            msgs = []
            db.execute("create table s3 ( i int, c char(5), d decimal(12,2) )")
            msgs.append(db.message)
            for f in ("a.tbl", "b.tbl"):
                db.execute(f'bulk insert s3 from "{tmp_path}/{f}" with ( fieldterminator="|" )')
                msgs.append(db.message)
                rep = db.load_report
                assert rep["path"] == setting and rep["rows"] == (513 if f == "a.tbl" else 40)
                assert rep["lines_patched"] == (1 if setting == 1 and f == "b.tbl" else 0)
            res = db.execute("select c, count(*) as n, sum(d) as total, max(d) as hi from s3 group by c")
            rows = db.execute("select i, c, d from s3 where i < 200 order by i")
            seen.append((msgs, res.text, rows.text))
            db.close()
        finally:
            ctx.close()
    assert seen[0] == seen[1]
    assert seen[0][0] == ["Created table s3\n", "Inserted 513 tuples\n", "Inserted 40 tuples\n"] and len(seen[0][1].splitlines()) > 10
