"""The environment switches the library reads are the rows of resql_amd/csrc/switches.h - the only place that reads the environment - and
every one of them is flipped on the GPU: over the seeded plans of tests/test_gpu_knobs.py, or by the test file named here (CPU check of the list)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "resql_amd", "csrc")

# switches flipped by a file of their own rather than over the seeded plans: the file that sets each
# (RSQ_KCACHE_USED_LOG selects nothing: __graft_entry__.build() sets it to learn which code objects the build resolves, and prunes the rest)
ELSEWHERE = {
    "RSQ_DEVICE_TAIL_MIN": "tests/test_gpu_device_tail.py",
    "RSQ_FORCE_GENERIC": "tests/test_gpu_generic_pipeline.py",
    "RSQ_MULTI_GENERAL_MERGE": "tests/test_gpu_multi.py",
    "RSQ_NARROW_SCANS": "tests/test_gpu_narrow_scan.py",
    "RSQ_DICT_SCANS": "tests/test_gpu_dict_scan.py",
    "RSQ_MAX_GRID": "tests/test_gpu_narrow_edges.py",
    "RSQ_KCACHE_USED_LOG": "__graft_entry__.py",
}
# preprocessor macros of the generated kernels, written into their text as "#define RSQ_...": not environment variables
MACROS = {"RSQ_CQ_NV", "RSQ_LC_SLOTS"}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _table():
    rows = re.findall(r"^    X\((RSQ_[A-Z0-9_]+),", _read("resql_amd", "csrc", "switches.h"), re.M)
    assert len(rows) == len(set(rows))
    return set(rows)


def _sources():
    return [f for f in sorted(os.listdir(SRC)) if f.endswith((".cpp", ".hip", ".h"))]


def test_only_switches_h_reads_the_environment():
    for f in _sources():
        if f != "switches.h":
            assert "getenv" not in _read("resql_amd", "csrc", f), f


def test_no_switch_name_is_spelled_outside_the_table():
    """a quoted "RSQ_..." outside switches.h would be a switch read (or documented) behind the table's back"""
    for f in _sources():
        if f != "switches.h":
            found = set(re.findall(r'"(RSQ_[A-Z0-9_]+)"', _read("resql_amd", "csrc", f)))
            assert found <= MACROS, (f, sorted(found - MACROS))


def test_the_switch_list_is_complete():
    """the table's rows == the switches flipped in tests/test_gpu_knobs.py plus the ones other files flip, each of which does set it; 31 of them
    (the cap of 30 this replaces counted 28 switches and the two macros, and missed the three switches then read in engine.h)"""
    table = _table()
    flipped = set(re.findall(r'^    \("(RSQ_[A-Z0-9_]+)", "', _read("tests", "test_gpu_knobs.py"), re.M))
    assert not flipped & set(ELSEWHERE), sorted(flipped & set(ELSEWHERE))
    assert table == flipped | set(ELSEWHERE), sorted(table ^ (flipped | set(ELSEWHERE)))
    for name, path in ELSEWHERE.items():
        assert re.search(r'(setenv\("%s", |environ\["%s"\] = )' % (name, name), _read(*path.split("/"))), (name, path)
    assert len(table) == 31


def test_design_lists_every_switch():
    design = _read("DESIGN.md")
    start = design.index("### Environment switches")
    section = design[start:design.index("\n## ", start)]
    missing = sorted(n for n in _table() if not re.search(r"\b%s\b" % n, section))
    assert not missing, missing
    assert "### Environment switches (31," in section
