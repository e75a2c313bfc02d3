"""The packing rule of the register aggregation's second form (resql_amd/csrc/row_cells.h) on the host: a C++ driver checks over random
envelopes, row counts and grids that the fields of a word are disjoint, that the largest sum the bound allows fits its field, that one
row more is refused, and that the bound covers the rows the kernel's loops deal to a lane's word (tests/cpp/row_cells_test.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fields_are_disjoint_and_the_bound_holds(tmp_path):
    exe = str(tmp_path / "row_cells_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "resql_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "row_cells_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "row_cells_test ok" in out.stdout
