"""The text of a result cell as the device writes it (resql_amd/csrc/result_text.h) against the host's definition - serializeSqlValue over
loadValue, and serializeResultView for whole rows - on the host: a C++ driver (tests/cpp/result_text_test.cpp) built with g++ and the
address / undefined-behaviour sanitizers.  The driver runs a fixed edge list and 20 000 seeded values through every type category and
hands the header heap blocks of exactly the bytes it may read and write."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cell_text_agrees_with_the_host_serializer(tmp_path):
    exe = str(tmp_path / "result_text_test")
    src = os.path.join(ROOT, "resql_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-I" + src, "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "result_text_test.cpp"), os.path.join(src, "hostref.cpp"), os.path.join(src, "hostpar.cpp"),
                           os.path.join(src, "expr.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "result_text_test ok" in out.stdout
