"""The plain field forms the device ingest parses (resql_amd/csrc/tbl_fields.h) against the host path's line function
(tbl.cpp tblParseLine), on the host: a C++ driver (tests/cpp/tbl_fields_test.cpp) built with g++.  The driver gets every field of
test_tbl_ingest.py's ACCEPTED / REJECTED lines and runs each of them, a fixed edge list and 20 000 seeded fields through every
type category."""
import os
import subprocess

import test_tbl_ingest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_forms_agree_with_the_host_line_function(tmp_path):
    fields = sorted({f for line in test_tbl_ingest.ACCEPTED + test_tbl_ingest.REJECTED for f in line.split("|")})
    listed = tmp_path / "fields.hex"
    listed.write_text("".join(f.encode().hex() + "\n" for f in fields))
    exe = str(tmp_path / "tbl_fields_test")
    src = os.path.join(ROOT, "resql_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-I" + src, "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "tbl_fields_test.cpp"), os.path.join(src, "tbl.cpp"), os.path.join(src, "expr.cpp"),
                           "-o", exe])
    out = subprocess.run([exe, str(listed)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "tbl_fields_test ok" in out.stdout
