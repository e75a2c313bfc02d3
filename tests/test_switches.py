"""The table of environment switches (resql_amd/csrc/switches.h) on the host: a C++ driver sets and unsets every kind of row and compares the
readers with the values the expressions they replaced gave (tests/cpp/switches_test.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_readers_parse_what_the_replaced_expressions_parsed(tmp_path):
    exe = str(tmp_path / "switches_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "resql_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "switches_test.cpp"), "-o", exe])
    env = {k: v for k, v in os.environ.items() if not k.startswith("RSQ_")}
    out = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "switches_test ok" in out.stdout
