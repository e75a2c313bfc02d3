"""The host's part of a dictionary-coded key in the device tail (resql_amd/csrc/dense_groups.h): the entries' hash terms and the classes
of entries equal up to trailing spaces, as a program of its own under the sanitizers.  No device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hash_terms_and_class_maps_of_a_coded_key(tmp_path):
    """tests/cpp/dense_tail_keys_test.cpp: terms against sums computed by hand for CHAR and VARCHAR (the empty entry, a full-width one,
    'ab' against 'ab ', a byte >= 0x80, anagrams), class maps for a class of three, a key without classes and a single entry"""
    exe = str(tmp_path / "dense_tail_keys_test")
    src = os.path.join(ROOT, "resql_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + src, "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "dense_tail_keys_test.cpp"), os.path.join(src, "hostpar.cpp"), "-lpthread", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "dense_tail_keys_test ok" in out.stdout
