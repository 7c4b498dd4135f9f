"""The plain-C++ part of the layer under the dCor, HSIC and n^2 test handles
(midagma_amd/csrc/coltest.h: bad_shape, listed_columns, NullCount) built with
g++ -fsanitize=address,undefined and run as a stand-alone program (tests/abi/coltest_test.cpp).
CPU only: the header's first part reads no HIP header."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "midagma_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_coltest_layer_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "coltest_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
           os.path.join(REPO, "tests", "abi", "coltest_test.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "AddressSanitizer on" in r.stdout and "all checks passed" in r.stdout
