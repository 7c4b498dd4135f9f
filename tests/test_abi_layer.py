"""The entry-point layer every C handle family shares (midagma_amd/csrc/abi.h: the per-family
message slots, abi_fail / abi_last_error, abi_guarded with its device hook, classify) built with
g++ -fsanitize=address,undefined over stand-in handle types and run as a stand-alone program
(tests/abi/abi_test.cpp).  CPU only: the header's first part reads no HIP header."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "midagma_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_abi_layer_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "abi_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-pthread", "-I", CSRC,
           os.path.join(REPO, "tests", "abi", "abi_test.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "AddressSanitizer on" in r.stdout and "all checks passed" in r.stdout
