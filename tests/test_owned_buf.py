"""The owning buffer type behind every device and pinned allocation (midagma_amd/csrc/owned_buf.h:
grow-only alloc, alloc_shifted, idempotent release, move-only, frees itself) built with
g++ -fsanitize=address,undefined over a malloc-backed, byte-counting policy and run as a stand-alone
program (tests/owned/owned_test.cpp).  CPU only."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "midagma_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_owned_buf_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "owned_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
           os.path.join(REPO, "tests", "owned", "owned_test.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "AddressSanitizer on" in r.stdout and "all checks passed, live bytes at exit 0" in r.stdout
