"""AddressSanitizer + UndefinedBehaviorSanitizer build of the scan merge's host side (csrc/scan_merge_check.cpp) with a driver that
feeds it an accept table, truncated, overlapping, out-of-range and decreasing-image tables, huge counts and the ends of int32 and
int64 on exactly-sized tables and message buffers (tests/native/scan_merge_check_sanitize.cpp).  CPU only, a stand-alone program:
nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_scan_merge_check_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "scan_merge_check_sanitize")
    # the sanitizers' runtimes are linked into the program itself, so it does not matter what else the loader brings in before it
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "rock-art-radnet_amd", "csrc", "scan_merge_check.cpp"), os.path.join(ROOT, "tests", "native", "scan_merge_check_sanitize.cpp"),
           "-o", exe]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
