"""AddressSanitizer + UndefinedBehaviorSanitizer build of the LZ deflate's host side (csrc/deflate_plan.cpp:
radnet_deflate_build_codes_lz, radnet_deflate_lz_piece_cap, radnet_deflate_stream_bits) with a driver that runs them on empty,
single-symbol, skewed (deeper than 15), all-30-distances and maximal histograms in exactly-sized buffers
(tests/native/deflate_lz_plan_sanitize.cpp).  CPU only, a stand-alone program: nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_deflate_lz_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "deflate_lz_plan_sanitize")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "rock-art-radnet_amd", "csrc", "deflate_plan.cpp"),
           os.path.join(ROOT, "tests", "native", "deflate_lz_plan_sanitize.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
