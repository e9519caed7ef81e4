"""AddressSanitizer + UndefinedBehaviorSanitizer build of the device inflate's host side (csrc/inflate_plan.cpp) with a driver that
chains unit tables in exactly-sized buffers, meets every refusal once and sums chunk CRCs on threads (tests/native/inflate_plan_sanitize.cpp).  CPU only, a
stand-alone program: nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_inflate_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "inflate_plan_sanitize")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-pthread",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "rock-art-radnet_amd", "csrc", "inflate_plan.cpp"),
           os.path.join(ROOT, "tests", "native", "inflate_plan_sanitize.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
