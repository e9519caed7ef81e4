"""AddressSanitizer + UndefinedBehaviorSanitizer build of the IDAT join's host side (csrc/png_join_plan.cpp) with a driver that feeds
it accept tables, one refuse table per reason and the ends of int64 on exactly-sized tables and message buffers
(tests/native/png_join_plan_sanitize.cpp).  CPU only, a stand-alone program: nothing is loaded into python, and the program runs in
the environment as it is."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_png_join_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "png_join_plan_sanitize")
    csrc = os.path.join(ROOT, "rock-art-radnet_amd", "csrc")
    # the sanitizers' runtimes are linked into the program itself, so it does not matter what else the loader brings in before it
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(csrc, "png_join_plan.cpp"),
           os.path.join(ROOT, "tests", "native", "png_join_plan_sanitize.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
