"""AddressSanitizer + UndefinedBehaviorSanitizer build of the CRC-32 kernels' host side (csrc/crc32_plan.cpp over csrc/crc32_rule.h)
with a driver that feeds it accept tables, one refuse table per bound and the ends of int64 on exactly-sized tables and message
buffers (tests/native/crc32_plan_sanitize.cpp).  CPU only, a stand-alone program: nothing is loaded into python, and the program
runs in the environment as it is."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_crc32_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "crc32_plan_sanitize")
    csrc = os.path.join(ROOT, "rock-art-radnet_amd", "csrc")
    # the sanitizers' runtimes are linked into the program itself, so it does not matter what else the loader brings in before it
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(csrc, "crc32_plan.cpp"),
           os.path.join(ROOT, "tests", "native", "crc32_plan_sanitize.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
