"""AddressSanitizer + UndefinedBehaviorSanitizer build of the launch plan of radnet_conv_wgrad_multi (csrc/wgrad_multi_plan.cpp) with a
driver that checks the prefix sums, the grouping by tile shape, the 16-problem cap that spills into a further launch, the slab and
counter placement and the refusals, on exactly-sized buffers (tests/native/wgrad_multi_plan_sanitize.cpp).  CPU only, a stand-alone
program: nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_wgrad_multi_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "wgrad_multi_plan_sanitize")
    csrc = os.path.join(ROOT, "rock-art-radnet_amd", "csrc")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-I", csrc, os.path.join(csrc, "wgrad_multi_plan.cpp"), os.path.join(ROOT, "tests", "native", "wgrad_multi_plan_sanitize.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
