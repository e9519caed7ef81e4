"""AddressSanitizer + UndefinedBehaviorSanitizer build of radnet_inflate_lz_chain (csrc/inflate_plan.cpp) with a driver that chains
unit tables in exactly-sized buffers: an accepted table, every refusal once, an unsorted table, a link table too small, the reach at
0, at the offset and one beyond it (tests/native/inflate_lz_plan_sanitize.cpp).  CPU only, a stand-alone program with its own main:
nothing is loaded into python, and the child's environment is the parent's, untouched."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
@pytest.mark.skipif(bool(os.environ.get("LD_PRELOAD")), reason="LD_PRELOAD is set: a sanitized program wants its runtime first")
def test_inflate_lz_chain_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "inflate_lz_plan_sanitize")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-pthread",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "rock-art-radnet_amd", "csrc", "inflate_plan.cpp"),
           os.path.join(ROOT, "tests", "native", "inflate_lz_plan_sanitize.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
