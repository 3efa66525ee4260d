"""The admission arithmetic (csrc/admit_dev.hpp: the IsLegal compare, the bucket
and its ranges, window membership, the state after rank w in either kind of
window, the upper-bound step) as plain host C++:
tests/cpp/test_admit_layer.cpp, a stand-alone program, built with g++ once
plain and once under AddressSanitizer + UndefinedBehaviorSanitizer.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_admit_layer_cpu(tmp_path, sanitize):
    exe = os.path.join(str(tmp_path), "test_admit_layer")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", *flags, "-I", os.path.join(ROOT, "nakevaleng_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_admit_layer.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr[-3000:]
