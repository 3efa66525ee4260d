"""The helpers the host comparators share (tools/cpu_common.hpp: the key compare,
the range split over threads, the little-endian load) as plain host C++:
tests/cpp/test_cpu_common.cpp, a stand-alone program, built with g++ once plain
and once under AddressSanitizer + UndefinedBehaviorSanitizer.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_cpu_common(tmp_path, sanitize):
    exe = os.path.join(str(tmp_path), "test_cpu_common")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-pthread", *flags, "-I", os.path.join(ROOT, "tools"),
                           os.path.join(ROOT, "tests", "cpp", "test_cpu_common.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr[-3000:]
