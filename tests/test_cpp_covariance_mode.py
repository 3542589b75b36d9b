"""Builds tests/cpp/covariance_mode_test.cpp with plain g++ from that file and ml_amd/csrc/host/em_math.cpp alone (no HIP, no
libmlhip.so) and runs it: the covariance mode's host functions -- the checked conversion from the ABI's int, covariance_doubles, and the
two conversions between a mode's covariance array and K full matrices, bit for bit against loops written in the test (the ascending-k
order of the tied pooling is part of the results' bits). No GPU.
-ffp-contract=off, like the library's own build: the test's reference loop must round every product before it is added."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ml_amd", "csrc")
EXE = os.path.join(ROOT, "tests", "cpp", "covariance_mode_test")


def _build():
    src = os.path.join(ROOT, "tests", "cpp", "covariance_mode_test.cpp")
    math = os.path.join(CSRC, "host", "em_math.cpp")
    deps = [src, math, os.path.join(CSRC, "host", "em_math.hpp"), os.path.join(CSRC, "host", "team.hpp"),
            os.path.join(CSRC, "device", "layout.hpp")]
    if os.path.exists(EXE) and os.path.getmtime(EXE) > max(os.path.getmtime(d) for d in deps):
        return
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-pthread", "-I", CSRC, src, math, "-o", EXE])


def test_covariance_mode_host_functions():
    _build()
    out = subprocess.run([EXE], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "covariance_mode_test: ok (9 shapes)" in out.stdout
