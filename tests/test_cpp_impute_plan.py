"""Builds tests/cpp/impute_plan_test.cpp with plain g++ from that file, ml_amd/csrc/host/impute_plan.cpp and host/em_math.cpp alone (no
HIP, no libmlhip.so) and runs it: the host plan of mlhip_em_impute -- masks, the stable order by pattern, the group bounds, the tiles
and their padding classes -- on N = 0, 1, 65, 1000 x d = 1, 3, 32, 33, 70 and four kinds of blocks. The same program is built and
run a second time with -fsanitize=address,undefined: a stand-alone program with its own main. No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ml_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "impute_plan_test.cpp")
SOURCES = [SRC, os.path.join(CSRC, "host", "impute_plan.cpp"), os.path.join(CSRC, "host", "em_math.cpp")]
DEPS = SOURCES + [os.path.join(CSRC, "host", name) for name in ("impute_plan.hpp", "em_math.hpp", "team.hpp")] + [os.path.join(CSRC, "device", "layout.hpp")]


def _build(exe, extra):
    """None, or the compiler's complaint."""
    if os.path.exists(exe) and os.path.getmtime(exe) > max(os.path.getmtime(d) for d in DEPS):
        return None
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-pthread", "-I", CSRC] + extra + SOURCES + ["-o", exe],
                         capture_output=True, text=True)
    return out.stderr if out.returncode else None


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "impute_plan_test: ok (81 blocks)" in out.stdout
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr


def test_impute_plan():
    exe = os.path.join(ROOT, "tests", "cpp", "impute_plan_test")
    complaint = _build(exe, [])
    assert complaint is None, complaint[-3000:]
    _run(exe)


def test_impute_plan_under_address_and_undefined_sanitizers():
    if os.environ.get("MLHIP_LIBRARY"):
        pytest.skip("already inside a sanitizer run (tests/test_sanitizers.py): its preloaded runtime is another compiler's")
    exe = os.path.join(ROOT, "tests", "cpp", "impute_plan_test_san")
    complaint = _build(exe, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if complaint is not None:
        if "cannot find" in complaint or "unrecognized" in complaint:
            pytest.skip("this toolchain has no runtime for -fsanitize=address,undefined")
        raise AssertionError(complaint[-3000:])
    _run(exe)
