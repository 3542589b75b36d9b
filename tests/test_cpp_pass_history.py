"""Builds tests/cpp/pass_history_test.cpp with plain g++ from that file and ml_amd/csrc/runtime/pass_history.hpp alone (no HIP, no
libmlhip.so) and runs it: the ring of the last three passes and the two route choices of a fit that read it -- the sparse or the dense
statistics kernel, the screened or the dense E-step -- and the report of mlhip_em_screen_counts, against tables written out by hand from
the rules (first passes, the bound at 16000 / 16001, a stale slot, wrap-around, a change of K, forced routes). The same program is
built and run a second time with -fsanitize=address,undefined: a stand-alone program with its own main. No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ml_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "pass_history_test.cpp")
DEPS = [SRC, os.path.join(CSRC, "runtime", "pass_history.hpp")]


def _build(exe, extra):
    """None, or the compiler's complaint."""
    if os.path.exists(exe) and os.path.getmtime(exe) > max(os.path.getmtime(d) for d in DEPS):
        return None
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", CSRC] + extra + [SRC, "-o", exe], capture_output=True, text=True)
    return out.stderr if out.returncode else None


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "pass_history_test: ok (112 checks)" in out.stdout
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr


def test_pass_history():
    exe = os.path.join(ROOT, "tests", "cpp", "pass_history_test")
    complaint = _build(exe, [])
    assert complaint is None, complaint[-3000:]
    _run(exe)


def test_pass_history_under_address_and_undefined_sanitizers():
    if os.environ.get("MLHIP_LIBRARY"):
        pytest.skip("already inside a sanitizer run (tests/test_sanitizers.py): its preloaded runtime is another compiler's")
    exe = os.path.join(ROOT, "tests", "cpp", "pass_history_test_san")
    complaint = _build(exe, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if complaint is not None:
        if "cannot find" in complaint or "unrecognized" in complaint:
            pytest.skip("this toolchain has no runtime for -fsanitize=address,undefined")
        raise AssertionError(complaint[-3000:])
    _run(exe)
