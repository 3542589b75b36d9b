"""Builds tests/cpp/estep_screen_bound_test.cpp with plain g++ from that file and ml_amd/csrc/device/em_screen_bound.hpp alone (no HIP,
no libmlhip.so) and runs it: the bound constants of the screened E-step in their host form against a long double evaluation of the
true new log-responsibilities (see the file's head). Once more as a stand-alone program under -fsanitize=address,undefined (skipped
where the toolchain lacks the runtime, and inside the run of tests/test_sanitizers.py). No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ml_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "estep_screen_bound_test.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "estep_screen_bound_test")


def test_bound_constants_hold():
    deps = [SRC, os.path.join(CSRC, "device", "em_screen_bound.hpp")]
    if not (os.path.exists(EXE) and os.path.getmtime(EXE) > max(os.path.getmtime(d) for d in deps)):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-I", CSRC, SRC, "-o", EXE])
    out = subprocess.run([EXE], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "estep_screen_bound_test: ok" in out.stdout


def test_bound_constants_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "estep_screen_bound_test")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if os.environ.get("MLHIP_LIBRARY"):
        pytest.skip("already inside a sanitizer run (tests/test_sanitizers.py): its preloaded runtime is another compiler's")
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *flags, "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True)
    if out.returncode != 0:
        if "cannot find" in out.stderr or "unrecognized" in out.stderr:
            pytest.skip("this toolchain has no runtime for " + " ".join(flags))
        raise AssertionError(out.stderr[-3000:])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1 halt_on_error=1")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0 and "estep_screen_bound_test: ok" in run.stdout, (run.stdout + run.stderr)[-4000:]
