"""Builds tests/cpp/condition_sample_test.cpp with plain g++ twice -- against include/ML/EM.hpp + libmlhip.so, and with
-DCONDITION_TEST_EIGEN against the Eigen-typed API (include/ML/EigenApi.hpp through include/eigen_api, tests/cpp/eigen_shim) -- and
runs both: EM::conditional_samples and EM::conditional_covariances of either surface give the bits of mlpp_em_conditional_samples and
mlpp_em_conditional_covariances, no points or no draws a dM x 0 matrix, bad arguments std::invalid_argument. Host mode (the model that
was never fitted, mlhip_em_condition_covariances) on CPU, fitted models on the GPU box. Also: the host helper
(ml_amd/csrc/host/em_math.cpp) with tests/cpp/condition_covariance_host_main.cpp as a stand-alone program under
-fsanitize=address,undefined (skipped where the toolchain lacks the runtime, and inside the run of tests/test_sanitizers.py)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "condition_sample_test.cpp")
LIB = os.path.join(ROOT, "ml_amd", "libmlhip.so")
EXE = os.path.join(ROOT, "tests", "cpp", "condition_sample_test")
EIGEN_EXE = os.path.join(ROOT, "tests", "cpp", "condition_sample_eigen_test")
LINK = ["-L", os.path.join(ROOT, "ml_amd"), "-lmlhip", "-Wl,-rpath," + os.path.join(ROOT, "ml_amd"), "-Wl,-rpath,/opt/rocm/lib"]


def _stale(exe, deps):
    return not os.path.exists(exe) or os.path.getmtime(exe) <= max(os.path.getmtime(d) for d in deps)


def _build():
    if _stale(EXE, [SRC, LIB, os.path.join(ROOT, "include", "ML", "EM.hpp")]):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), SRC, "-o", EXE] + LINK)


def _build_eigen():
    deps = [SRC, LIB, os.path.join(ROOT, "include", "ML", "EigenApi.hpp"), os.path.join(ROOT, "tests", "cpp", "eigen_shim", "Eigen", "Core")]
    if _stale(EIGEN_EXE, deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-DCONDITION_TEST_EIGEN",
                               "-I", os.path.join(ROOT, "tests", "cpp", "eigen_shim"), "-I", os.path.join(ROOT, "include", "eigen_api"),
                               "-I", os.path.join(ROOT, "include"), SRC, "-o", EIGEN_EXE] + LINK)


def _run(exe, mode):
    out = subprocess.run([exe, mode], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


def test_cpp_condition_sample_host_paths():
    _build()
    _run(EXE, "host")


def test_eigen_typed_condition_sample_host_paths():
    _build_eigen()
    _run(EIGEN_EXE, "host")


def test_host_condition_covariances_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "condition_covariance_host_main")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if os.environ.get("MLHIP_LIBRARY"):
        pytest.skip("already inside a sanitizer run (tests/test_sanitizers.py): its preloaded runtime is another compiler's")
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *flags, "-I", os.path.join(ROOT, "ml_amd", "csrc"),
                          os.path.join(ROOT, "tests", "cpp", "condition_covariance_host_main.cpp"),
                          os.path.join(ROOT, "ml_amd", "csrc", "host", "em_math.cpp"), "-o", exe, "-pthread"], capture_output=True, text=True)
    if out.returncode != 0:
        if "cannot find" in out.stderr or "unrecognized" in out.stderr:
            pytest.skip("this toolchain has no runtime for " + " ".join(flags))
        raise AssertionError(out.stderr[-3000:])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1 halt_on_error=1")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    print(run.stdout)
    assert run.returncode == 0 and "condition covariance host ok" in run.stdout, (run.stdout + run.stderr)[-4000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr


@pytest.mark.gpu
def test_cpp_condition_sample_gives_the_bits_of_the_c_surface():
    _build()
    _run(EXE, "gpu")


@pytest.mark.gpu
def test_eigen_typed_condition_sample_gives_the_bits_of_the_c_surface():
    _build_eigen()
    _run(EIGEN_EXE, "gpu")
