"""Builds tests/cpp/impute_test.cpp with plain g++ twice -- against include/ML/EM.hpp + libmlhip.so, and with -DIMPUTE_TEST_EIGEN
against the Eigen-typed API (include/ML/EigenApi.hpp through include/eigen_api, tests/cpp/eigen_shim) -- and runs both: EM::impute
of either surface gives the bits of mlpp_em_impute (imputed block, log-densities, responsibilities), observed entries keep their
bits, no points give a d x 0 matrix, a wrong number of rows std::invalid_argument. Host mode (the model that was never fitted,
mlhip_em_impute_plan, mlhip_em_impute_route) on CPU, fitted models on the GPU box."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "impute_test.cpp")
LIB = os.path.join(ROOT, "ml_amd", "libmlhip.so")
EXE = os.path.join(ROOT, "tests", "cpp", "impute_test")
EIGEN_EXE = os.path.join(ROOT, "tests", "cpp", "impute_eigen_test")
LINK = ["-L", os.path.join(ROOT, "ml_amd"), "-lmlhip", "-Wl,-rpath," + os.path.join(ROOT, "ml_amd"), "-Wl,-rpath,/opt/rocm/lib"]


def _stale(exe, deps):
    return not os.path.exists(exe) or os.path.getmtime(exe) <= max(os.path.getmtime(d) for d in deps)


def _build():
    if _stale(EXE, [SRC, LIB, os.path.join(ROOT, "include", "ML", "EM.hpp")]):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), SRC, "-o", EXE] + LINK)


def _build_eigen():
    deps = [SRC, LIB, os.path.join(ROOT, "include", "ML", "EigenApi.hpp"), os.path.join(ROOT, "tests", "cpp", "eigen_shim", "Eigen", "Core")]
    if _stale(EIGEN_EXE, deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-DIMPUTE_TEST_EIGEN",
                               "-I", os.path.join(ROOT, "tests", "cpp", "eigen_shim"), "-I", os.path.join(ROOT, "include", "eigen_api"),
                               "-I", os.path.join(ROOT, "include"), SRC, "-o", EIGEN_EXE] + LINK)


def _run(exe, mode):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MLHIP_IMPUTE")}
    out = subprocess.run([exe, mode], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout + out.stderr


def test_cpp_impute_host_paths():
    _build()
    _run(EXE, "host")


def test_eigen_typed_impute_host_paths():
    _build_eigen()
    _run(EIGEN_EXE, "host")


@pytest.mark.gpu
def test_cpp_impute_gives_the_bits_of_the_c_surface():
    _build()
    _run(EXE, "gpu")


@pytest.mark.gpu
def test_eigen_typed_impute_gives_the_bits_of_the_c_surface():
    _build_eigen()
    _run(EIGEN_EXE, "gpu")
