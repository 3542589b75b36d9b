"""Builds tests/cpp/silhouette_test.cpp with plain g++ twice -- against include/ML/Clustering.hpp, include/ML/EM.hpp + libmlhip.so, and
with -DSILHOUETTE_TEST_EIGEN against the Eigen-typed API (include/ML/EigenApi.hpp through include/eigen_api, tests/cpp/eigen_shim) --
and runs both: Clustering::silhouette_samples / silhouette_score of either surface give the bits of mlpp_silhouette_samples, EM::bic /
aic the bits of their formulas on mean_log_density; argument errors throw std::invalid_argument before any device work, and the
parameter count of an exact fit needs no device. Host mode on the CPU, the rest where an MI355X is present."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "silhouette_test.cpp")
LIB = os.path.join(ROOT, "ml_amd", "libmlhip.so")
EXE = os.path.join(ROOT, "tests", "cpp", "silhouette_test")
EIGEN_EXE = os.path.join(ROOT, "tests", "cpp", "silhouette_eigen_test")
LINK = ["-L", os.path.join(ROOT, "ml_amd"), "-lmlhip", "-Wl,-rpath," + os.path.join(ROOT, "ml_amd"), "-Wl,-rpath,/opt/rocm/lib"]


def _stale(exe, deps):
    return not os.path.exists(exe) or os.path.getmtime(exe) <= max(os.path.getmtime(d) for d in deps)


def _build():
    if _stale(EXE, [SRC, LIB, os.path.join(ROOT, "include", "ML", "EM.hpp"), os.path.join(ROOT, "include", "ML", "Clustering.hpp")]):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), SRC, "-o", EXE] + LINK)


def _build_eigen():
    deps = [SRC, LIB, os.path.join(ROOT, "include", "ML", "EigenApi.hpp"), os.path.join(ROOT, "tests", "cpp", "eigen_shim", "Eigen", "Core")]
    if _stale(EIGEN_EXE, deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-DSILHOUETTE_TEST_EIGEN",
                               "-I", os.path.join(ROOT, "tests", "cpp", "eigen_shim"), "-I", os.path.join(ROOT, "include", "eigen_api"),
                               "-I", os.path.join(ROOT, "include"), SRC, "-o", EIGEN_EXE] + LINK)


def _run(exe, mode):
    out = subprocess.run([exe, mode], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


def test_cpp_silhouette_host_paths():
    _build()
    _run(EXE, "host")


def test_eigen_typed_silhouette_host_paths():
    _build_eigen()
    _run(EIGEN_EXE, "host")


@pytest.mark.gpu
def test_cpp_silhouette_gives_the_bits_of_the_c_surface():
    _build()
    _run(EXE, "gpu")


@pytest.mark.gpu
def test_eigen_typed_silhouette_gives_the_bits_of_the_c_surface():
    _build_eigen()
    _run(EIGEN_EXE, "gpu")
