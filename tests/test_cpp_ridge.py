"""Builds tests/cpp/ridge_fit_test.cpp with plain g++ against include/ML/*.hpp + libmlhip.so and runs it: the covariance
regularisation of the C++ facade (EM::set_covariance_regularisation / covariance_regularisation); and
tests/cpp/ridge_fit_eigen_test.cpp, the same methods of the Eigen-typed API (include/ML/EigenApi.hpp) against tests/cpp/eigen_shim.
Host mode (default, round trip, std::domain_error) on CPU; the fits of a collinear sample in the three covariance types on the GPU box."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "ridge_fit_test")


def _build():
    src = os.path.join(ROOT, "tests", "cpp", "ridge_fit_test.cpp")
    deps = [src, os.path.join(ROOT, "ml_amd", "libmlhip.so"), os.path.join(ROOT, "include", "ML", "EM.hpp")]
    if os.path.exists(EXE) and os.path.getmtime(EXE) > max(os.path.getmtime(d) for d in deps):
        return
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), src,
                           "-o", EXE, "-L", os.path.join(ROOT, "ml_amd"), "-lmlhip",
                           "-Wl,-rpath," + os.path.join(ROOT, "ml_amd"), "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_covariance_regularisation_host_paths():
    _build()
    out = subprocess.run([EXE, "host"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


@pytest.mark.gpu
def test_cpp_regularised_fits_of_a_collinear_sample():
    _build()
    out = subprocess.run([EXE, "gpu"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


EIGEN_EXE = os.path.join(ROOT, "tests", "cpp", "ridge_fit_eigen_test")


def _build_eigen():
    src = os.path.join(ROOT, "tests", "cpp", "ridge_fit_eigen_test.cpp")
    deps = [src, os.path.join(ROOT, "ml_amd", "libmlhip.so"), os.path.join(ROOT, "include", "ML", "EigenApi.hpp"),
            os.path.join(ROOT, "tests", "cpp", "eigen_shim", "Eigen", "Core")]
    if os.path.exists(EIGEN_EXE) and os.path.getmtime(EIGEN_EXE) > max(os.path.getmtime(d) for d in deps):
        return
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "tests", "cpp", "eigen_shim"),
                           "-I", os.path.join(ROOT, "include", "eigen_api"), "-I", os.path.join(ROOT, "include"), src, "-o", EIGEN_EXE,
                           "-L", os.path.join(ROOT, "ml_amd"), "-lmlhip", "-Wl,-rpath," + os.path.join(ROOT, "ml_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])


def test_eigen_typed_covariance_regularisation_host_paths():
    _build_eigen()
    out = subprocess.run([EIGEN_EXE, "host"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


@pytest.mark.gpu
def test_eigen_typed_regularised_fits_of_a_collinear_sample():
    _build_eigen()
    out = subprocess.run([EIGEN_EXE, "gpu"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
