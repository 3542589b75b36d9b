"""Builds tests/cpp/kmeans_weighted_fit_test.cpp with plain g++ against include/ML/*.hpp + libmlhip.so and runs it:
KMeans::fit(data, weights) of the C++ facade, and (-DWEIGHTED_EIGEN, include/eigen_api first) the same overload of the Eigen-typed
API against tests/cpp/eigen_shim. Host mode (argument errors, refused before any device work) on CPU, the weighted fit against the
replicated sample's on the GPU box."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "kmeans_weighted_fit_test.cpp")
EXE = {False: os.path.join(ROOT, "tests", "cpp", "kmeans_weighted_fit_test"),
       True: os.path.join(ROOT, "tests", "cpp", "kmeans_weighted_fit_eigen_test")}


def _build(eigen):
    exe = EXE[eigen]
    deps = [SRC, os.path.join(ROOT, "ml_amd", "libmlhip.so"), os.path.join(ROOT, "include", "ML", "KMeans.hpp"),
            os.path.join(ROOT, "include", "ML", "EigenApi.hpp")]
    if os.path.exists(exe) and os.path.getmtime(exe) > max(os.path.getmtime(d) for d in deps):
        return exe
    extra = ["-DWEIGHTED_EIGEN", "-I", os.path.join(ROOT, "tests", "cpp", "eigen_shim"), "-I", os.path.join(ROOT, "include", "eigen_api")] if eigen else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra"] + extra + ["-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                           "-L", os.path.join(ROOT, "ml_amd"), "-lmlhip", "-Wl,-rpath," + os.path.join(ROOT, "ml_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.parametrize("eigen", [False, True], ids=["facade", "eigen"])
def test_kmeans_weighted_fit_overload_host_paths(eigen):
    out = subprocess.run([_build(eigen), "host"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("eigen", [False, True], ids=["facade", "eigen"])
def test_kmeans_weighted_fit_overload_on_the_gpu(eigen):
    out = subprocess.run([_build(eigen), "gpu"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
