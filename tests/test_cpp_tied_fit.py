"""Builds tests/cpp/tied_fit_test.cpp with plain g++ against include/ML/*.hpp + libmlhip.so and runs it: EM::CovarianceType::Tied of
the C++ facade. Host mode (the type is accepted) on CPU; on the GPU box a tied fit whose printed parameters must be those of
mlhip_em_iterate with MLHIP_COVARIANCE_TIED from the same start (the facade's loop is that call). With -DTIED_EIGEN (include/eigen_api
first, tests/cpp/eigen_shim) the same enum through the Eigen-typed API of include/ML/EigenApi.hpp."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "tied_fit_test.cpp")
EXE = {False: os.path.join(ROOT, "tests", "cpp", "tied_fit_test"), True: os.path.join(ROOT, "tests", "cpp", "tied_fit_eigen_test")}


def _build(eigen=False):
    exe = EXE[eigen]
    deps = [SRC, os.path.join(ROOT, "ml_amd", "libmlhip.so"), os.path.join(ROOT, "include", "ML", "EM.hpp"),
            os.path.join(ROOT, "include", "ML", "EigenApi.hpp")]
    if os.path.exists(exe) and os.path.getmtime(exe) > max(os.path.getmtime(d) for d in deps):
        return exe
    extra = ["-DTIED_EIGEN", "-I", os.path.join(ROOT, "tests", "cpp", "eigen_shim"), "-I", os.path.join(ROOT, "include", "eigen_api")] if eigen else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra"] + extra + ["-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                           "-L", os.path.join(ROOT, "ml_amd"), "-lmlhip", "-Wl,-rpath," + os.path.join(ROOT, "ml_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.parametrize("eigen", [False, True], ids=["facade", "eigen"])
def test_tied_covariance_type_host_paths(eigen):
    out = subprocess.run([_build(eigen), "host"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


@pytest.mark.gpu
def test_tied_fit_through_the_eigen_api_on_the_gpu():
    out = subprocess.run([_build(True), "gpu"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


@pytest.mark.gpu
def test_tied_fit_on_the_gpu_matches_the_c_abi():
    from ml_amd import _lib
    out = subprocess.run([_build(), "gpu"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    values = {}
    for line in out.stdout.splitlines():
        key, _, rest = line.partition(" ")
        values.setdefault(key, []).extend(rest.split())
    n, d, K, steps = (int(v) for v in values["shape"])
    X = np.array(values["x"], dtype=np.float64).reshape(n, d)
    start = np.array(values["start"], dtype=np.float64).reshape(K, d)
    ctx = _lib.Context()
    dt = _lib.Data(ctx, X)
    # the facade's default start: the given means, equal mixing, the pooled copies of the sample covariance
    cov = dt.sample_covariance()[1]
    pooled = np.zeros((d, d))
    for _ in range(K):
        pooled += (1.0 / K) * cov
    done, _, ll, pi, mu, S, _ = dt.em_iterate(np.full(K, 1.0 / K), start, pooled, steps, tied=True)
    dt.close()
    ctx.close()
    assert done == steps
    assert float(values["ll"][0]) == ll
    assert np.array_equal(np.array(values["pi"], dtype=np.float64), pi)
    assert np.array_equal(np.array(values["mu"], dtype=np.float64).reshape(K, d), mu)
    assert np.array_equal(np.array(values["cov"], dtype=np.float64).reshape(d, d), S)
