"""Builds tests/cpp/em_restarts_test.cpp with plain g++ against include/ML/*.hpp + libmlhip.so and runs it:
EM::set_number_initialisations of the C++ facade. Host mode (setter, exception, getters) on CPU, for the facade and -- with
-DRESTARTS_EIGEN (include/eigen_api first, tests/cpp/eigen_shim) -- the Eigen-typed API of include/ML/EigenApi.hpp; on the GPU box a
fit with 3 initialisations whose printed parameters must be those of the winner of Data.em_iterate_restarts from the same starts
(the facade's loop is that call)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "em_restarts_test.cpp")
EXE = {False: os.path.join(ROOT, "tests", "cpp", "em_restarts_test"), True: os.path.join(ROOT, "tests", "cpp", "em_restarts_eigen_test")}


def _build(eigen=False):
    exe = EXE[eigen]
    deps = [SRC, os.path.join(ROOT, "ml_amd", "libmlhip.so"), os.path.join(ROOT, "include", "ML", "EM.hpp"),
            os.path.join(ROOT, "include", "ML", "EigenApi.hpp")]
    if os.path.exists(exe) and os.path.getmtime(exe) > max(os.path.getmtime(d) for d in deps):
        return exe
    extra = ["-DRESTARTS_EIGEN", "-I", os.path.join(ROOT, "tests", "cpp", "eigen_shim"), "-I", os.path.join(ROOT, "include", "eigen_api")] if eigen else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra"] + extra + ["-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                           "-L", os.path.join(ROOT, "ml_amd"), "-lmlhip", "-Wl,-rpath," + os.path.join(ROOT, "ml_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.parametrize("eigen", [False, True], ids=["facade", "eigen"])
def test_number_initialisations_host_paths(eigen):
    out = subprocess.run([_build(eigen), "host"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


@pytest.mark.gpu
def test_fit_with_restarts_through_the_eigen_api_on_the_gpu():
    out = subprocess.run([_build(True), "gpu"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


@pytest.mark.gpu
def test_fit_with_restarts_on_the_gpu_matches_the_c_abi():
    from ml_amd import _lib
    out = subprocess.run([_build(), "gpu"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    values = {}
    for line in out.stdout.splitlines():
        key, _, rest = line.partition(" ")
        values.setdefault(key, []).extend(rest.split())
    n, d, K, steps, R = (int(v) for v in values["shape"])
    X = np.array(values["x"], dtype=np.float64).reshape(n, d)
    ctx = _lib.Context()
    dt = _lib.Data(ctx, X)
    # the starts of the test's initialiser (start r: the points r, r + 401, r + 802), equal mixing, copies of the sample covariance
    cov = dt.sample_covariance()[1]
    mu0 = np.stack([X[[r + 401 * k for k in range(K)]] for r in range(R)])
    restarts, best = dt.em_iterate_restarts(np.full((R, K), 1.0 / K), mu0, np.stack([np.stack([cov] * K)] * R), steps)
    dt.close()
    ctx.close()
    assert int(values["best"][0]) == best
    assert np.array_equal(np.array(values["lls"], dtype=np.float64), [r[2] for r in restarts])
    done, _, ll, pi, mu, S, _ = restarts[best]
    assert done == steps
    assert float(values["ll"][0]) == ll
    assert np.array_equal(np.array(values["pi"], dtype=np.float64), pi)
    assert np.array_equal(np.array(values["mu"], dtype=np.float64).reshape(K, d), mu)
    # (printed row by row from column-major d x d matrices: entry (a, b) of a symmetric matrix either way)
    assert np.array_equal(np.array(values["cov"], dtype=np.float64).reshape(K, d, d), S)
