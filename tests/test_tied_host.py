"""Tied-covariance EM without a GPU: the M-step's closing arithmetic (mlhip_em_finalize_statistics_tied, the host helper both routes
of mlhip_em_step_tied end in) against the scikit-learn covariance_type='tied' fixtures, the Python surface's argument checks, and
the new symbols. Tolerances as in tests/test_gpu_diag.py: mixing / means 1e-11, covariance 1e-10 (max-norm relative). CPU only."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden

TIED_CASES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "em_tied_onestep_*.npz")))


def relerr(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, np.max(np.abs(b)))


def packed_scatter(Xt):
    """sum_i [x~_i; 1][x~_i; 1]^T as the packed lower triangle, entry (a, b), a >= b, at a (a + 1) / 2 + b."""
    n, d = Xt.shape
    Z = np.hstack([Xt, np.ones((n, 1))])
    M = Z.T @ Z
    return np.array([M[a, b] for a in range(d + 1) for b in range(a + 1)])


def test_the_five_fixtures_exist():
    assert TIED_CASES == ["em_tied_onestep_%s.npz" % t for t in ("d13_K5", "d16_K16", "d32_K8", "d4_K3", "d7_K40")]


@pytest.mark.parametrize("case", TIED_CASES)
def test_finalize_statistics_tied_matches_sklearn_fixture(case):
    from ml_amd import _lib
    g = load_golden(case)
    X, R0 = g["X"], g["R0"]
    n, d = X.shape
    shift = X.mean(axis=0)
    Xt = X - shift
    stats = np.hstack([R0.T @ Xt, R0.sum(axis=0)[:, None]])          # K x (d + 1): [S1_k | S0_k]
    pi1, mu1, S1 = _lib.finalize_statistics_tied(stats, packed_scatter(Xt), shift, float(n))
    assert relerr(pi1, g["pi1"]) < 1e-11
    assert relerr(mu1, g["mu1"]) < 1e-11
    assert relerr(S1, g["Sigma1"]) < 1e-10
    assert np.array_equal(S1, S1.T)
    assert abs(pi1.sum() - 1) < 1e-12


def test_finalize_statistics_tied_is_the_pooled_full_closing():
    """Sigma = sum_k pi_k Sigma_k over mlhip_em_finalize_statistics' covariances (the composed route), ridge 1e-15 once."""
    from ml_amd import _lib
    rng = np.random.default_rng(5)
    n, d, K = 300, 5, 3
    X = rng.standard_normal((n, d)) @ rng.standard_normal((d, d)) + 3.0
    R = rng.dirichlet(np.ones(K), n)
    shift = X.mean(axis=0)
    Xt = X - shift
    full = np.empty((K, (d + 1) * (d + 2) // 2))                      # packed sum_i r_ik [x~_i; 1][x~_i; 1]^T per component
    Z = np.hstack([Xt, np.ones((n, 1))])
    for k in range(K):
        M = (Z * R[:, k][:, None]).T @ Z
        full[k] = [M[a, b] for a in range(d + 1) for b in range(a + 1)]
    pi_f, mu_f, S_f = np.empty(K), np.empty((K, d)), np.empty((K, d, d))
    _lib.check(_lib.lib.mlhip_em_finalize_statistics(d, K, _lib.dptr(np.ascontiguousarray(full)), _lib.dptr(shift), C.c_double(n),
                                                     _lib.dptr(pi_f), _lib.dptr(mu_f), _lib.dptr(S_f)))
    stats = np.hstack([R.T @ Xt, R.sum(axis=0)[:, None]])
    pi_t, mu_t, S_t = _lib.finalize_statistics_tied(stats, packed_scatter(Xt), shift, float(n))
    assert relerr(pi_t, pi_f) < 1e-13 and relerr(mu_t, mu_f) < 1e-13
    assert relerr(S_t, np.einsum("k,kab->ab", pi_f, S_f)) < 1e-12


def test_finalize_statistics_tied_checks_its_arguments():
    from ml_amd import _lib
    assert _lib.lib.mlhip_em_finalize_statistics_tied(2, 1, None, None, None, C.c_double(1.0), None, None, None) == _lib.E_INVALID_ARGUMENT


def test_covariance_type_strings():
    from ml_amd.cppyml import clustering
    em = clustering.EM(3)
    em.set_covariance_type("tied")
    em.set_covariance_type("diag")
    em.set_covariance_type("full")
    with pytest.raises(ValueError):
        em.set_covariance_type("spherical")


def test_a_tied_fit_needs_a_device():
    from ml_amd import _lib
    from ml_amd.cppyml import clustering
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    em = clustering.EM(2)
    em.set_covariance_type("tied")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        em.fit(np.random.default_rng(0).standard_normal((50, 3)))


def test_new_symbols_are_exported():
    from ml_amd import _lib
    for name in ("mlhip_em_step_tied", "mlhip_em_finalize_statistics_tied", "mlhip_em_tied_route"):
        assert hasattr(_lib.lib, name), name
    route = C.c_int()
    assert _lib.lib.mlhip_em_tied_route(None, 2, C.byref(route)) == _lib.E_INVALID_ARGUMENT
    assert _lib.lib.mlhip_em_step_tied(None, None, 2, None, None, None, None, None, None, None) == _lib.E_INVALID_ARGUMENT
