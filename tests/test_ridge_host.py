"""The covariance ridge without a GPU: the host closings with the ridge given (mlhip_em_finalize_statistics_ridge / _tied_ridge) --
exact identities between two ridges, the default as the case of the old entry points, the scikit-learn reg_covar = 1e-3 fixtures
(tests/golden/make_ridge_golden.py) --, the argument checks of the helpers and of EM.set_covariance_regularisation, and the new
symbols. Tolerances as in tests/test_tied_host.py for the same quantities: mixing / means 1e-11, covariances 1e-10 (max-norm
relative). CPU only."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden

R = 1e-3
BAD = (float("nan"), float("inf"), -float("inf"), -1e-3)


def relerr(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, np.max(np.abs(b)))


def packed(M):
    """The lower triangle of a symmetric (d + 1) x (d + 1) matrix, entry (a, b), a >= b, at a (a + 1) / 2 + b."""
    return np.array([M[a, b] for a in range(M.shape[0]) for b in range(a + 1)])


def full_statistics(Xt, Rk):
    """K packed records sum_i r_ik [x~_i; 1][x~_i; 1]^T."""
    Z = np.hstack([Xt, np.ones((Xt.shape[0], 1))])
    return np.array([packed((Z * Rk[:, k][:, None]).T @ Z) for k in range(Rk.shape[1])])


def tied_statistics(Xt, Rk):
    """K x (d + 1) rows [S1_k | S0_k] and the packed total scatter."""
    Z = np.hstack([Xt, np.ones((Xt.shape[0], 1))])
    return np.hstack([Rk.T @ Xt, Rk.sum(axis=0)[:, None]]), packed(Z.T @ Z)


def random_statistics():
    rng = np.random.default_rng(7)
    n, d, K = 300, 5, 4
    X = rng.standard_normal((n, d)) @ rng.standard_normal((d, d)) + 3.0
    Rk = rng.dirichlet(np.ones(K), n)
    shift = X.mean(axis=0)
    return n, d, K, X - shift, Rk, shift


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def test_full_closing_adds_the_ridge_to_the_diagonal_and_nothing_else():
    from ml_amd import _lib
    n, d, K, Xt, Rk, shift = random_statistics()
    st = full_statistics(Xt, Rk)
    pi0, mu0, S0 = _lib.finalize_statistics_ridge(st, shift, float(n), 0.0)
    pi1, mu1, S1 = _lib.finalize_statistics_ridge(st, shift, float(n), R)
    assert same_bits(pi0, pi1) and same_bits(mu0, mu1)
    off = ~np.eye(d, dtype=bool)
    assert same_bits(S0[:, off], S1[:, off])
    diag0, diag1 = np.einsum("kaa->ka", S0), np.einsum("kaa->ka", S1)
    assert same_bits(diag1, diag0 + np.float64(R))
    assert (diag1 != diag0).all()
    # the old entry point is the default ridge's case
    pid, mud, Sd = _lib.finalize_statistics_ridge(st, shift, float(n), _lib.DEFAULT_COVARIANCE_RIDGE)
    pio, muo, So = np.empty(K), np.empty((K, d)), np.empty((K, d, d))
    _lib.check(_lib.lib.mlhip_em_finalize_statistics(d, K, _lib.dptr(st), _lib.dptr(shift), C.c_double(n), _lib.dptr(pio), _lib.dptr(muo),
                                                     _lib.dptr(So)))
    assert same_bits(pid, pio) and same_bits(mud, muo) and same_bits(Sd, So)
    assert same_bits(np.einsum("kaa->ka", So), diag0 + np.float64(1e-15))
    # -0.0 counts as 0
    _, _, Sm = _lib.finalize_statistics_ridge(st, shift, float(n), -0.0)
    assert same_bits(Sm, S0)


def test_tied_closing_adds_the_ridge_once():
    from ml_amd import _lib
    n, d, K, Xt, Rk, shift = random_statistics()
    st, T = tied_statistics(Xt, Rk)
    pi0, mu0, S0 = _lib.finalize_statistics_tied(st, T, shift, float(n), ridge=0.0)
    pi1, mu1, S1 = _lib.finalize_statistics_tied(st, T, shift, float(n), ridge=R)
    assert same_bits(pi0, pi1) and same_bits(mu0, mu1)
    off = ~np.eye(d, dtype=bool)
    assert same_bits(S0[off], S1[off])
    assert same_bits(np.diag(S1), np.diag(S0) + np.float64(R))
    pid, mud, Sd = _lib.finalize_statistics_tied(st, T, shift, float(n), ridge=_lib.DEFAULT_COVARIANCE_RIDGE)
    pio, muo, So = _lib.finalize_statistics_tied(st, T, shift, float(n))
    assert same_bits(pid, pio) and same_bits(mud, muo) and same_bits(Sd, So)
    assert same_bits(np.diag(So), np.diag(S0) + np.float64(1e-15))


def test_full_fixture_matches_sklearn_reg_covar():
    from ml_amd import _lib
    g = load_golden("em_ridge_onestep_full_d4_K3.npz")
    X, R0, ridge = g["X"], g["R0"], float(g["ridge"])
    assert ridge == R and X.shape[0] <= 800
    shift = X.mean(axis=0)
    pi1, mu1, S1 = _lib.finalize_statistics_ridge(full_statistics(X - shift, R0), shift, float(X.shape[0]), ridge)
    assert relerr(pi1, g["pi1"]) < 1e-11
    assert relerr(mu1, g["mu1"]) < 1e-11
    assert relerr(S1, g["Sigma1"]) < 1e-10
    # the ridge is what the fixture pins: the default's covariances miss it by r on the diagonal
    _, _, Sd = _lib.finalize_statistics_ridge(full_statistics(X - shift, R0), shift, float(X.shape[0]), 1e-15)
    assert relerr(Sd, g["Sigma1"]) > 1e-5


def test_diag_fixture_matches_sklearn_reg_covar():
    """No host diagonal closing is exported: the fixture goes through the `_ridge` FULL closing of the full statistics, whose
    covariances' diagonals are the diagonal mode's variances entry by entry (the device path: tests/test_gpu_ridge.py)."""
    from ml_amd import _lib
    g = load_golden("em_ridge_onestep_diag_d7_K5.npz")
    X, R0, ridge = g["X"], g["R0"], float(g["ridge"])
    assert ridge == R and X.shape[0] <= 800
    shift = X.mean(axis=0)
    pi1, mu1, S1 = _lib.finalize_statistics_ridge(full_statistics(X - shift, R0), shift, float(X.shape[0]), ridge)
    assert relerr(pi1, g["pi1"]) < 1e-11
    assert relerr(mu1, g["mu1"]) < 1e-11
    assert relerr(np.einsum("kaa->ka", S1), g["var1"]) < 1e-10


def test_tied_fixture_matches_sklearn_reg_covar():
    from ml_amd import _lib
    g = load_golden("em_ridge_onestep_tied_d13_K5.npz")
    X, R0, ridge = g["X"], g["R0"], float(g["ridge"])
    assert ridge == R and X.shape[0] <= 800
    shift = X.mean(axis=0)
    st, T = tied_statistics(X - shift, R0)
    pi1, mu1, S1 = _lib.finalize_statistics_tied(st, T, shift, float(X.shape[0]), ridge=ridge)
    assert relerr(pi1, g["pi1"]) < 1e-11
    assert relerr(mu1, g["mu1"]) < 1e-11
    assert relerr(S1, g["Sigma1"]) < 1e-10
    assert np.array_equal(S1, S1.T)


@pytest.mark.parametrize("bad", BAD)
def test_helpers_refuse_a_bad_ridge(bad):
    from ml_amd import _lib
    n, d, K, Xt, Rk, shift = random_statistics()
    st = full_statistics(Xt, Rk)
    pi, mu, S = np.full(K, 7.0), np.full((K, d), 7.0), np.full((K, d, d), 7.0)
    rc = _lib.lib.mlhip_em_finalize_statistics_ridge(d, K, _lib.dptr(st), _lib.dptr(shift), float(n), bad, _lib.dptr(pi), _lib.dptr(mu), _lib.dptr(S))
    assert rc == _lib.E_INVALID_ARGUMENT
    assert (pi == 7.0).all() and (S == 7.0).all()
    ts, T = tied_statistics(Xt, Rk)
    St = np.full((d, d), 7.0)
    rc = _lib.lib.mlhip_em_finalize_statistics_tied_ridge(d, K, _lib.dptr(ts), _lib.dptr(T), _lib.dptr(shift), float(n), bad, _lib.dptr(pi),
                                                          _lib.dptr(mu), _lib.dptr(St))
    assert rc == _lib.E_INVALID_ARGUMENT
    assert (St == 7.0).all()
    with pytest.raises(ValueError):
        _lib.finalize_statistics_ridge(st, shift, float(n), bad)


def test_em_covariance_regularisation_surface():
    from ml_amd.cppyml import clustering
    em = clustering.EM(3)
    assert em.covariance_regularisation == 1e-15
    for value in (0.0, R):
        em.set_covariance_regularisation(value)
        assert em.covariance_regularisation == value
    for bad in BAD:
        with pytest.raises(ValueError):
            em.set_covariance_regularisation(bad)
        assert em.covariance_regularisation == R
    assert "set_covariance_regularisation" in clustering.__doc__ and "EM.covariance_regularisation" in clustering.__doc__


def test_new_symbols_are_exported():
    from ml_amd import _lib
    for name in ("mlhip_data_set_covariance_ridge", "mlhip_data_covariance_ridge", "mlhip_em_finalize_statistics_ridge",
                 "mlhip_em_finalize_statistics_tied_ridge", "mlpp_em_set_covariance_regularisation", "mlpp_em_covariance_regularisation"):
        assert hasattr(_lib.lib, name), name
    ridge = C.c_double()
    assert _lib.lib.mlhip_data_covariance_ridge(None, C.byref(ridge)) == _lib.E_INVALID_ARGUMENT
    assert _lib.lib.mlhip_data_set_covariance_ridge(None, None, 1e-3) == _lib.E_INVALID_ARGUMENT
    assert hasattr(_lib.Data, "set_covariance_ridge") and isinstance(_lib.Data.covariance_ridge, property)
