"""The data conditions of tests/test_gpu_units.py, checked without a GPU, for every case and scaling of tests/units_cases.py:

(a) the fp64 restatements -- the whitening chain's q, the direct-form K-means distance in the reference's fma order, the two-pass
    covariance and M-step -- give the unit-scale BITS after unscaling: no input of the suite leaves the normal range, so a difference
    seen on the GPU is the kernel's;
(b) the extended-precision reference stays finite on the scaled inputs;
(c) the allowance U of units_cases covers the restatement's own deviation in a log-density with a factor of 4 to spare, and no row of
    any case is within 2 U of a tie (the GPU module's label checks leave out no row).

`python tests/test_units_cases.py` prints the measured factors (units_cases' docstring holds them)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import hp_cases                        # noqa: E402
from oracle import hp_reference as hp              # noqa: E402
import units_cases as uc                           # noqa: E402


def _finite(step):
    return all(np.isfinite(np.asarray(part, dtype=np.float64)).all() for part in step)


@functools.lru_cache(maxsize=None)
def _unit_em(shape):
    X, pi0, mu0, S0 = uc.em_problem(shape)
    q = uc.whitened_q(X, mu0, S0)
    lw = uc.log_constants(pi0, S0) - 0.5 * q
    return q, lw


def em_measure(shape, scaling):
    """(q bits equal, largest |lw' + sum ln f - lw|, U, rows within 2 U of a tie) of the whitening restatement."""
    d = shape[0]
    q1, lw1 = _unit_em(shape)
    X, pi0, mu0, S0 = uc.em_problem(shape, scaling)
    q = uc.whitened_q(X, mu0, S0)
    coef = uc.log_constants(pi0, S0)
    lw = coef - 0.5 * q
    ln_f = uc.sum_ln_f(scaling, d)
    U = uc.allowance(d, coef, ln_f, np.abs(lw).max())
    dev = float(np.abs((lw + ln_f) - lw1).max())
    return uc.same_bits(q, q1), dev, U, int(uc.undecided_rows(lw1, U).sum())


@pytest.mark.parametrize("scaling", uc.SCALINGS)
@pytest.mark.parametrize("shape", uc.EM_SHAPES, ids=[f"d{s[0]}-K{s[1]}" for s in uc.EM_SHAPES])
def test_whitening_restatement_is_covariant_and_inside_the_allowance(shape, scaling):
    same, dev, U, undecided = em_measure(shape, scaling)
    assert same                                    # (a)
    assert dev <= U / 4, (dev, U)                  # (c)
    assert undecided == 0


@pytest.mark.parametrize("scaling", uc.SCALINGS)
@pytest.mark.parametrize("shape", uc.EM_SHAPES, ids=[f"d{s[0]}-K{s[1]}" for s in uc.EM_SHAPES])
def test_reference_em_step_is_finite(shape, scaling):
    assert _finite(hp.em_step(*uc.em_problem(shape, scaling)))        # (b)


@pytest.mark.parametrize("scaling", uc.SCALINGS)
@pytest.mark.parametrize("shape", uc.DIAG_SHAPES, ids=[f"d{s[0]}-K{s[1]}" for s in uc.DIAG_SHAPES])
def test_diagonal_cases(shape, scaling):
    d = shape[0]
    X1, pi0, mu1, v1 = uc.em_problem(shape, None, diagonal=True)
    X, _, mu, v = uc.em_problem(shape, scaling, diagonal=True)
    q1 = np.stack([(((X1 - mu1[k]) ** 2) / v1[k]).sum(axis=1) for k in range(len(pi0))], axis=1)
    q = np.stack([(((X - mu[k]) ** 2) / v[k]).sum(axis=1) for k in range(len(pi0))], axis=1)
    assert uc.same_bits(q, q1)
    ref = hp.em_step_diag(X, pi0, mu, v)
    assert _finite(ref)
    coef1 = np.log(pi0) - 0.5 * np.log(v1).sum(axis=1)
    coef = np.log(pi0) - 0.5 * np.log(v).sum(axis=1)
    ln_f = uc.sum_ln_f(scaling, d)
    lw1, lw = coef1 - 0.5 * q1, coef - 0.5 * q
    U = uc.allowance(d, coef, ln_f, np.abs(lw).max())
    assert np.abs((lw + ln_f) - lw1).max() <= U / 4
    assert uc.undecided_rows(lw1, U).sum() == 0


@pytest.mark.parametrize("scaling", uc.SCALINGS)
def test_tied_case(scaling):
    d = uc.TIED_SHAPE[0]
    X1, pi0, mu1, S1 = uc.tied_problem()
    X, _, mu, S = uc.tied_problem(scaling)
    K = len(pi0)
    q1, q = uc.whitened_q(X1, mu1, np.stack([S1] * K)), uc.whitened_q(X, mu, np.stack([S] * K))
    assert uc.same_bits(q, q1)
    assert _finite(hp.em_step_tied(X, pi0, mu, S))
    coef1, coef = uc.log_constants(pi0, np.stack([S1] * K)), uc.log_constants(pi0, np.stack([S] * K))
    ln_f = uc.sum_ln_f(scaling, d)
    lw1, lw = coef1 - 0.5 * q1, coef - 0.5 * q
    U = uc.allowance(d, coef, ln_f, np.abs(lw).max())
    assert np.abs((lw + ln_f) - lw1).max() <= U / 4
    assert uc.undecided_rows(lw1, U).sum() == 0


KM_SHAPES = sorted({c[1] for c in uc.KM_CASES} | {uc.KM_RESIDENT_SHAPE, uc.KM_WEIGHTED_SHAPE})


@pytest.mark.parametrize("scaling", uc.UNIFORM)
@pytest.mark.parametrize("shape", KM_SHAPES, ids=[f"d{s[0]}-K{s[1]}" for s in KM_SHAPES])
def test_direct_form_distances_are_covariant(shape, scaling):
    d, K, n = shape
    X1, C1 = uc.km_problem(shape)
    X, C = uc.km_problem(shape, scaling)
    f2 = 4.0 ** int(uc.exponents(scaling, d)[0])
    if K > 200:                                   # (the chunked-table shape: a seeded tenth of the rows is the same statement)
        rows = np.random.default_rng(5).choice(n, n // 10, replace=False)
        X1, X = X1[rows], X[rows]
    D1, D = uc.direct_distances(X1, C1), uc.direct_distances(X, C)
    assert uc.same_bits(D / f2, D1)               # (a)
    assert np.array_equal(D.argmin(axis=1), D1.argmin(axis=1))
    assert _finite(hp.kmeans_step(X, C))          # (b)


@pytest.mark.parametrize("scaling", uc.UNIFORM)
def test_lattice_ties_survive_the_scaling(scaling):
    X1, C1 = uc.lattice_problem()
    X, C = uc.lattice_problem(scaling)
    f2 = 4.0 ** int(uc.exponents(scaling, X.shape[1])[0])
    D1, D = uc.direct_distances(X1[::5], C1), uc.direct_distances(X[::5], C)
    assert uc.same_bits(D / f2, D1)
    assert ((D1 == D1.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum() >= 40           # rows whose nearest centroids tie EXACTLY


@pytest.mark.parametrize("name,shape,env,route", uc.KM_MIXED_CASES, ids=[c[0] for c in uc.KM_MIXED_CASES])
def test_mixed_unit_kmeans_rows_are_decided(name, shape, env, route):
    """M60 is not covariant for K-means; the GPU case is held to the reference on the scaled input, which must separate 99.9 % of the
    rows by more than 64 * 2^-53 * distance (test_gpu_hp_error.py's margin)."""
    X, C = uc.km_problem(shape, "M60")
    dist, _, margin, *_ = hp.kmeans_step(X, C)
    assert np.isfinite(dist.astype(np.float64)).all()
    assert (margin > 64 * hp.EPS64 * dist).mean() >= 0.999


@pytest.mark.parametrize("scaling", uc.SCALINGS)
@pytest.mark.parametrize("d,n", uc.DATA_SHAPES)
def test_two_pass_covariance_is_covariant(d, n, scaling):
    X1 = hp_cases.problem(d, 1, n, 1.5)[0]
    f = uc.factors(scaling, d)
    m1, c1 = uc.two_pass_covariance(X1)
    m, c = uc.two_pass_covariance(uc.points(X1, f))
    assert uc.same_bits(m / f, m1) and uc.same_bits(c / f[:, None] / f[None, :], c1)
    assert _finite(hp.sample_covariance(uc.points(X1, f)))


@pytest.mark.parametrize("scaling", uc.SCALINGS)
@pytest.mark.parametrize("d,K,n,env", uc.MSTEP_CASES[:-1], ids=[f"d{c[0]}-K{c[1]}" for c in uc.MSTEP_CASES[:-1]])
def test_two_pass_mstep_is_covariant(d, K, n, env, scaling):
    X1 = hp_cases.problem(d, K, n, 1.0)[0]
    R = uc.responsibilities(n, K, 100 * d + K)
    f = uc.factors(scaling, d)
    pi1, mu1, S1 = uc.two_pass_mstep(X1, R)
    pi, mu, S = uc.two_pass_mstep(uc.points(X1, f), R)
    assert uc.same_bits(pi, pi1) and uc.same_bits(mu / f, mu1) and uc.same_bits(S / f[:, None] / f[None, :], S1)
    assert _finite(hp.m_step(uc.points(X1, f), R))


def test_screen_case_is_covariant_under_the_scalings_it_is_screened_at():
    import estep_screen_cases as sc
    d, K, n = uc.SCREEN_SHAPE
    X1, p = sc.mixture(d, K, n, 5)
    q1 = uc.whitened_q(X1[:257], p[1], p[2])
    for scaling in uc.SCALINGS:
        f = uc.factors(scaling, d)
        assert uc.same_bits(uc.whitened_q(uc.points(X1[:257], f), uc.points(p[1], f), uc.covariances(p[2], f)), q1)


def test_the_step_cases_are_the_edge_suites_routes():
    """units_cases restates test_gpu_hp_edges.STEP_ROUTES (one EM step per row of it, then two more shapes): the copy may not drift."""
    from test_gpu_hp_edges import STEP_ROUTES
    assert uc.EM_CASES[:len(STEP_ROUTES)] == STEP_ROUTES and len(uc.EM_CASES) == len(STEP_ROUTES) + 2


def test_the_scalings_are_what_the_module_says():
    for d in (2, 32, 136):
        assert set(uc.exponents("U-300", d)) == {-300} and set(uc.exponents("U+300", d)) == {300}
        s16, s60 = uc.exponents("M16", d), uc.exponents("M60", d)
        assert s16.min() >= 0 and s16.max() <= 16 and s60.min() >= -60 and s60.max() <= 60
        assert 2.0 ** (s16.max() - s16.min()) < 1e5
    assert uc.ridge("U-300") == 1e-15 * 2.0 ** -600 and uc.ridge("U+300") == 1e-15 * 2.0 ** 600 and uc.ridge("M60") == 0.0
    assert all(shape[2] % 64 for shape in uc.EM_SHAPES + uc.DIAG_SHAPES) and all(c[1][2] % 64 for c in uc.KM_CASES)


if __name__ == "__main__":
    worst = None
    for shape in uc.EM_SHAPES:
        for scaling in uc.SCALINGS:
            same, dev, U, undecided = em_measure(shape, scaling)
            factor = U / dev if dev > 0 else float("inf")
            print(f"UNITS-CPU d={shape[0]} K={shape[1]} N={shape[2]} {scaling} | q bits equal: {same} | deviation {dev:.2e} | U {U:.2e} | "
                  f"U / deviation {factor:.0f} | rows within 2 U of a tie {undecided}", flush=True)
            if worst is None or factor < worst[0]:
                worst = (factor, shape, scaling)
    print("smallest U / deviation:", worst)
