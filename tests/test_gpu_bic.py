"""EM.bic and EM.aic on the device: after a small fit in each covariance mode they are scikit-learn's formulas on score(X) bit for
bit (-2 N score(X) + p log N and + 2 p), on held-out data too, and on the fit's own data they agree with the fit's log_likelihood to
1e-12 relative. The fits run to a relative tolerance of 1e-13 on well separated blobs (fast linear convergence), so the last iteration moved the
log-likelihood by less than that and the likelihood of the final parameters (what score(X) evaluates) is the one the fit reports."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def blobs(n, d, K, seed):
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(K, d)) * 8
    labels = np.arange(n) % K
    return np.ascontiguousarray(centres[labels] + rng.normal(size=(n, d)))


@pytest.mark.parametrize("mode", ["full", "diag", "tied"])
def test_bic_and_aic_are_the_formulas_on_score(mode):
    from ml_amd.cppyml import clustering
    d, K, n = 4, 3, 900
    X = blobs(n, d, K, seed=11)
    em = clustering.EM(K)
    em.set_seed(2)
    em.set_covariance_type(mode)
    em.set_absolute_tolerance(0.0)
    em.set_relative_tolerance(1e-13)
    em.set_maximum_steps(500)
    assert em.fit(X) and em.converged
    p = em.number_parameters
    assert p == {"full": K * d * (d + 1) // 2, "diag": K * d, "tied": d * (d + 1) // 2}[mode] + K * d + K - 1
    for Y in (X, blobs(333, d, K, seed=12)):
        m = len(Y)
        score = em.score(Y)
        assert em.bic(Y) == -2.0 * m * score + p * math.log(m)
        assert em.aic(Y) == -2.0 * m * score + 2.0 * p
    ll = em.log_likelihood
    bic_ll, aic_ll = -2.0 * n * ll + p * math.log(n), -2.0 * n * ll + 2.0 * p
    print(f"{mode}: bic {em.bic(X):.6f} (from log_likelihood {bic_ll:.6f}), aic {em.aic(X):.6f}")
    assert abs(em.bic(X) - bic_ll) <= 1e-12 * abs(bic_ll)
    assert abs(em.aic(X) - aic_ll) <= 1e-12 * abs(aic_ll)


def test_bic_prefers_the_true_number_of_components():
    from ml_amd.cppyml import clustering
    X = blobs(1200, 3, 3, seed=21)
    scores = {}
    for K in (1, 2, 3, 4, 5):
        em = clustering.EM(K)
        em.set_seed(5)
        em.fit(X)
        scores[K] = em.bic(X)
    assert min(scores, key=scores.get) == 3, scores
