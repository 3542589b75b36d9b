"""EM.number_parameters without a GPU: the exact N == K fit needs no device, so the count can be read in every covariance mode.
BIC and AIC themselves run the scoring pass: tests/test_gpu_bic.py. CPU only."""
import numpy as np
import pytest


def expected(mode, d, K):
    covariance = {"full": K * d * (d + 1) // 2, "diag": K * d, "tied": d * (d + 1) // 2}[mode]
    return covariance + K * d + K - 1


@pytest.mark.parametrize("mode", ["full", "diag", "tied"])
@pytest.mark.parametrize("d,K", [(1, 1), (1, 4), (2, 3), (5, 2), (17, 6), (32, 3)])
def test_number_parameters(mode, d, K):
    from ml_amd.cppyml import clustering
    em = clustering.EM(K)
    em.set_covariance_type(mode)
    assert em.fit(np.random.default_rng(d * 100 + K).normal(size=(K, d)))     # N == K: the exact fit, host only
    assert em.number_parameters == expected(mode, d, K)
    other = "diag" if mode != "diag" else "full"
    em.set_covariance_type(other)                                              # the count is of the mode the model was FITTED in
    assert em.number_parameters == expected(mode, d, K)


def test_unfitted_model_raises():
    from ml_amd.cppyml import clustering
    em = clustering.EM(3)
    with pytest.raises(ValueError):
        em.number_parameters
    X = np.zeros((5, 2))
    for method in (em.bic, em.aic):
        with pytest.raises(ValueError):
            method(X)
        with pytest.raises(TypeError):
            method(X.astype(np.float32))
