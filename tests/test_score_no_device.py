"""Without a GPU the batch queries fail loudly like `fit` does: there is no CPU fallback (skipped where a GPU is present, like
tests/test_abi_exports.py's check of `fit`); argument errors still come first. CPU only."""
import numpy as np
import pytest


def test_batch_queries_need_a_device():
    from ml_amd import _lib
    from ml_amd.cppyml import clustering
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    X = np.array([[0.0, 1.0, 2.0], [3.0, 5.0, 4.0]])
    em = clustering.EM(2)
    assert em.fit(X)                                       # N == K: the exact fit needs no device
    km = clustering.KMeans(2)
    km.fit(X)
    Y = np.zeros((10, 3))
    for method in (em.score_samples, em.score, em.predict, em.predict_proba, km.predict):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            method(Y)
        with pytest.raises(TypeError):
            method(Y.astype(np.float32))
    for method in (em.score_samples, em.predict, em.predict_proba, km.predict):
        with pytest.raises(ValueError):
            method(np.zeros((10, 4)))


def test_new_entry_points_check_their_arguments_without_a_device():
    from ml_amd import _lib
    k = _lib.C.c_int()
    assert _lib.lib.mlhip_em_score(None, None, 2, 0, None, None, None, None, None) == _lib.E_INVALID_ARGUMENT
    assert _lib.lib.mlhip_em_score_route(None, 2, _lib.C.byref(k)) == _lib.E_INVALID_ARGUMENT
