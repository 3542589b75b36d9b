"""Weighted K-means without a GPU: the new symbols are exported, the entry points check their arguments, KMeans.fit refuses bad
weights (type, dtype, length, values) before any device work, and a well-formed weighted fit then fails like every other device
call (no CPU fallback). CPU only."""
import ctypes as C

import numpy as np
import pytest

SYMBOLS = ("mlhip_kmeans_step_weighted", "mlhip_kmeans_iterate_weighted", "mlhip_kmeans_assign_weighted", "mlpp_kmeans_fit_weighted")


def test_new_symbols_are_exported():
    from ml_amd import _lib
    for name in SYMBOLS:
        assert hasattr(_lib.lib, name), name


def test_entry_points_refuse_null_arguments():
    from ml_amd import _lib
    inertia, changed, conv, steps = C.c_double(), C.c_uint64(), C.c_int(), C.c_uint32()
    assert _lib.lib.mlhip_kmeans_step_weighted(None, None, 2, None, C.byref(inertia), C.byref(changed), None, None) == _lib.E_INVALID_ARGUMENT
    assert _lib.lib.mlhip_kmeans_iterate_weighted(None, None, 2, None, None, C.c_uint32(5), C.c_double(0.0), C.byref(steps), C.byref(conv),
                                                  C.byref(inertia), None) == _lib.E_INVALID_ARGUMENT
    assert _lib.lib.mlhip_kmeans_assign_weighted(None, None, 2, None, C.byref(inertia), C.byref(changed)) == _lib.E_INVALID_ARGUMENT
    assert _lib.lib.mlpp_kmeans_fit_weighted(None, None, None, C.c_uint64(0), 2, C.byref(conv)) == _lib.E_INVALID_ARGUMENT


def test_fit_refuses_a_wrong_type_or_dtype():
    from ml_amd.cppyml import clustering
    X = np.random.default_rng(0).standard_normal((50, 3))
    km = clustering.KMeans(2)
    for bad in ([1.0] * 50, np.ones(50, dtype=np.float32), np.ones(50, dtype=np.int64)):
        with pytest.raises(TypeError):
            km.fit(X, sample_weight=bad)


def test_fit_refuses_bad_values_before_any_device_work():
    """ValueError, not the RuntimeError of a missing device: the checks run first, with or without a GPU."""
    from ml_amd.cppyml import clustering
    X = np.random.default_rng(0).standard_normal((50, 3))
    km = clustering.KMeans(2)
    negative, nan, inf = np.ones(50), np.ones(50), np.ones(50)
    negative[7], nan[11], inf[13] = -1.0, np.nan, np.inf
    for bad in (np.ones(49), np.ones((50, 1)), np.ones(100)[::2], negative, nan, inf, np.zeros(50)):
        with pytest.raises(ValueError):
            km.fit(X, sample_weight=bad)


def test_a_weighted_fit_needs_a_device():
    from ml_amd import _lib
    from ml_amd.cppyml import clustering
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    X = np.random.default_rng(0).standard_normal((50, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        clustering.KMeans(2).fit(X, sample_weight=np.ones(50))
