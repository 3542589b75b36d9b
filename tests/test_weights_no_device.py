"""Row weights without a GPU: the new symbols are exported, the entry points check their arguments and then fail like every
other device call (no CPU fallback), and the Python layers refuse a wrong type, dtype or length before any device call. CPU only."""
import ctypes as C

import numpy as np
import pytest


def test_new_symbols_are_exported():
    from ml_amd import _lib
    for name in ("mlhip_data_set_weights", "mlhip_data_weight_sum", "mlpp_em_fit_weighted"):
        assert hasattr(_lib.lib, name), name


def test_entry_points_check_their_arguments_without_a_device():
    from ml_amd import _lib
    total = C.c_double()
    assert _lib.lib.mlhip_data_set_weights(None, None, None) == _lib.E_INVALID_ARGUMENT
    assert _lib.lib.mlhip_data_weight_sum(None, C.byref(total)) == _lib.E_INVALID_ARGUMENT
    conv = C.c_int()
    assert _lib.lib.mlpp_em_fit_weighted(None, None, None, C.c_uint64(0), 2, C.byref(conv)) == _lib.E_INVALID_ARGUMENT


def test_weight_arguments_are_checked_before_any_device_call():
    from ml_amd import _lib
    from ml_amd.cppyml import clustering
    X = np.random.default_rng(0).standard_normal((50, 3))
    em = clustering.EM(2)
    for bad in ([1.0] * 50, np.ones(50, dtype=np.float32), np.ones(50, dtype=np.int64)):
        with pytest.raises(TypeError):
            em.fit(X, sample_weight=bad)
        with pytest.raises(TypeError):
            _lib.require_weights(bad, 50)
    for bad in (np.ones(49), np.ones((50, 1)), np.ones(100)[::2]):
        with pytest.raises(ValueError):
            em.fit(X, sample_weight=bad)
        with pytest.raises(ValueError):
            _lib.require_weights(bad, 50)
    w = np.ones(50)
    assert _lib.require_weights(w, 50) is w


def test_a_weighted_fit_needs_a_device():
    from ml_amd import _lib
    from ml_amd.cppyml import clustering
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    X = np.random.default_rng(0).standard_normal((50, 3))
    with pytest.raises(RuntimeError):
        clustering.EM(2).fit(X, sample_weight=np.ones(50))
    with pytest.raises(RuntimeError):
        _lib.Context(0)
