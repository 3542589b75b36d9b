"""EM restarts without a GPU: the setter and getters of EM.set_number_initialisations, the selection rule as the plain host function
mlhip_em_select_restart on hand-made vectors, the new symbols, the argument checks of the entry points, and a fit with restarts on a
machine without a device (no CPU fallback). CPU only."""
import ctypes as C

import numpy as np
import pytest

NAN, INF = float("nan"), float("inf")


def test_number_initialisations_surface():
    from ml_amd.cppyml import clustering
    em = clustering.EM(3)
    assert em.number_initialisations == 1                            # the default: the reference's behaviour
    for value in (4, 1, 17):
        em.set_number_initialisations(value)
        assert em.number_initialisations == value
    with pytest.raises(ValueError, match="At least 1 initialisation required"):
        em.set_number_initialisations(0)
    assert em.number_initialisations == 17                           # a refused value changes nothing
    assert em.best_initialisation == 0
    for values in (em.initialisation_log_likelihoods, em.initialisation_steps, em.initialisation_converged):
        assert len(values) == 0                                      # nothing fitted yet
    for name in ("EM.set_number_initialisations", "EM.number_initialisations", "EM.best_initialisation", "EM.initialisation_log_likelihoods",
                 "EM.initialisation_steps", "EM.initialisation_converged"):
        assert name in clustering.__doc__, name


def test_the_exact_fit_ignores_the_setting():
    """N == K needs no device and no restarts: one entry per vector, like a fit with one initialisation."""
    from ml_amd.cppyml import clustering
    X = np.array([[0.0, 1.0], [2.0, 3.0], [5.0, 8.0]])
    em = clustering.EM(3)
    em.set_number_initialisations(4)
    assert em.fit(X)
    assert em.best_initialisation == 0
    assert list(em.initialisation_log_likelihoods) == [INF] and list(em.initialisation_steps) == [0]
    assert list(em.initialisation_converged) == [True]
    assert np.array_equal(em.means, X.T)


# (log-likelihoods, converged flags, the restart the rule keeps)
SELECTIONS = [
    ([-3.0, -1.0, -2.0], [1, 0, 1], 2),            # a converged restart beats a better one that did not converge
    ([-2.0, -1.0, -1.0, -1.5], [1, 1, 1, 1], 1),   # ties go to the first
    ([-1.0, -1.0], [0, 0], 0),
    ([NAN, -5.0, -4.0], [1, 1, 1], 2),             # NaN never wins ...
    ([-5.0, NAN], [1, 1], 0),
    ([NAN, -7.0], [1, 0], 1),                      # ... not even as the only converged one
    ([-3.0, -2.0, -4.0], [0, 0, 0], 1),            # none converged: the same rule over all
    ([NAN, NAN, NAN], [1, 0, 1], 0),               # all NaN: restart 0
    ([NAN, NAN], [0, 0], 0),
    ([-1.25], [0], 0), ([-1.25], [1], 0), ([NAN], [1], 0),       # R = 1
    ([-INF, -1e308], [1, 1], 1), ([INF, 1.0], [0, 1], 1), ([INF, 1.0], [1, 1], 0),
    ([-2.0, -1.0], [7, -1], 1),                    # any nonzero flag counts as converged
]


@pytest.mark.parametrize("ll,converged,want", SELECTIONS)
def test_select_restart(ll, converged, want):
    from ml_amd import _lib
    assert _lib.em_select_restart(ll, converged) == want


def test_new_symbols_are_exported():
    from ml_amd import _lib
    for name in ("mlhip_em_iterate_restarts", "mlhip_em_select_restart", "mlhip_em_restarts_route", "mlpp_em_set_number_initialisations",
                 "mlpp_em_number_initialisations", "mlpp_em_best_initialisation", "mlpp_em_initialisation_log_likelihoods",
                 "mlpp_em_initialisation_steps", "mlpp_em_initialisation_converged"):
        assert hasattr(_lib.lib, name), name
    assert hasattr(_lib.Data, "em_iterate_restarts") and hasattr(_lib.Data, "em_restarts_route")


def test_entry_points_check_their_arguments_without_a_device():
    from ml_amd import _lib
    lib, bad = _lib.lib, _lib.E_INVALID_ARGUMENT
    ll, conv, best = (C.c_double * 2)(-1.0, -2.0), (C.c_int * 2)(1, 1), C.c_uint32(9)
    assert lib.mlhip_em_select_restart(2, None, conv, C.byref(best)) == bad
    assert lib.mlhip_em_select_restart(2, ll, None, C.byref(best)) == bad
    assert lib.mlhip_em_select_restart(2, ll, conv, None) == bad
    assert lib.mlhip_em_select_restart(0, ll, conv, C.byref(best)) == bad
    assert best.value == 9
    assert lib.mlhip_em_select_restart(2, ll, conv, C.byref(best)) == _lib.OK and best.value == 0
    route, per_launch = C.c_int(), C.c_uint32()
    assert lib.mlhip_em_restarts_route(None, 3, 0, 2, C.byref(route), C.byref(per_launch)) == bad
    steps = (C.c_uint32 * 2)()
    x = (C.c_double * 64)()
    assert lib.mlhip_em_iterate_restarts(None, None, 3, 0, 2, x, x, x, 5, 0.0, 0.0, steps, conv, ll, None, C.byref(best)) == bad
    count, value = C.c_uint32(), C.c_uint32()
    assert lib.mlpp_em_set_number_initialisations(None, 2) == bad
    assert lib.mlpp_em_number_initialisations(None, C.byref(value)) == bad
    assert lib.mlpp_em_best_initialisation(None, C.byref(value)) == bad
    for getter in (lib.mlpp_em_initialisation_log_likelihoods, lib.mlpp_em_initialisation_steps, lib.mlpp_em_initialisation_converged):
        assert getter(None, None, 0, C.byref(count)) == bad
    from ml_amd.cppyml import clustering
    em = clustering.EM(2)
    assert lib.mlpp_em_number_initialisations(em._h, None) == bad
    assert lib.mlpp_em_initialisation_steps(em._h, None, 0, None) == bad
    assert lib.mlpp_em_initialisation_steps(em._h, None, 3, C.byref(count)) == bad       # room announced, no array


def test_a_fit_with_restarts_needs_a_device():
    from ml_amd import _lib
    from ml_amd.cppyml import clustering
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    X = np.random.default_rng(0).standard_normal((50, 3))
    em = clustering.EM(2)
    em.set_number_initialisations(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        em.fit(X)
