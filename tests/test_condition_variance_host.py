"""Conditional variance, everything that needs no GPU: the argument errors of EM.conditional_variance and of the C entry points, the
exports, and the restatement (tests/condition_variance_reference.py) against what does not go through it -- a brute-force second
moment, K = 1, its own float64 error and positive definiteness on the shapes tests/test_gpu_condition_variance.py uses. CPU only."""
import numpy as np
import pytest

import condition_variance_reference as ref


def first(n):
    return tuple(range(n))


# the accuracy shapes of tests/test_gpu_condition_variance.py below the second-tile case (restated: that file needs the library)
N = 321
SHAPES = ([(1, 3, 2, (2, 0), n) for n in (1, 63, 64, 65, 257)] +
          [(2, 8, K, (6, 1, 3, 4), N) for K in (1, 16, 17, 64, 65)] +
          [(3, dO + 3, 3, first(dO), N) for dO in (1, 5, 12, 31, 32, 33)] +
          [(4, 4 + dM, 3, (3, 0, 2, 1), N) for dM in (1, 7, 8, 16, 17, 32, 33)] +
          [(5, 64, 40, first(32), N)] +
          [(6, 130, 3, tuple(int(c) for c in np.random.default_rng(130).permutation(130)[:70]), N)])


def shape_id(s):
    return "d%d-K%d-dO%d-n%d" % (s[1], s[2], len(s[3]), s[4])


def test_an_unfitted_model_raises_value_error():
    from ml_amd.cppyml import clustering
    with pytest.raises(ValueError, match="has not been fitted"):
        clustering.EM(3).conditional_variance(np.zeros((4, 1)), [0])


def _exactly_fitted():
    from ml_amd.cppyml import clustering
    em = clustering.EM(2)
    assert em.fit(np.array([[0.0, 1.0, 2.0], [3.0, 5.0, 4.0]]))  # N == K: the exact fit needs no device
    return em


def test_conditional_variance_raises_as_conditional_mean_does_before_device_work():
    em = _exactly_fitted()
    Y = np.zeros((10, 2))
    for bad in (Y.astype(np.float32), np.asfortranarray(Y), Y[:, 0], Y.tolist()):
        with pytest.raises(TypeError):
            em.conditional_variance(bad, [0, 1])
        with pytest.raises(TypeError):
            em.conditional_mean(bad, [0, 1])
    for bad in ([0.5, 1], 3, None):
        with pytest.raises(TypeError):
            em.conditional_variance(Y, bad)
        with pytest.raises(TypeError):
            em.conditional_mean(Y, bad)
    for bad in ([], [0, 1, 2], [0, 3], [-1, 0], [1, 1]):
        X = Y if len(bad) == 2 else np.zeros((10, max(len(bad), 1)))
        for kwargs in ({}, {"covariance": True}, {"return_mean": True}):
            with pytest.raises(ValueError):
                em.conditional_variance(X, bad, **kwargs)
        with pytest.raises(ValueError):
            em.conditional_mean(X, bad)
    with pytest.raises(ValueError, match="one column per observed coordinate"):
        em.conditional_variance(np.zeros((10, 1)), [0, 1])        # one column, two coordinates


def test_a_fitted_model_needs_a_device():
    from ml_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present: tests/test_gpu_condition_variance.py has the other side")
    em = _exactly_fitted()
    for kwargs in ({}, {"covariance": True}, {"return_mean": True}):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            em.conditional_variance(np.zeros((10, 2)), [2, 0], **kwargs)


def test_new_symbols_are_exported():
    from ml_amd import _lib
    from ml_amd.cppyml import clustering
    for name in ("mlhip_em_conditional_variances", "mlhip_em_condition_variance_route", "mlpp_em_conditional_variances"):
        assert hasattr(_lib.lib, name), name
    assert callable(_lib.em_conditional_variances) and callable(_lib.em_condition_variance_route)
    assert not hasattr(_lib.Data, "em_conditional_variances") and not hasattr(_lib.Data, "em_condition_variance_route")
    assert callable(clustering.EM.conditional_variance)
    assert "`EM.conditional_variance`" in clustering.__doc__


def test_entry_points_check_their_arguments_without_a_device():
    from ml_amd import _lib
    C, lib = _lib.C, _lib.lib
    INVALID = _lib.E_INVALID_ARGUMENT
    P = _lib.dptr
    a = np.zeros(8)
    stand_in = C.create_string_buffer(8)
    fake = C.c_void_p(C.addressof(stand_in))                     # (only compared with NULL before the error is found)
    k = C.c_int()
    tail = (0, P(a), C.c_int64(1), None, C.c_int64(1), None)
    assert lib.mlhip_em_conditional_variances(None, None, 2, 1, P(a), P(a), P(a), P(a), P(a), P(a), *tail) == INVALID
    assert lib.mlhip_em_conditional_variances(fake, None, 2, 1, P(a), P(a), P(a), P(a), P(a), P(a), *tail) == INVALID
    assert lib.mlhip_em_condition_variance_route(None, 2, 1, 0, C.byref(k)) == INVALID
    assert lib.mlpp_em_conditional_variances(None, None, 0, None, C.c_uint64(0), 0, None, None) == INVALID


# ---- the restatement itself ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", SHAPES, ids=shape_id)
def test_the_float64_restatement_sits_at_rounding_of_the_longdouble_one_and_is_positive_definite(key):
    c = ref.case(*key)
    for form in ("diag", "full"):
        err = ref.error(c["v64"][form], c["vld"][form])
        print("VARIANCE restatement %s %s: float64 against longdouble %.2e, between-component share %.2f" %
              (shape_id(key), form, err, ref.between_share(c)))
        assert err <= 1e-14
    assert (c["v64"]["diag"] > 0).all()
    assert np.array_equal(np.diagonal(c["v64"]["full"], axis1=1, axis2=2) > 0, np.ones_like(c["v64"]["diag"], dtype=bool))
    sym = 0.5 * (c["v64"]["full"] + np.swapaxes(c["v64"]["full"], 1, 2))
    assert np.linalg.eigvalsh(sym).min() > 0


@pytest.mark.parametrize("key", [SHAPES[4], SHAPES[7], SHAPES[10], SHAPES[17]], ids=shape_id)
def test_the_centred_form_agrees_with_the_brute_force_second_moment(key):
    """sum_k r_k (C_k + t_k t_k^T) - y y^T in longdouble against the centred form, to 1e-15 of the largest variance."""
    c = ref.case(*key)
    ld = c["ld"]
    brute = ref.brute_force(ld["r"], ld["m"], ld["y"], c["Cld"])
    scale = np.abs(c["vld"]["full"]).max()
    assert float(np.abs(brute - c["vld"]["full"]).max() / scale) <= 1e-15
    assert float(np.abs(np.diagonal(brute, axis1=1, axis2=2) - c["vld"]["diag"]).max() / scale) <= 1e-15


def test_one_component_gives_its_conditioned_covariance():
    c = ref.case(2, 8, 1, (6, 1, 3, 4), N)
    for tag, mean, C in (("v64", "f64", c["C64"]), ("vld", "ld", c["Cld"])):
        assert (c[mean]["r"] == 1).all()
        assert np.array_equal(c[tag]["full"], np.broadcast_to(C[0], c[tag]["full"].shape))
        assert np.array_equal(c[tag]["diag"], np.broadcast_to(np.diag(C[0]), c[tag]["diag"].shape))
        assert not c[tag]["between"].any()


def test_some_accuracy_case_is_dominated_by_the_between_component_term():
    shares = {shape_id(k): ref.between_share(ref.case(*k)) for k in SHAPES}
    print("VARIANCE between-component shares: %s" % {k: round(v, 2) for k, v in shares.items()})
    assert max(shares.values()) > 0.5
