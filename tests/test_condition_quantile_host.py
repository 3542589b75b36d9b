"""Conditional CDF and quantiles, everything that needs no GPU: mlhip_em_condition_scales against the restatement
(tests/condition_quantile_reference.py), the argument errors of EM.conditional_cdf / EM.conditional_quantile and of the C entry points,
the exports, and the restatement against what does not go through it -- its longdouble Phi against mpmath at 40 digits, K = 1, the
bisection's quantiles through the CDF, its own float64 error on the shapes tests/test_gpu_condition_quantile.py uses, and the numpy
restatement of conditional_sample's draws for that file's seed. CPU only."""
import mpmath as mp
import numpy as np
import pytest

import condition_reference as cref
import condition_quantile_reference as ref
import condition_sample_reference as sref

LD = np.longdouble


def first(n):
    return tuple(range(n))


# the accuracy shapes of tests/test_gpu_condition_quantile.py (restated: that file needs a device)
N = 300
SHAPES = ([(1, 2, 2, (1,), n) for n in (1, 63, 65, 257)] +
          [(3, dO + dM, 3, first(dO), N) for dO, dM in ((1, 1), (3, 4), (4, 5), (8, 8), (9, 16), (16, 17), (32, 32), (33, 3), (3, 33))] +
          [(2, 8, K, (6, 1, 3, 4), N) for K in (1, 3, 64, 65)])
SAMPLE_KEY = (9, 4, 3, (2,), 16)
SAMPLE_SEED = 20261020
SAMPLE_P = (0.05, 0.5, 0.95)


def shape_id(s):
    return "d%d-K%d-dO%d-n%d" % (s[1], s[2], len(s[3]), s[4])


# ---- mlhip_em_condition_scales ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", [SHAPES[5], SHAPES[10], SHAPES[15]], ids=shape_id)
def test_scales_are_the_square_roots_of_the_conditioned_variances(key):
    from ml_amd import _lib
    c = ref.case(*key)
    C_m, _ = _lib.em_condition_covariances(c["covs"], c["observed"])
    s, w = _lib.em_condition_scales(C_m)
    dM = C_m.shape[1]
    assert np.array_equal(s, np.sqrt(C_m[:, np.arange(dM), np.arange(dM)])) and np.array_equal(w, 1.0 / s)      # one sqrt, one division
    assert float(np.abs(s.astype(LD) - c["sld"]).max() / c["sld"].max()) <= 1e-13          # (the conditioning's own rounding)
    assert s.shape == (len(c["mixing"]), dM) and s.flags.c_contiguous and w.flags.c_contiguous


def test_scales_of_a_diagonal_model_are_the_square_roots_of_its_variances_exactly():
    from ml_amd import _lib
    rng = np.random.default_rng(7)
    variances = rng.uniform(0.2, 3.0, (5, 9))
    observed = [7, 2, 3, 0]
    C_m, _ = _lib.em_condition_covariances(variances, observed, diagonal=True)
    s, w = _lib.em_condition_scales(C_m)
    M = cref.missing_of(9, observed)
    assert np.array_equal(s, np.sqrt(variances[:, M])) and np.array_equal(w, 1.0 / np.sqrt(variances[:, M]))


@pytest.mark.parametrize("bad", [0.0, -1.0, np.nan, np.inf, -np.inf])
def test_scales_of_a_variance_that_is_not_positive_and_finite_are_a_domain_error(bad):
    from ml_amd import _lib
    C_m = np.stack([np.eye(3), 2 * np.eye(3)])
    C_m[1, 2, 2] = bad
    s, w = np.empty((2, 3)), np.empty((2, 3))
    rc = _lib.lib.mlhip_em_condition_scales(2, 3, _lib.dptr(C_m), _lib.dptr(s), _lib.dptr(w))
    assert rc == _lib.E_DOMAIN
    with pytest.raises(ValueError):
        _lib.em_condition_scales(C_m)
    C_m[1, 2, 2] = 1.0
    C_m[0, 0, 1] = np.nan                                         # (off the diagonal: not read)
    assert np.array_equal(_lib.em_condition_scales(C_m)[0], np.sqrt(np.array([[1.0, 1, 1], [2, 2, 1]])))


# ---- argument errors without a device -----------------------------------------------------------------------------------------------------

def test_an_unfitted_model_raises_value_error():
    from ml_amd.cppyml import clustering
    with pytest.raises(ValueError, match="has not been fitted"):
        clustering.EM(3).conditional_cdf(np.zeros((4, 1)), [0], np.zeros((4, 1)))
    with pytest.raises(ValueError, match="has not been fitted"):
        clustering.EM(3).conditional_quantile(np.zeros((4, 1)), [0], [0.5])


def _exactly_fitted():
    from ml_amd.cppyml import clustering
    em = clustering.EM(2)
    assert em.fit(np.array([[0.0, 1.0, 2.0], [3.0, 5.0, 4.0]]))  # N == K: the exact fit needs no device
    return em


def test_the_model_surface_raises_before_device_work():
    em = _exactly_fitted()
    Y, V = np.zeros((10, 2)), np.zeros((10, 1))
    for bad in (Y.astype(np.float32), np.asfortranarray(Y), Y[:, 0], Y.tolist()):
        with pytest.raises(TypeError):
            em.conditional_cdf(bad, [0, 1], V)
        with pytest.raises(TypeError):
            em.conditional_quantile(bad, [0, 1], [0.5])
    for bad in ([0.5, 1], 3, None):
        with pytest.raises(TypeError):
            em.conditional_cdf(Y, bad, V)
        with pytest.raises(TypeError):
            em.conditional_quantile(Y, bad, [0.5])
    for bad in ([], [0, 1, 2], [0, 3], [-1, 0], [1, 1]):
        X = Y if len(bad) == 2 else np.zeros((10, max(len(bad), 1)))
        with pytest.raises(ValueError):
            em.conditional_cdf(X, bad, V)
        with pytest.raises(ValueError):
            em.conditional_quantile(X, bad, [0.5])
    with pytest.raises(ValueError, match="one column per observed coordinate"):
        em.conditional_cdf(np.zeros((10, 1)), [0, 1], V)
    with pytest.raises(ValueError, match="one column per observed coordinate"):
        em.conditional_quantile(np.zeros((10, 1)), [0, 1], [0.5])
    # values: C-contiguous float64 (N, dM)
    for bad in (V.astype(np.float32), np.zeros((10, 2))[:, :1], V[:, 0], V.tolist(), None):
        with pytest.raises(TypeError):
            em.conditional_cdf(Y, [0, 1], bad)
    for bad in (np.zeros((10, 2)), np.zeros((9, 1)), np.zeros((0, 1))):
        with pytest.raises(ValueError):
            em.conditional_cdf(Y, [0, 1], bad)
    # probabilities: a 1-D sequence of floats strictly inside (0, 1)
    for bad in ([0.0], [1.0], [0.5, -0.1], [1.5], [np.nan], [0.5, np.inf], 0.5, None, [[0.5]], ["a"]):
        with pytest.raises(ValueError):
            em.conditional_quantile(Y, [0, 1], bad)


def test_a_fitted_model_needs_a_device():
    from ml_amd import _lib
    if _lib.device_count() > 0:
        return                                                   # (a GPU is present: tests/test_gpu_condition_quantile.py has the other side)
    em = _exactly_fitted()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        em.conditional_cdf(np.zeros((10, 2)), [2, 0], np.zeros((10, 1)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        em.conditional_quantile(np.zeros((10, 2)), [2, 0], [0.05, 0.5])


def test_new_symbols_are_exported():
    from ml_amd import _lib
    from ml_amd.cppyml import clustering
    for name in ("mlhip_normal_cdf", "mlhip_normal_quantile", "mlhip_em_condition_scales", "mlhip_em_conditional_cdfs",
                 "mlhip_em_conditional_quantiles", "mlhip_em_condition_quantile_route",
                 "mlpp_em_conditional_cdfs", "mlpp_em_conditional_quantiles"):
        assert hasattr(_lib.lib, name), name
    for name in ("em_conditional_cdfs", "em_conditional_quantiles", "em_condition_quantile_route", "em_condition_scales", "normal_cdf",
                 "normal_quantile"):
        assert callable(getattr(_lib, name)) and not hasattr(_lib.Data, name), name
    assert callable(clustering.EM.conditional_cdf) and callable(clustering.EM.conditional_quantile)
    assert "`EM.conditional_cdf`" in clustering.__doc__ and "`EM.conditional_quantile`" in clustering.__doc__
    assert _lib.QUANTILE_MAX_TRIPS == 84


def test_entry_points_check_their_arguments_without_a_device():
    from ml_amd import _lib
    C, lib = _lib.C, _lib.lib
    INVALID = _lib.E_INVALID_ARGUMENT
    P = _lib.dptr
    a = np.full(8, 0.5)
    stand_in = C.create_string_buffer(8)
    fake = C.c_void_p(C.addressof(stand_in))                     # (only compared with NULL before the error is found)
    k = C.c_int()
    model = (P(a),) * 7
    cdf_tail = (P(a), C.c_int64(1), P(a), C.c_int64(1), None, C.c_int64(1), None)
    quantile_tail = (P(a), C.c_uint32(1), P(a), C.c_int64(1), None, C.c_int64(1), None, None)
    assert lib.mlhip_em_conditional_cdfs(None, None, 2, 1, *model, *cdf_tail) == INVALID
    assert lib.mlhip_em_conditional_cdfs(fake, None, 2, 1, *model, *cdf_tail) == INVALID
    assert lib.mlhip_em_conditional_quantiles(None, None, 2, 1, *model, *quantile_tail) == INVALID
    assert lib.mlhip_em_conditional_quantiles(fake, None, 2, 1, *model, *quantile_tail) == INVALID
    assert lib.mlhip_em_condition_quantile_route(None, 2, 1, 0, C.byref(k)) == INVALID
    assert lib.mlhip_em_condition_quantile_route(None, 2, 1, 1, C.byref(k)) == INVALID
    assert lib.mlpp_em_conditional_cdfs(None, None, 0, None, C.c_uint64(0), None, None) == INVALID
    assert lib.mlpp_em_conditional_quantiles(None, None, 0, None, C.c_uint64(0), None, C.c_uint64(0), None) == INVALID
    assert lib.mlhip_em_condition_scales(0, 1, P(a), P(a), P(a)) == INVALID
    assert lib.mlhip_em_condition_scales(1, 0, P(a), P(a), P(a)) == INVALID
    assert lib.mlhip_em_condition_scales(1, 1, None, P(a), P(a)) == INVALID
    assert lib.mlhip_em_condition_scales(1, 1, P(a), None, P(a)) == INVALID
    assert lib.mlhip_normal_cdf(None, C.c_uint64(1), P(a)) == INVALID and lib.mlhip_normal_cdf(None, C.c_uint64(0), None) == 0
    assert lib.mlhip_normal_quantile(P(a), C.c_uint64(1), None) == INVALID and lib.mlhip_normal_quantile(None, C.c_uint64(0), None) == 0


# ---- the restatement itself ---------------------------------------------------------------------------------------------------------------

def test_the_longdouble_cdf_against_forty_digits():
    """ncdf_ld carries the limits of the GPU tests: within 5e-17 of mpmath wherever Phi is a normal double, 1e-17 for |a| <= 20."""
    mp.mp.dps = 40
    a = np.concatenate([np.linspace(-37.0, 9.0, 1151), np.linspace(-3.2, 3.2, 641), [0.0, -1.5, 1.5, -3.0, 3.0]])
    F = ref.ncdf_ld(a)
    worst, worst_inner = 0.0, 0.0
    for x, f in zip(a, F):
        exact = mp.ncdf(mp.mpf(float(x)))
        hi = float(f)
        err = float(abs(mp.mpf(hi) + mp.mpf(float(f - LD(hi))) - exact) / exact)
        worst = max(worst, err)
        if abs(x) <= 20:
            worst_inner = max(worst_inner, err)
    print("ncdf_ld against mpmath: %.2e, |a| <= 20: %.2e" % (worst, worst_inner))
    assert worst <= 5e-17 and worst_inner <= 1e-17
    assert ref.ncdf_ld(np.array([0.0]))[0] == LD(0.5) and np.isnan(ref.ncdf_ld(np.array([np.nan]))[0])


@pytest.mark.parametrize("key", SHAPES, ids=shape_id)
def test_the_float64_restatement_sits_at_rounding_of_the_longdouble_one(key):
    c = ref.case(*key)
    err = ref.error(c["F64"], c["Fld"])
    print("CDF restatement %s: float64 against longdouble %.2e; F in [%.2e, %.6f]" % (shape_id(key), err, float(c["Fld"].min()), float(c["Fld"].max())))
    assert err <= 1e-13
    assert (c["Fld"] >= 0).all() and (c["Fld"] <= 1 + 1e-15).all()
    if len(c["values"]) > 8:
        assert c["Fld"].min() < 0.05 and c["Fld"].max() > 0.95   # the values reach both tails


def test_one_component_is_a_normal_distribution():
    c = ref.case(2, 8, 1, (6, 1, 3, 4), N)
    for mean, s in (("f64", c["s64"]), ("ld", c["sld"])):
        r, m = c[mean]["r"], c[mean]["m"]
        assert (r == 1).all()
        for p in (1e-9, 0.05, 0.5, 0.999):
            q = ref.quantile(r, m, s, p)
            want = m[:, 0] + s[0][None] * ref.nquantile(p, r.dtype.type)
            assert float(np.abs(q - want).max()) <= 4e-15 * float(np.abs(want).max())


@pytest.mark.parametrize("key", [SHAPES[5], SHAPES[7], SHAPES[14]], ids=shape_id)
def test_the_bisected_quantile_inverts_the_cdf(key):
    """In longdouble on the first 16 rows: F(q_p) = p S to the bracket's resolution, and the certificate the GPU test applies holds for
    the restatement's own float64 quantiles with the float64 restatement's responsibilities standing in for the E-step's."""
    c = ref.case(*key)
    r, m, s = c["ld"]["r"][:16], c["ld"]["m"][:16], c["sld"]
    for p in (1e-9, 0.05, 0.5, 0.999):
        q = ref.quantile(r, m, s, p)
        F = ref.cdf(r, m, s, q)
        T = LD(p) * r.sum(axis=1)[:, None]
        slope = ref.density(r, m, s, q)
        assert (np.abs(F - T) <= 1e-17 + 4 * slope * np.spacing(np.abs(q))).all(), p


def test_the_certificate_accepts_the_float64_restatement_and_rejects_a_shifted_quantile():
    from hp_limits import FLOOR
    key = SHAPES[5]
    c = ref.case(*key)
    r64 = c["f64"]["r"]
    q = ref.quantile(c["f64"]["r"], c["f64"]["m"], c["s64"], 0.05)
    ok, worst = ref.certificate(c, q, 0.05, r64, FLOOR)
    assert ok.all() and worst < 1
    ok, worst = ref.certificate(c, q + 1e-9 * c["s64"].min(), 0.05, r64, FLOOR)
    assert not ok.all() and worst > 1                            # a part in 1e9 of a scale is found out


def test_the_draws_of_the_gpu_tests_seed_agree_with_the_restatements_quantiles():
    """The numpy restatement of conditional_sample (tests/condition_sample_reference.py) with the seed tests/test_gpu_condition_quantile.py
    uses, 4096 draws for its 16 rows, against the restatement's own quantiles: all 144 shares within 4.5 binomial standard errors."""
    c = ref.case(*SAMPLE_KEY)
    draws = 4096
    X, _, _ = sref.sample(c["mixing"], c["means"], c["covs"], c["observed"], c["X_observed"], n_draws=draws, seed=SAMPLE_SEED)
    worst = 0.0
    for p in SAMPLE_P:
        q = ref.quantile(c["f64"]["r"], c["f64"]["m"], c["s64"], p)
        z = np.abs((X <= q[None]).mean(axis=0) - p) / np.sqrt(p * (1 - p) / draws)
        assert z.shape == (16, 3)
        worst = max(worst, float(z.max()))
    print("restated draws against restated quantiles: worst %.2f binomial standard errors" % worst)
    assert worst <= 4.5
