"""Conditioning a mixture on known coordinates, everything that needs no GPU: mlhip_em_condition against the numpy restatement
(tests/condition_reference.py), the diagonal and tied special cases, the argument errors of the new entry points, the exports, and
the model surface's behaviour before any device work and without a device. CPU only."""
import numpy as np
import pytest

import condition_reference as ref

LD = np.longdouble
EPS = 2.0 ** -53

# (d, observed): the issue's shapes
SHAPES = [(3, [2, 0]), (8, [0, 2, 4, 6, 7]), (7, [6, 1, 3]), (32, list(range(16))), (70, [int(c) for c in np.random.default_rng(70).permutation(70)[:40]])]


@pytest.mark.parametrize("d,observed", SHAPES, ids=lambda v: str(v) if isinstance(v, int) else "O%d" % len(v))
def test_condition_against_the_restatement(d, observed):
    """The selections are copies, bit for bit. The maps are held to the longdouble restatement within 4 x the float64 restatement's
    own error or, where that is smaller, within the backward-error bound of the two triangular solves: (dO + 1) eps cond(Sigma_OO) per
    solve (Higham, Accuracy and Stability, thm 8.5 with the factor's own (dO + 1) eps), relative to the largest map."""
    from ml_amd import _lib
    K = 3
    _, means, covs = ref.model(d, d, K)
    mu_o, S_oo, A, mu_m = _lib.em_condition(means, covs, observed)
    M = ref.missing_of(d, observed)
    assert mu_o.shape == (K, len(observed)) and S_oo.shape == (K, len(observed), len(observed))
    assert A.shape == (K, len(M), len(observed)) and mu_m.shape == (K, len(M))
    assert np.array_equal(mu_o, means[:, observed]) and np.array_equal(mu_m, means[:, M])
    assert np.array_equal(S_oo, covs[:, observed][:, :, observed])
    _, _, A64, _, _ = ref.condition(means, covs, observed)
    _, _, Ald, _, _ = ref.condition(means, covs, observed, LD)
    for k in range(K):
        scale = np.abs(Ald[k]).max()
        err = float(np.abs(A[k].astype(LD) - Ald[k]).max() / scale)
        err64 = float(np.abs(A64[k].astype(LD) - Ald[k]).max() / scale)
        bound = 4 * (len(observed) + 1) * EPS * np.linalg.cond(S_oo[k])
        print("d %d dO %d k %d: maps %.2e, float64 restatement %.2e, solve bound %.2e" % (d, len(observed), k, err, err64, bound))
        assert err <= max(4 * err64, bound)


def test_diagonal_input_gives_maps_of_positive_zero():
    from ml_amd import _lib
    rng = np.random.default_rng(5)
    K, d, observed = 4, 9, [7, 2, 3, 0]
    means, variances = rng.standard_normal((K, d)), rng.uniform(0.2, 3.0, (K, d))
    mu_o, S_oo, A, mu_m = _lib.em_condition(means, variances, observed, diagonal=True)
    assert not A.any() and not np.signbit(A).any()
    assert np.array_equal(S_oo, np.stack([np.diag(v[observed]) for v in variances]))
    assert np.array_equal(mu_o, means[:, observed]) and np.array_equal(mu_m, means[:, ref.missing_of(d, observed)])
    # the same variances as full matrices: the same bits
    full = _lib.em_condition(means, np.stack([np.diag(v) for v in variances]), observed)
    for a, b in zip((mu_o, S_oo, A, mu_m), full):
        assert np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def test_tied_input_gives_k_maps_with_equal_bits():
    from ml_amd import _lib
    K, d, observed = 5, 11, [10, 4, 5, 1, 0, 8]
    _, means, covs = ref.model(3, d, K)
    mu_o, S_oo, A, mu_m = _lib.em_condition(means, covs[0], observed, tied=True)
    for k in range(1, K):
        assert np.array_equal(A[k].view(np.uint64), A[0].view(np.uint64)) and np.array_equal(S_oo[k], S_oo[0])
    full = _lib.em_condition(means, np.stack([covs[0]] * K), observed)
    for a, b in zip((mu_o, S_oo, A, mu_m), full):
        assert np.array_equal(a, b)


def _condition_status(lib, C, **a):
    return lib.mlhip_em_condition(C.c_uint32(a["d"]), C.c_uint32(a["K"]), a["ctype"], a["means"], a["covs"], a["observed"],
                                  C.c_uint32(a["n_observed"]), a["mu_o"], a["S_oo"], a["maps"], a["mu_m"])


def test_condition_checks_its_arguments():
    from ml_amd import _lib
    C, lib = _lib.C, _lib.lib
    P, U = _lib.dptr, _lib.u32ptr
    INVALID = _lib.E_INVALID_ARGUMENT
    K, d = 2, 4
    means, covs = np.zeros((K, d)), np.stack([np.eye(d)] * K)
    obs = np.array([3, 1], dtype=np.uint32)
    mu_o, S_oo, A, mu_m = np.full((K, 2), 7.0), np.full((K, 2, 2), 7.0), np.full((K, 2, 2), 7.0), np.full((K, 2), 7.0)
    good = dict(d=d, K=K, ctype=0, means=P(means), covs=P(covs), observed=U(obs), n_observed=2, mu_o=P(mu_o), S_oo=P(S_oo), maps=P(A), mu_m=P(mu_m))

    def status(**change):
        return _condition_status(lib, C, **dict(good, **change))

    for name in ("means", "covs", "observed", "mu_o", "S_oo", "maps", "mu_m"):
        assert status(**{name: None}) == INVALID, name
    assert status(K=0) == INVALID and status(d=0) == INVALID and status(d=4097) == INVALID
    assert status(ctype=3) == INVALID and status(ctype=-1) == INVALID
    assert status(n_observed=0) == INVALID and status(n_observed=d) == INVALID and status(n_observed=d + 1) == INVALID
    assert status(observed=U(np.array([3, 4], dtype=np.uint32))) == INVALID           # an index >= d
    assert status(observed=U(np.array([1, 1], dtype=np.uint32))) == INVALID           # a duplicate
    assert b"" != lib.mlhip_last_error()
    # before any work: nothing was written
    assert (mu_o == 7).all() and (S_oo == 7).all() and (A == 7).all() and (mu_m == 7).all()
    assert status() == _lib.OK and np.array_equal(A, np.zeros((K, 2, 2)))
    for bad in ([5, 1], [1, 1], [], [0, 1, 2, 3]):
        with pytest.raises(ValueError):
            _lib.em_condition(means, covs, bad)


def test_a_block_that_is_not_positive_definite_is_refused():
    from ml_amd import _lib
    S = np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    means = np.zeros((1, 3))
    with pytest.raises(ValueError, match="positive definite"):
        _lib.em_condition(means, S[None], [0, 1])
    out = [np.empty((1, 2)), np.empty((1, 2, 2)), np.empty((1, 1, 2)), np.empty((1, 1))]
    obs = np.array([0, 1], dtype=np.uint32)
    rc = _lib.lib.mlhip_em_condition(3, 1, 0, _lib.dptr(means), _lib.dptr(S), _lib.u32ptr(obs), 2, *[_lib.dptr(o) for o in out])
    assert rc == _lib.E_DOMAIN
    _lib.em_condition(means, S[None], [2])                        # (the block that IS positive definite conditions)
    with pytest.raises(ValueError):
        _lib.em_condition(means, np.zeros((1, 3)), [1], diagonal=True)


def test_conditional_means_entry_points_check_their_arguments_without_a_device():
    from ml_amd import _lib
    C, lib = _lib.C, _lib.lib
    INVALID = _lib.E_INVALID_ARGUMENT
    P = _lib.dptr
    a = np.zeros(8)
    stand_in = C.create_string_buffer(8)
    fake = C.c_void_p(C.addressof(stand_in))                     # (only compared with NULL before the error is found)
    k = C.c_int()
    assert lib.mlhip_em_conditional_means(None, None, 2, 1, P(a), P(a), P(a), P(a), P(a), P(a), C.c_int64(1), None) == INVALID
    assert lib.mlhip_em_conditional_means(fake, None, 2, 1, P(a), P(a), P(a), P(a), P(a), P(a), C.c_int64(1), None) == INVALID
    assert lib.mlhip_em_condition_route(None, 2, 1, C.byref(k)) == INVALID
    assert lib.mlpp_em_conditional_means(None, None, 0, None, C.c_uint64(0), None, None) == INVALID


def test_new_symbols_are_exported():
    from ml_amd import _lib
    from ml_amd.cppyml import clustering
    for name in ("mlhip_em_condition", "mlhip_em_conditional_means", "mlhip_em_condition_route", "mlpp_em_conditional_means"):
        assert hasattr(_lib.lib, name), name
    assert callable(_lib.em_condition) and callable(_lib.Data.em_conditional_means) and callable(_lib.Data.em_condition_route)
    assert callable(clustering.EM.conditional_mean)
    assert "`EM.conditional_mean`" in clustering.__doc__


def test_conditional_mean_raises_before_device_work_and_needs_a_device():
    from ml_amd import _lib
    from ml_amd.cppyml import clustering
    fresh = clustering.EM(2)
    X = np.zeros((10, 1))
    with pytest.raises(ValueError):                               # before a fit
        fresh.conditional_mean(X, [0])
    em = clustering.EM(2)
    assert em.fit(np.array([[0.0, 1.0, 2.0], [3.0, 5.0, 4.0]]))  # N == K: the exact fit needs no device
    Y = np.zeros((10, 2))
    for bad in (Y.astype(np.float32), np.asfortranarray(Y), Y[:, 0], Y.tolist()):
        with pytest.raises(TypeError):
            em.conditional_mean(bad, [0, 1])
    for bad in ([0.5, 1], 3, None):
        with pytest.raises(TypeError):
            em.conditional_mean(Y, bad)
    for bad in ([], [0, 1, 2], [0, 3], [-1, 0], [1, 1]):
        with pytest.raises(ValueError):
            em.conditional_mean(Y if len(bad) == 2 else np.zeros((10, max(len(bad), 1))), bad)
    with pytest.raises(ValueError):
        em.conditional_mean(X, [0, 1])                            # one column, two coordinates
    if _lib.device_count() > 0:
        return                                                   # (the rest is what happens WITHOUT a GPU; tests/test_gpu_condition.py has the other side)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        em.conditional_mean(Y, [2, 0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        em.conditional_mean(np.zeros((0, 1)), [1], return_log_density=True)
