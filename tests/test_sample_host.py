"""The sampler's definition and everything of it that needs no GPU: Philox known answers, the numpy restatement
(tests/sample_reference.py) against the statistical conditions the device's output is held to, prefix and seam of the restatement,
mlhip_cholesky_lower against Higham's bound, the argument errors of the new entry points, and the four surfaces' behaviour without a
device. CPU only."""
import numpy as np
import pytest

import sample_reference as ref


@pytest.mark.parametrize("counter,key,expected", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, expected):
    got = tuple(int(w[0]) for w in ref.philox4x32_10(counter, key))
    assert got == expected, [hex(v) for v in got]


def test_uniform_is_exact_and_strictly_inside_the_unit_interval():
    lo = np.array([0, 0xffffffff, 0x00000fff, 0x00001000], dtype=np.uint64)
    hi = np.array([0, 0xffffffff, 0, 0], dtype=np.uint64)
    u = ref.uniform(lo, hi)
    assert u[0] == 2.0 ** -53 and u[1] == 1 - 2.0 ** -53 and u[2] == u[0] and u[3] == 1.5 * 2.0 ** -52
    assert np.array_equal(ref.uniform(lo, hi, np.longdouble).astype(np.float64), u)


def _factors(covs):
    return np.stack([np.linalg.cholesky(S) for S in covs])


@pytest.mark.parametrize("n,d,K,seed", ref.STATISTICAL_CASES)
def test_the_restatement_meets_the_statistical_conditions(n, d, K, seed):
    mixing, means, covs = ref.parameters(d, K)
    L = _factors(covs)
    X, labels = ref.sample(mixing, means, L, n, seed)
    count_z, mean_dev, cov_dev = ref.statistics(X, labels, mixing, means, L)
    print("n %d d %d K %d: count z %.2f, mean %.2f, covariance %.2f" % (n, d, K, count_z, mean_dev, cov_dev))
    assert count_z <= ref.STATISTICAL_BOUND and mean_dev <= ref.STATISTICAL_BOUND and cov_dev <= ref.STATISTICAL_BOUND


def test_restatement_prefix_and_seam():
    mixing, means, covs = ref.parameters(13, 5)
    L = _factors(covs)
    X, labels = ref.sample(mixing, means, L, 4099, 2)
    Xa, la = ref.sample(mixing, means, L, 100, 2)
    Xb, lb = ref.sample(mixing, means, L, 50, 2, first_row=50)
    assert np.array_equal(Xa, X[:100]) and np.array_equal(la, labels[:100])
    assert np.array_equal(Xb, X[50:100]) and np.array_equal(lb, labels[50:100])


def test_float64_and_longdouble_restatements_agree_within_the_tolerance():
    """numpy's float64 stands in for the device: the tolerance leaves a correct evaluation room."""
    for d, K in ((2, 3), (13, 5), (33, 3)):
        mixing, means, covs = ref.parameters(d, K)
        L = _factors(covs)
        X, labels = ref.sample(mixing, means, L, 1000, 7)
        Xl, ll, tol = ref.sample(mixing, means, L, 1000, 7, dtype=np.longdouble, with_tolerance=True)
        assert np.array_equal(labels, ll)
        ratio = np.max(np.abs(X.astype(np.longdouble) - Xl) / tol)
        print("d %d K %d: worst error / tolerance %.3f" % (d, K, ratio))
        assert ratio <= 1


# ---- mlhip_cholesky_lower ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [1, 2, 7, 33, 47, 48, 65, 130])
def test_cholesky_lower_meets_highams_bound(d):
    from ml_amd import _lib
    rng = np.random.default_rng(d)
    A = rng.standard_normal((d, d))
    S = A @ A.T / d + 0.5 * np.eye(d)
    S = 0.5 * (S + S.T)
    L = _lib.cholesky_lower(S)
    assert np.array_equal(np.triu(L, 1), np.zeros((d, d)))
    Lx = L.astype(np.longdouble)
    m = d + 1
    gamma = m * ref.EPS / (1 - m * ref.EPS)
    residual = np.abs(Lx @ Lx.T - S.astype(np.longdouble))
    bound = gamma * (np.abs(Lx) @ np.abs(Lx).T)
    assert np.all(residual <= bound), float(np.max(residual / bound))


def test_cholesky_lower_of_a_diagonal_matrix_is_the_square_root_exactly():
    from ml_amd import _lib
    v = np.random.default_rng(3).uniform(0.1, 9.0, 50)
    assert np.array_equal(_lib.cholesky_lower(np.diag(v)), np.diag(np.sqrt(v)))
    assert np.array_equal(_lib.cholesky_lower(np.diag(v[:5])), np.diag(np.sqrt(v[:5])))


def test_cholesky_lower_refuses_an_indefinite_matrix():
    from ml_amd import _lib
    S = np.array([[1.0, 2.0], [2.0, 1.0]])
    out = np.empty((2, 2))
    assert _lib.lib.mlhip_cholesky_lower(2, _lib.dptr(S), _lib.dptr(out)) == _lib.E_DOMAIN
    with pytest.raises(ValueError):
        _lib.cholesky_lower(S)
    with pytest.raises(ValueError):
        _lib.cholesky_lower(np.zeros((3, 3)))
    assert _lib.lib.mlhip_cholesky_lower(0, _lib.dptr(S), _lib.dptr(out)) == _lib.E_INVALID_ARGUMENT
    assert _lib.lib.mlhip_cholesky_lower(2, None, _lib.dptr(out)) == _lib.E_INVALID_ARGUMENT


# ---- argument errors, exports, surfaces without a device --------------------------------------------------------------------------

def _call(C, lib, ctx, d, K, ctype, mixing, means, covs, seed, first_row, n, x, ld, labels):
    return lib.mlhip_em_sample(ctx, C.c_uint32(d), C.c_uint32(K), ctype, mixing, means, covs, C.c_uint64(seed), C.c_uint64(first_row),
                               C.c_uint64(n), x, C.c_int64(ld), labels)


def test_sampling_entry_points_check_their_arguments_without_a_device():
    """Every argument error is raised before any device work: a context pointer that is never dereferenced stands in for one."""
    from ml_amd import _lib
    C, lib = _lib.C, _lib.lib
    d, K, n = 3, 2, 10
    pi, mu, S = np.array([0.25, 0.75]), np.zeros((K, d)), np.stack([np.eye(d)] * K)
    X, lab = np.empty((n, d)), np.empty(n, dtype=np.uint32)
    stand_in = C.create_string_buffer(8)
    fake = C.c_void_p(C.addressof(stand_in))                     # (only compared with NULL before the error is found)
    P, U = _lib.dptr, _lib.u32ptr
    INVALID = _lib.E_INVALID_ARGUMENT
    good = dict(ctx=fake, d=d, K=K, ctype=0, mixing=P(pi), means=P(mu), covs=P(S), seed=1, first_row=0, n=n, x=P(X), ld=d, labels=U(lab))

    def status(**change):
        return _call(C, lib, **dict(good, **change))

    assert status(ctx=None) == INVALID
    assert status(mixing=None) == INVALID and status(means=None) == INVALID and status(covs=None) == INVALID
    assert status(x=None, labels=None) == INVALID
    assert status(K=0) == INVALID and status(d=0) == INVALID and status(d=4097) == INVALID
    assert status(ctype=3) == INVALID and status(ctype=-1) == INVALID
    assert status(ld=d - 1) == INVALID
    assert status(first_row=2 ** 64 - 5, n=10) == INVALID
    for bad in ([-0.25, 1.25], [np.nan, 1.0], [np.inf, 1.0], [0.0, 0.0]):
        assert status(mixing=P(np.array(bad))) == INVALID, bad
    for bad in (np.nan, np.inf):
        m = mu.copy()
        m[1, 2] = bad
        assert status(means=P(m)) == INVALID
    assert b"" != lib.mlhip_last_error()

    handle = C.c_void_p()

    def data_status(**change):
        a = dict(good, **change)
        return lib.mlhip_em_sample_data(a["ctx"], C.c_uint32(a["d"]), C.c_uint32(a["K"]), a["ctype"], a["mixing"], a["means"], a["covs"],
                                        C.c_uint64(a["seed"]), C.c_uint64(a["first_row"]), C.c_uint64(a["n"]), a["labels"],
                                        a.get("out", C.byref(handle)))

    assert data_status(ctx=None) == INVALID and data_status(out=None) == INVALID
    assert data_status(K=0) == INVALID and data_status(d=0) == INVALID and data_status(d=4097) == INVALID and data_status(ctype=7) == INVALID
    assert data_status(mixing=P(np.array([-1.0, 2.0]))) == INVALID
    assert data_status(first_row=2 ** 64 - 5, n=10) == INVALID
    assert data_status(n=2 ** 32) == INVALID                      # beyond the per-rank row limit of mlhip_data_upload
    assert not handle.value

    k = C.c_int()
    assert lib.mlhip_em_sample_route(0, 2, C.byref(k)) == INVALID and lib.mlhip_em_sample_route(4097, 2, C.byref(k)) == INVALID
    assert lib.mlhip_em_sample_route(3, 0, C.byref(k)) == INVALID and lib.mlhip_em_sample_route(3, 2, None) == INVALID


def test_sample_route_cut_offs(monkeypatch):
    """The documented cut-offs (mlhip.h): the table in LDS while K (d (d+1)/2 + d) doubles fit beside the staging tile and the thresholds
    in 64 KiB, the plain tier above d = 64; MLHIP_SAMPLE_TABLE=global moves the LDS-table shapes to the global table."""
    from ml_amd import _lib
    monkeypatch.delenv("MLHIP_SAMPLE_TABLE", raising=False)
    for d, K, want in ((1, 1, "lds_table"), (2, 3, "lds_table"), (7, 40, "lds_table"), (13, 5, "lds_table"), (32, 64, "global_table"),
                       (64, 4, "global_table"), (64, 1, "lds_table"), (65, 2, "plain"), (130, 3, "plain"), (4096, 1, "plain")):
        assert _lib.em_sample_route(d, K) == want, (d, K)
        waves = 4 if d <= 16 else 2 if d <= 32 else 1
        fits = 8 * (waves * 64 * (d | 1) + (K if K <= 2048 else 0) + K * (d * (d + 1) // 2 + d)) <= 64 * 1024
        assert d > 64 or (want == "lds_table") == fits
    monkeypatch.setenv("MLHIP_SAMPLE_TABLE", "global")
    assert _lib.em_sample_route(2, 3) == "global_table" and _lib.em_sample_route(65, 2) == "plain"


def test_new_symbols_are_exported():
    from ml_amd import _lib
    for name in ("mlhip_em_sample", "mlhip_em_sample_data", "mlhip_cholesky_lower", "mlhip_em_sample_route", "mlpp_em_sample"):
        assert hasattr(_lib.lib, name), name
    assert callable(_lib.Context.em_sample) and callable(_lib.Context.em_sample_data) and callable(_lib.Data.adopt)


def test_sample_needs_a_device_and_a_fitted_model():
    from ml_amd import _lib
    from ml_amd.cppyml import clustering
    fresh = clustering.EM(2)
    Y = np.zeros((10, 3))
    with pytest.raises(Exception) as unfitted_score:
        fresh.score_samples(Y)
    with pytest.raises(type(unfitted_score.value)):              # before a fit: as score_samples fails
        fresh.sample(10)
    with pytest.raises(ValueError):
        fresh.sample(-1)
    if _lib.device_count() > 0:
        return                                                   # (the rest is what happens WITHOUT a GPU; tests/test_gpu_sample.py has the other side)
    em = clustering.EM(2)
    assert em.fit(np.array([[0.0, 1.0, 2.0], [3.0, 5.0, 4.0]]))  # N == K: the exact fit needs no device
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        em.sample(10)
    with pytest.raises(ValueError):
        em.sample(-1)                                            # (argument errors still come first)
