"""Conditional draws, everything that needs no GPU: mlhip_em_condition_covariances against the longdouble Schur complement of the numpy
restatement (tests/condition_sample_reference.py), the structure of its outputs, the label rule and the statistical conditions on
the restatement itself -- the ones tests/test_gpu_condition_sample.py asks of the device, so that the GPU test cannot fail for a
reason the definition has --, the margin condition of every accuracy case there, the exports and the argument errors. CPU only."""
import numpy as np
import pytest

import condition_reference as cref
import condition_sample_reference as ref
from hp_limits import FLOOR
from test_condition_host import SHAPES
from test_gpu_condition import SHAPES as GPU_SHAPES, shape_id

LD = np.longdouble


def _error(a, a_ld, scale):
    return float(np.abs(np.asarray(a, dtype=LD) - a_ld).max() / scale)


@pytest.mark.parametrize("d,observed", SHAPES, ids=lambda v: str(v) if isinstance(v, int) else "O%d" % len(v))
def test_condition_covariances_against_the_restatement(d, observed):
    """C_k against the longdouble Schur complement, relative to max |Sigma_MM|, within 4 max(err_f64, FLOOR), err_f64 the float64
    restatement's own error; G_k G_k^T = C_k by the same rule; C_k symmetric bit for bit, G_k lower with +0.0 above the diagonal."""
    from ml_amd import _lib
    K = 3
    _, _, covs = cref.model(d, d, K)
    C, G = _lib.em_condition_covariances(covs, observed)
    M = cref.missing_of(d, observed)
    assert C.shape == (K, len(M), len(M)) and G.shape == C.shape
    C64, _ = ref.covariances(covs, observed)
    Cld, _ = ref.covariances(covs, observed, LD)
    for k in range(K):
        scale = np.abs(covs[k][M][:, M]).max()
        err, err64 = _error(C[k], Cld[k], scale), _error(C64[k], Cld[k], scale)
        product = _error(G[k].astype(LD) @ G[k].astype(LD).T, Cld[k], scale)
        print("d %d dO %d k %d: C %.2e, float64 restatement %.2e, G G^T %.2e" % (d, len(observed), k, err, err64, product))
        limit = 4 * max(err64, FLOOR)
        assert err <= limit and product <= limit
        assert np.array_equal(C[k], C[k].T)
        assert not np.triu(G[k], 1).any() and not np.signbit(np.triu(G[k], 1)).any() and (np.diag(G[k]) > 0).all()
    # without the factors: the same covariances
    C_only = np.empty_like(C)
    obs = np.array(observed, dtype=np.uint32)
    rc = _lib.lib.mlhip_em_condition_covariances(d, K, 0, _lib.dptr(np.ascontiguousarray(covs)), _lib.u32ptr(obs), len(obs), _lib.dptr(C_only), None)
    assert rc == _lib.OK and np.array_equal(C_only, C)


def test_diagonal_input_is_exact_and_tied_input_gives_copies():
    from ml_amd import _lib
    rng = np.random.default_rng(5)
    K, d, observed = 4, 9, [7, 2, 3, 0]
    variances = rng.uniform(0.2, 3.0, (K, d))
    M = cref.missing_of(d, observed)
    C, G = _lib.em_condition_covariances(variances, observed, diagonal=True)
    assert np.array_equal(C, np.stack([np.diag(v[M]) for v in variances])) and not np.signbit(C).any()
    assert np.array_equal(G, np.stack([np.diag(np.sqrt(v[M])) for v in variances])) and not np.signbit(G).any()
    full = _lib.em_condition_covariances(np.stack([np.diag(v) for v in variances]), observed)
    assert np.array_equal(full[0], C) and np.array_equal(full[1], G)
    K, d, observed = 5, 11, [10, 4, 5, 1, 0, 8]
    _, _, covs = cref.model(3, d, K)
    C, G = _lib.em_condition_covariances(covs[0], observed, tied=True, K=K)
    for k in range(1, K):
        assert np.array_equal(C[k].view(np.uint64), C[0].view(np.uint64)) and np.array_equal(G[k].view(np.uint64), G[0].view(np.uint64))
    full = _lib.em_condition_covariances(np.stack([covs[0]] * K), observed)
    assert np.array_equal(full[0], C) and np.array_equal(full[1], G)


def test_condition_covariances_checks_its_arguments_and_refuses_indefinite_blocks():
    from ml_amd import _lib
    C, lib = _lib.C, _lib.lib
    P, U = _lib.dptr, _lib.u32ptr
    INVALID = _lib.E_INVALID_ARGUMENT
    K, d = 2, 4
    covs = np.stack([np.eye(d)] * K)
    obs = np.array([3, 1], dtype=np.uint32)
    C_m, G = np.full((K, 2, 2), 7.0), np.full((K, 2, 2), 7.0)
    good = dict(d=d, K=K, ctype=0, covs=P(covs), observed=U(obs), n_observed=2, C_m=P(C_m), G=P(G))

    def status(**change):
        a = dict(good, **change)
        return lib.mlhip_em_condition_covariances(C.c_uint32(a["d"]), C.c_uint32(a["K"]), a["ctype"], a["covs"], a["observed"],
                                                  C.c_uint32(a["n_observed"]), a["C_m"], a["G"])

    for name in ("covs", "observed", "C_m"):
        assert status(**{name: None}) == INVALID, name
    assert status(K=0) == INVALID and status(d=0) == INVALID and status(d=4097) == INVALID
    assert status(ctype=3) == INVALID and status(ctype=-1) == INVALID
    assert status(n_observed=0) == INVALID and status(n_observed=d) == INVALID and status(n_observed=d + 1) == INVALID
    assert status(observed=U(np.array([3, 4], dtype=np.uint32))) == INVALID
    assert status(observed=U(np.array([1, 1], dtype=np.uint32))) == INVALID
    assert (C_m == 7).all() and (G == 7).all()                   # before any work: nothing was written
    assert status() == _lib.OK and np.array_equal(C_m, np.stack([np.eye(2)] * K)) and np.array_equal(G, C_m)
    # Sigma_OO indefinite; Sigma_OO fine but the Schur complement not
    S = np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    with pytest.raises(ValueError, match="positive definite"):
        _lib.em_condition_covariances(S[None], [0, 1])
    with pytest.raises(ValueError, match="positive definite"):
        _lib.em_condition_covariances(S[None], [0])
    out = np.empty((1, 2, 2))
    one = np.array([0], dtype=np.uint32)
    assert lib.mlhip_em_condition_covariances(3, 1, 0, P(S), U(one), 1, P(out), None) == _lib.E_DOMAIN


def test_the_label_rule():
    u = np.array([0.0000001, 0.3, 0.5, 0.9999999])
    # a component without a share is never drawn, the last one included
    r = np.tile(np.array([0.25, 0.0, 0.75, 0.0]), (4, 1))
    labels, _ = ref.labels_of(r, u)
    assert labels.tolist() == [0, 2, 2, 2]
    r = np.tile(np.array([0.0, 1.0, 0.0]), (4, 1))
    assert ref.labels_of(r, u)[0].tolist() == [1, 1, 1, 1]
    # u S < s_k fails for every k only through rounding; then the largest k with a share takes the row
    r = np.array([[0.5, 0.5, 0.0]])
    assert ref.labels_of(r, np.array([1.0]))[0].tolist() == [1]
    # K = 1, and a NaN
    assert not ref.labels_of(np.ones((4, 1)), u)[0].any()
    assert ref.labels_of(np.array([[0.5, np.nan]]), np.array([0.1]))[0].tolist() == [ref.NO_LABEL]
    # every uniform of 10^5 rows against a column of zero shares in front, in the middle and at the end
    rows = np.arange(100000, dtype=np.uint64)
    r = np.tile(np.array([0.0, 0.3, 0.0, 0.7, 0.0]), (len(rows), 1))
    labels, _ = ref.labels_of(r, ref.uniforms(3, rows, 0))
    assert set(labels.tolist()) == {1, 3} and abs((labels == 1).mean() - 0.3) < 0.01


def test_the_streams_are_the_samplers_generator_with_another_fourth_word():
    import sample_reference as sref
    rows = np.arange(50, dtype=np.uint64) + np.uint64(2 ** 33)
    for block in (0, 1, 5):
        assert all(np.array_equal(a, b) for a, b in zip(ref.row_words(9, rows, block, 0), sref.row_words(9, rows, block)))
        assert not np.array_equal(ref.row_words(9, rows, block, 1)[0], sref.row_words(9, rows, block)[0])
    assert not np.any(ref.normals(9, rows, 6, 0)[0] == sref.normals(9, rows, 6)[0])
    assert not np.any(ref.normals(9, rows, 6, 0)[0] == ref.normals(9, rows, 6, 1)[0])


def test_the_statistical_conditions_hold_on_the_restatement():
    key = ref.MOMENTS_CASE
    c = ref.case(*key)
    X, _, _ = ref.sample(c["mixing"], c["means"], c["covs"], c["observed"], c["X_observed"], n_draws=1, seed=1, r=c["f64"]["r"])
    score = ref.moment_scores(c["X_observed"], c["X"][:, cref.missing_of(key[1], key[3])], X[0])
    print("moments on the restatement: %.2f standard errors" % score)
    assert score <= ref.STATISTICAL_BOUND
    c = ref.case(*ref.DRAWS_CASE)
    X, _, _ = ref.sample(c["mixing"], c["means"], c["covs"], c["observed"], c["X_observed"], n_draws=ref.DRAWS, seed=2, r=c["f64"]["r"])
    score = ref.draw_mean_scores(X, c["f64"]["y"])
    print("mean over %d draws on the restatement: %.2f standard errors" % (ref.DRAWS, score))
    assert score <= ref.STATISTICAL_BOUND


@pytest.mark.parametrize("key", GPU_SHAPES, ids=shape_id)
def test_no_row_of_the_accuracy_cases_lies_in_the_margin(key):
    """|u S - s_k| > 2^-40 S for every k with r_k > 0, on the float64 restatement's responsibilities, seeds 0 and 7, draws 0 .. 2."""
    c = ref.case(*key)
    rows = np.arange(key[4], dtype=np.uint64)
    smallest = np.inf
    for seed in (0, 7):
        for q in range(3):
            smallest = min(smallest, float(ref.labels_of(c["f64"]["r"], ref.uniforms(seed, rows, q))[1].min()))
    print("%s: smallest margin %.2e" % (shape_id(key), smallest))
    assert smallest > ref.MARGIN


def test_new_symbols_are_exported():
    from ml_amd import _lib
    from ml_amd.cppyml import clustering
    for name in ("mlhip_em_condition_covariances", "mlhip_em_conditional_samples", "mlhip_em_conditional_sample_route",
                 "mlpp_em_conditional_covariances", "mlpp_em_conditional_samples"):
        assert hasattr(_lib.lib, name), name
    assert callable(_lib.em_condition_covariances) and callable(_lib.Data.em_conditional_samples)
    assert callable(_lib.Data.em_conditional_sample_route)
    assert callable(clustering.EM.conditional_sample) and callable(clustering.EM.conditional_covariances)
    assert "`EM.conditional_sample`" in clustering.__doc__ and "`EM.conditional_covariances`" in clustering.__doc__


def test_entry_points_check_their_arguments_without_a_device():
    from ml_amd import _lib
    C, lib = _lib.C, _lib.lib
    INVALID = _lib.E_INVALID_ARGUMENT
    P = _lib.dptr
    a = np.zeros(8)
    stand_in = C.create_string_buffer(8)
    fake = C.c_void_p(C.addressof(stand_in))                     # (only compared with NULL before the error is found)
    k = C.c_int()
    tail = (C.c_uint64(0), C.c_uint64(0), C.c_uint32(0), C.c_uint32(1), P(a), C.c_int64(1), None)
    assert lib.mlhip_em_conditional_samples(None, None, 2, 1, P(a), P(a), P(a), P(a), P(a), P(a), *tail) == INVALID
    assert lib.mlhip_em_conditional_samples(fake, None, 2, 1, P(a), P(a), P(a), P(a), P(a), P(a), *tail) == INVALID
    assert lib.mlhip_em_conditional_sample_route(None, 2, 1, C.byref(k)) == INVALID
    assert lib.mlpp_em_conditional_samples(None, None, 0, None, C.c_uint64(0), C.c_uint64(1), C.c_uint64(0), None, None) == INVALID
    assert lib.mlpp_em_conditional_covariances(None, None, 0, None) == INVALID


def test_conditional_sample_raises_before_device_work_and_needs_a_device():
    from ml_amd import _lib
    from ml_amd.cppyml import clustering
    fresh = clustering.EM(2)
    X = np.zeros((10, 1))
    with pytest.raises(ValueError):                               # before a fit
        fresh.conditional_sample(X, [0])
    with pytest.raises(ValueError):
        fresh.conditional_covariances([0])
    em = clustering.EM(2)
    assert em.fit(np.array([[0.0, 1.0, 2.0], [3.0, 5.0, 4.0]]))  # N == K: the exact fit needs no device
    Y = np.zeros((10, 2))
    for bad in (Y.astype(np.float32), np.asfortranarray(Y), Y[:, 0], Y.tolist()):
        with pytest.raises(TypeError):
            em.conditional_sample(bad, [0, 1])
    for bad in ([0.5, 1], 3, None):
        with pytest.raises(TypeError):
            em.conditional_sample(Y, bad)
        with pytest.raises(TypeError):
            em.conditional_covariances(bad)
    for bad in ([], [0, 1, 2], [0, 3], [-1, 0], [1, 1]):
        with pytest.raises(ValueError):
            em.conditional_sample(Y if len(bad) == 2 else np.zeros((10, max(len(bad), 1))), bad)
        with pytest.raises(ValueError):
            em.conditional_covariances(bad)
    with pytest.raises(ValueError):
        em.conditional_sample(X, [0, 1])                          # one column, two coordinates
    for bad in (-1, 2 ** 32):
        with pytest.raises(ValueError):
            em.conditional_sample(Y, [0, 1], n_draws=bad)
    for bad in (1.5, "3", None, True):
        with pytest.raises(TypeError):
            em.conditional_sample(Y, [0, 1], n_draws=bad)
    with pytest.raises(ValueError):
        em.conditional_sample(Y, [0, 1], seed=-1)
    if _lib.device_count() > 0:
        return                                                   # (the rest is what happens WITHOUT a GPU; tests/test_gpu_condition_sample.py has the other side)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        em.conditional_sample(Y, [2, 0])
