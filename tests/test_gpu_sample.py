"""mlhip_em_sample / mlhip_em_sample_data and EM.sample on the device against the numpy restatement of the definition
(tests/sample_reference.py): every coordinate within the derived tolerance of the longdouble form (L from mlhip_cholesky_lower),
labels equal; the statistical conditions the restatement meets on the CPU (tests/test_sample_host.py) on the device's own output; the
counter edges; and the bitwise invariants -- call splits, device groups, diagonal against full, tied against K copies, LDS table
against global table, handle form against an upload of the host form."""
import numpy as np
import pytest

import sample_reference as ref

pytestmark = pytest.mark.gpu

N = 4099            # 64 tiles of 64 rows and a ragged one


@pytest.fixture(scope="module")
def ctx():
    from ml_amd import _lib
    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def group():
    from ml_amd import _lib
    g = _lib.Context.group(3, device_ids=[0, 0, 0])
    yield g
    g.close()


_MODELS = {}


def model(d, K):
    """(mixing, means, covs, L) of the shape's mixture, L from the library; computed once."""
    from ml_amd import _lib
    if (d, K) not in _MODELS:
        mixing, means, covs = ref.parameters(d, K)
        _MODELS[d, K] = (mixing, means, covs, np.stack([_lib.cholesky_lower(S) for S in covs]))
    return _MODELS[d, K]


_REFERENCES = {}


def reference(d, K, n, seed, first_row=0):
    """The longdouble restatement and its tolerance; computed once per case and left unchanged."""
    key = (d, K, n, seed, first_row)
    if key not in _REFERENCES:
        mixing, means, _, L = model(d, K)
        _REFERENCES[key] = ref.sample(mixing, means, L, n, seed, first_row, dtype=np.longdouble, with_tolerance=True)
    return _REFERENCES[key]


def check_against_restatement(X, labels, d, K, n, seed, first_row=0):
    Xr, lr, tol = reference(d, K, n, seed, first_row)
    assert X.shape == (n, d) and X.flags.c_contiguous and labels.dtype == np.uint32
    assert np.array_equal(labels, lr), np.nonzero(labels != lr)[0][:10]
    ratio = float(np.max(np.abs(X.astype(np.longdouble) - Xr) / tol))
    print("d %d K %d n %d: worst error / tolerance %.3f" % (d, K, n, ratio))
    assert ratio <= 1, ratio


@pytest.mark.parametrize("d,K,route", [(1, 1, "lds_table"), (2, 3, "lds_table"), (3, 2, "lds_table"), (7, 40, "lds_table"),
                                       (13, 5, "lds_table"), (32, 8, None), (32, 64, "global_table"), (33, 3, None), (50, 2, "lds_table"),
                                       (64, 1, "lds_table"), (64, 4, None), (65, 2, "plain"), (130, 3, "plain")])
def test_against_the_restatement(ctx, monkeypatch, d, K, route):
    from ml_amd import _lib
    monkeypatch.delenv("MLHIP_SAMPLE_TABLE", raising=False)
    monkeypatch.delenv("MLHIP_SAMPLE_ROWS", raising=False)
    got = _lib.em_sample_route(d, K)
    assert got == route if route else got in ("lds_table", "global_table")   # (d <= 64: the register tier, whichever table)
    mixing, means, covs, _ = model(d, K)
    ctx.timing_enable(True)
    ctx.timing_reset()
    X, labels = ctx.em_sample(mixing, means, covs, N, seed=11)
    launches = ctx.timing_get("em_sample")[1]
    ctx.timing_enable(False)
    assert launches == 1
    check_against_restatement(X, labels, d, K, N, 11)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_draws(ctx, n):
    mixing, means, covs, _ = model(4, 3)
    X, labels = ctx.em_sample(mixing, means, covs, n, seed=5)
    check_against_restatement(X, labels, 4, 3, n, 5)


def test_an_empty_draw(ctx):
    mixing, means, covs, _ = model(4, 3)
    X, labels = ctx.em_sample(mixing, means, covs, 0, seed=5)
    assert X.shape == (0, 4) and labels.shape == (0,)
    data, labels = ctx.em_sample_data(mixing, means, covs, 0, seed=5)
    assert data.n_global == 0 and labels.shape == (0,)
    data.close()


@pytest.mark.parametrize("n,d,K,seed", ref.STATISTICAL_CASES)
def test_statistical_conditions_on_the_device_output(ctx, n, d, K, seed):
    mixing, means, covs, L = model(d, K)
    X, labels = ctx.em_sample(mixing, means, covs, n, seed=seed)
    count_z, mean_dev, cov_dev = ref.statistics(X, labels, mixing, means, L)
    print("n %d d %d K %d: count z %.2f, mean %.2f, covariance %.2f" % (n, d, K, count_z, mean_dev, cov_dev))
    assert count_z <= ref.STATISTICAL_BOUND and mean_dev <= ref.STATISTICAL_BOUND and cov_dev <= ref.STATISTICAL_BOUND


def test_counter_edges(ctx):
    mixing, means, covs, _ = model(13, 5)
    first = 2 ** 32 - 7                                          # the row index carries into the second counter word
    X, labels = ctx.em_sample(mixing, means, covs, 20, seed=3, first_row=first)
    check_against_restatement(X, labels, 13, 5, 20, 3, first)
    seed = 2 ** 32 + 2                                           # the second key word is nonzero
    X2, labels2 = ctx.em_sample(mixing, means, covs, 200, seed=seed)
    check_against_restatement(X2, labels2, 13, 5, 200, seed)
    X3, _ = ctx.em_sample(mixing, means, covs, 200, seed=2)
    assert not np.array_equal(X2, X3)


@pytest.mark.parametrize("d,K", [(13, 5), (32, 64), (65, 2)])
def test_call_splits_chunks_and_groups_give_the_same_bits(ctx, group, monkeypatch, d, K):
    mixing, means, covs, _ = model(d, K)
    monkeypatch.delenv("MLHIP_SAMPLE_ROWS", raising=False)
    X, labels = ctx.em_sample(mixing, means, covs, 1000, seed=21)
    Xa, la = ctx.em_sample(mixing, means, covs, 333, seed=21)
    Xb, lb = ctx.em_sample(mixing, means, covs, 667, seed=21, first_row=333)
    assert np.array_equal(np.vstack([Xa, Xb]), X) and np.array_equal(np.concatenate([la, lb]), labels)
    Xg, lg = group.em_sample(mixing, means, covs, 1000, seed=21)
    assert np.array_equal(Xg, X) and np.array_equal(lg, labels)
    monkeypatch.setenv("MLHIP_SAMPLE_ROWS", "192")               # six chunks inside one call, the last one ragged
    Xc, lc = ctx.em_sample(mixing, means, covs, 1000, seed=21)
    assert np.array_equal(Xc, X) and np.array_equal(lc, labels)


@pytest.mark.parametrize("d,K", [(64, 1), (65, 2)])
def test_one_launch_past_two_to_the_31_bytes(ctx, monkeypatch, d, K):
    """Byte offsets beyond 2^31 inside ONE launch (what the handle form does at such sizes): the block's last rows are the rows a small
    call draws at the same global indices."""
    mixing, means, covs, _ = model(d, K)
    n = 4_200_000                                                # n d 8 = 2.15e9 (d = 64) bytes
    monkeypatch.setenv("MLHIP_SAMPLE_ROWS", str(1 << 23))       # the whole draw is one chunk
    X, labels = ctx.em_sample(mixing, means, covs, n, seed=6)
    monkeypatch.delenv("MLHIP_SAMPLE_ROWS")
    for first in (0, n // 2 + 11, n - 100):
        Xs, ls = ctx.em_sample(mixing, means, covs, 100, seed=6, first_row=first)
        assert np.array_equal(X[first:first + 100], Xs) and np.array_equal(labels[first:first + 100], ls), first


@pytest.mark.parametrize("d,K", [(2, 3), (13, 5), (33, 3), (64, 1)])
def test_lds_and_global_tables_give_the_same_bits(ctx, monkeypatch, d, K):
    from ml_amd import _lib
    mixing, means, covs, _ = model(d, K)
    monkeypatch.delenv("MLHIP_SAMPLE_TABLE", raising=False)
    assert _lib.em_sample_route(d, K) == "lds_table"
    X, labels = ctx.em_sample(mixing, means, covs, N, seed=8)
    monkeypatch.setenv("MLHIP_SAMPLE_TABLE", "global")
    assert _lib.em_sample_route(d, K) == "global_table"
    Xg, lg = ctx.em_sample(mixing, means, covs, N, seed=8)
    assert np.array_equal(Xg, X) and np.array_equal(lg, labels)


@pytest.mark.parametrize("d,K", [(7, 4), (33, 3), (70, 2)])
def test_diagonal_and_tied_input(ctx, d, K):
    rng = np.random.default_rng(d)
    mixing, means, covs = ref.parameters(d, K)
    variances = rng.uniform(0.2, 3.0, (K, d))
    Xd, ld = ctx.em_sample(mixing, means, variances, 1500, seed=4, diagonal=True)
    Xf, lf = ctx.em_sample(mixing, means, np.stack([np.diag(v) for v in variances]), 1500, seed=4)
    assert np.array_equal(Xd, Xf) and np.array_equal(ld, lf)
    Xt, lt = ctx.em_sample(mixing, means, covs[0], 1500, seed=4, tied=True)
    Xk, lk = ctx.em_sample(mixing, means, np.stack([covs[0]] * K), 1500, seed=4)
    assert np.array_equal(Xt, Xk) and np.array_equal(lt, lk)
    assert np.array_equal(lt, ld)                                # (labels depend on the mixing weights alone)


@pytest.mark.parametrize("zero", [0, 2, 4])
def test_a_zero_weight_component_is_never_drawn(ctx, zero):
    mixing, means, covs, L = model(13, 5)
    mixing = mixing.copy()
    mixing[zero] = 0.0
    X, labels = ctx.em_sample(mixing, means, covs, N, seed=13)
    assert not np.any(labels == zero)
    want = ref.labels_of(mixing, 13, np.arange(N, dtype=np.uint64))
    assert np.array_equal(labels, want)
    Xr, lr, tol = ref.sample(mixing, means, L, N, 13, dtype=np.longdouble, with_tolerance=True)
    assert np.all(np.abs(X.astype(np.longdouble) - Xr) <= tol)


def test_only_one_output_and_errors(ctx):
    from ml_amd import _lib
    C, lib = _lib.C, _lib.lib
    mixing, means, covs, _ = model(4, 3)
    X, labels = ctx.em_sample(mixing, means, covs, 500, seed=2)
    only_x, only_l = np.empty((500, 4)), np.empty(500, dtype=np.uint32)
    args = (ctx.handle, C.c_uint32(4), C.c_uint32(3), 0, _lib.dptr(mixing), _lib.dptr(means), _lib.dptr(covs), C.c_uint64(2), C.c_uint64(0),
            C.c_uint64(500))
    assert lib.mlhip_em_sample(*args, _lib.dptr(only_x), C.c_int64(4), None) == 0 and np.array_equal(only_x, X)
    assert lib.mlhip_em_sample(*args, None, C.c_int64(4), _lib.u32ptr(only_l)) == 0 and np.array_equal(only_l, labels)
    wide = np.full((500, 6), -7.0)                               # ld > d: the rows land `ld` apart, the gaps stay
    assert lib.mlhip_em_sample(*args, _lib.dptr(wide), C.c_int64(6), None) == 0
    assert np.array_equal(wide[:, :4], X) and np.all(wide[:, 4:] == -7.0)
    bad = covs.copy()
    bad[1] = np.array([[1.0, 2.0, 0, 0], [2.0, 1.0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    with pytest.raises(ValueError):                              # MLHIP_E_DOMAIN: not positive definite, as in a fit
        ctx.em_sample(mixing, means, bad, 10)
    with pytest.raises(ValueError):
        ctx.em_sample(mixing, means, np.array([[1.0, -1.0, 1.0, 1.0]] * 3), 10, diagonal=True)


@pytest.mark.parametrize("grouped", [False, True])
def test_the_handle_form_is_the_upload_of_the_host_form(ctx, group, grouped):
    from ml_amd import _lib
    c = group if grouped else ctx
    mixing, means, covs, _ = model(13, 5)
    X, labels = c.em_sample(mixing, means, covs, N, seed=17)
    made, made_labels = c.em_sample_data(mixing, means, covs, N, seed=17)
    uploaded = _lib.Data(c, X)
    try:
        assert np.array_equal(made_labels, labels)
        assert made.n == N and made.d == 13 and made.n_global == N
        assert np.array_equal(made.shift, uploaded.shift)
        for a, b in zip(made.sample_covariance(), uploaded.sample_covariance()):
            assert np.array_equal(a, b)
        step_made, step_uploaded = made.em_step(mixing, means, covs), uploaded.em_step(mixing, means, covs)
        assert step_made[0] == step_uploaded[0]
        for a, b in zip(step_made[1:], step_uploaded[1:]):
            assert np.array_equal(a, b)
        if grouped:
            assert [made.shard_rows(s) for s in range(3)] == [uploaded.shard_rows(s) for s in range(3)]
    finally:
        made.close()
        uploaded.close()


def _training_block():
    mixing, means, covs, L = model(4, 3)
    return ref.sample(mixing, means, L, 3000, 99)[0]


@pytest.mark.parametrize("covariance_type", ["full", "diag", "tied"])
def test_model_sample_is_the_context_call_on_the_fitted_parameters(ctx, covariance_type):
    from ml_amd.cppyml import clustering
    X = _training_block()
    em = clustering.EM(3)
    em.set_seed(5)
    em.set_covariance_type(covariance_type)
    em.fit(X)
    S, labels = em.sample(2000, seed=9)
    assert S.shape == (2000, 4) and S.flags.c_contiguous and S.dtype == np.float64 and labels.dtype == np.uint32
    covs = np.stack([em.covariance(k) for k in range(3)])
    Sc, lc = ctx.em_sample(em.mixing_probabilities, np.ascontiguousarray(em.means.T), covs, 2000, seed=9)
    assert np.array_equal(S, Sc) and np.array_equal(labels, lc)
    again, _ = em.sample(2000, seed=9)
    other, _ = em.sample(2000, seed=10)
    assert np.array_equal(again, S) and not np.array_equal(other, S)
    shorter, _ = em.sample(100, seed=9)
    assert np.array_equal(shorter, S[:100])
    empty, empty_labels = em.sample(0)
    assert empty.shape == (0, 4) and empty_labels.shape == (0,)


def test_sample_leaves_the_models_random_engine_alone():
    from ml_amd.cppyml import clustering
    X = _training_block()

    def fits(sample_between):
        em = clustering.EM(3)
        em.set_seed(7)
        em.fit(X)
        if sample_between:
            em.sample(500, seed=1)
        em.fit(X)
        return em.log_likelihood, em.means.copy(), em.mixing_probabilities.copy()

    for a, b in zip(fits(False), fits(True)):
        assert np.array_equal(a, b)
