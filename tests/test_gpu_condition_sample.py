"""mlhip_em_conditional_samples and EM.conditional_sample on the device against the numpy restatement of the definition
(tests/condition_sample_reference.py), on the shapes of tests/test_gpu_condition.py. Parameters go in directly through
Data.em_conditional_samples, conditioned by the library's own host helpers (held by tests/test_condition_host.py and
tests/test_condition_sample_host.py).

Accuracy. Labels: the restatement's label rule on the responsibilities the existing E-step kernels give for the marginal parameters
on the same handle (mlhip_em_expectation + mlhip_em_responsibilities) must give the device's label on every row outside the margin
|u S - s_k| <= 2^-40 S (any k with r_k > 0); tests/test_condition_sample_host.py shows on the float64 restatement that no row of these
cases lies inside it, and the count left out is asserted to be 0 here. Values: against the longdouble restatement under the device's
labels, per coordinate within
    (dO + dM + 3) eps (|mu_M,j| + sum_c |A_jc| |z_c| + sum_c |G_jc| |zeta_c|) + 16 eps sum_c |G_jc| rad_c,   eps = 2^-52
(sample_reference.tolerance with the dO terms of the map chain: a derivation, not a measurement). One line per case is printed with
the worst ratio; over all cases it was 0.18 on an MI355X.

Bitwise: chunks, a prefix of a longer block, a call split over first_row, a draw of a longer call against a call of its own, device
groups, the plain tier against the register tier. Definition checks: a separated mixture, K = 1 with a diagonal model, seeds and
draws, no normal shared with EM.sample. Statistical checks at fixed seeds, bounds of 5 standard errors (the same conditions hold on the
float64 restatement: tests/test_condition_sample_host.py). Then the model surface."""
import numpy as np
import pytest

import condition_reference as cref
import condition_sample_reference as ref
import sample_reference as sref
from test_gpu_condition import CHUNKED, SHAPES, expected_route, first, separated, shape_id

pytestmark = pytest.mark.gpu

SWITCHES = ("MLHIP_CONDITION", "MLHIP_CONDITION_ROWS", "MLHIP_CONDITION_SKIP", "MLHIP_SCORE", "MLHIP_SCORE_ROWS")
LD = np.longdouble
SEED, DRAWS = 7, 3


@pytest.fixture(scope="module")
def ctx():
    from ml_amd import _lib
    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


_CONDITIONED = {}


def conditioned(key):
    """ref.case(*key) with the library's own conditioning of its model beside it: (case, (mu_o, S_oo, A, mu_m, G)); computed once."""
    from ml_amd import _lib
    if key not in _CONDITIONED:
        c = ref.case(*key)
        _, G = _lib.em_condition_covariances(c["covs"], c["observed"])
        _CONDITIONED[key] = (c, _lib.em_condition(c["means"], c["covs"], c["observed"]) + (G,))
    return _CONDITIONED[key]


def on_device(context, key, rows=None, start=0, **kw):
    """Rows [start, rows) of the case's block as a block of their own (first_row stays the caller's)."""
    from ml_amd import _lib
    c, model = conditioned(key)
    X = np.ascontiguousarray(c["X_observed"][start:rows])
    data = _lib.Data(context, X)
    kw.setdefault("seed", SEED)
    kw.setdefault("n_draws", DRAWS)
    out = data.em_conditional_samples(c["mixing"], *model, **kw)
    data.close()
    return out


def bits(a):
    return a.view(np.uint64)


@pytest.mark.parametrize("key", SHAPES, ids=shape_id)
def test_against_the_restatement(ctx, key):
    from ml_amd import _lib
    _, d, K, observed, n = key
    dO, dM = len(observed), d - len(observed)
    c, (mu_o, S_oo, A, mu_m, G) = conditioned(key)
    data = _lib.Data(ctx, c["X_observed"])
    assert data.em_conditional_sample_route(K, dM) == expected_route(dO, dM)
    ctx.timing_enable(True)
    ctx.timing_reset()
    X, labels = data.em_conditional_samples(c["mixing"], mu_o, S_oo, A, mu_m, G, n_draws=DRAWS, seed=SEED, labels=True)
    launches = ctx.timing_get("em_condition_sample")[1]
    ctx.timing_enable(False)
    data.em_expectation(c["mixing"], mu_o, S_oo)
    R = data.em_responsibilities(K)
    data.close()
    assert launches == 1
    assert X.shape == (DRAWS, n, dM) and X.flags.c_contiguous and X.dtype == np.float64
    assert labels.shape == (DRAWS, n) and labels.dtype == np.uint32
    rows = np.arange(n, dtype=np.uint64)
    worst, left_out = 0.0, 0
    for q in range(DRAWS):
        want, margin = ref.labels_of(R, ref.uniforms(SEED, rows, q))
        decided = margin > ref.MARGIN
        left_out += int((~decided).sum())
        assert np.array_equal(labels[q][decided], want[decided]), (q, np.nonzero(labels[q] != want)[0][:8])
        zeta, rad = ref.normals(SEED, rows, dM, q, LD)
        x_ld = ref.rows_given(labels[q], c["X_observed"], mu_o, A, mu_m, G, zeta, LD)
        tol = ref.tolerance(labels[q], c["X_observed"], mu_o, A, mu_m, G, zeta, rad)
        ratio = float(np.max(np.abs(X[q].astype(LD) - x_ld) / tol))
        assert ratio <= 1.0, (q, ratio)
        worst = max(worst, ratio)
    print("CONDITION SAMPLE %s: worst error / tolerance %.3f, rows left out of the label comparison %d" % (shape_id(key), worst, left_out))
    assert left_out == 0


# ---- bitwise invariants -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", CHUNKED, ids=shape_id)
@pytest.mark.parametrize("rows", ["64", "192", "512"])
def test_chunk_rows_give_the_bits_of_one_chunk(ctx, monkeypatch, key, rows):
    X, labels = on_device(ctx, key, labels=True)
    monkeypatch.setenv("MLHIP_CONDITION_ROWS", rows)
    ctx.timing_enable(True)
    ctx.timing_reset()
    X_c, labels_c = on_device(ctx, key, labels=True)
    launches = ctx.timing_get("em_condition_sample")[1]
    ctx.timing_enable(False)
    chunk = -(-int(rows) // 256) * 256
    assert launches == -(-key[4] // chunk) and launches > 1
    assert np.array_equal(bits(X_c), bits(X)) and np.array_equal(labels_c, labels)


@pytest.mark.parametrize("key", CHUNKED, ids=shape_id)
def test_prefixes_and_row_splits_give_the_bits_of_the_whole_block(ctx, key):
    X, labels = on_device(ctx, key, labels=True)
    for n in (1, 63, 300, 513):
        X_p, labels_p = on_device(ctx, key, rows=n, labels=True)
        assert np.array_equal(bits(X_p), bits(X[:, :n])) and np.array_equal(labels_p, labels[:, :n]), n
    for a, b in ((1, 64), (63, 321), (300, 513), (513, key[4])):
        X_s, labels_s = on_device(ctx, key, rows=b, start=a, first_row=a, labels=True)
        assert np.array_equal(bits(X_s), bits(X[:, a:b])) and np.array_equal(labels_s, labels[:, a:b]), (a, b)
    # the same rows under other global indices are other draws
    assert not np.array_equal(on_device(ctx, key, rows=64, start=1, first_row=0), X[:, 1:64])


@pytest.mark.parametrize("key", CHUNKED, ids=shape_id)
def test_a_draw_of_a_longer_call_has_the_bits_of_a_call_of_its_own(ctx, key):
    """(eleven draws: the register tier labels eight at a time)"""
    X, labels = on_device(ctx, key, n_draws=11, labels=True)
    assert np.array_equal(bits(X[:DRAWS]), bits(on_device(ctx, key)))
    for q in (0, 1, 2, 7, 8, 10):
        X_q, labels_q = on_device(ctx, key, n_draws=1, first_draw=q, labels=True)
        assert np.array_equal(bits(X_q[0]), bits(X[q])) and np.array_equal(labels_q[0], labels[q]), q
    X_t = on_device(ctx, key, n_draws=4, first_draw=7)
    assert np.array_equal(bits(X_t), bits(X[7:]))


@pytest.mark.parametrize("shards", [2, 3])
@pytest.mark.parametrize("key", CHUNKED, ids=shape_id)
def test_a_device_group_gives_the_single_context_bits(ctx, key, shards):
    from ml_amd import _lib
    X, labels = on_device(ctx, key, labels=True, first_row=5)
    group = _lib.Context.group(shards, device_ids=[0] * shards)
    try:
        X_g, labels_g = on_device(group, key, labels=True, first_row=5)
    finally:
        group.close()
    assert np.array_equal(bits(X_g), bits(X)) and np.array_equal(labels_g, labels)


@pytest.mark.parametrize("key", [SHAPES[6], SHAPES[8], SHAPES[13], SHAPES[17], SHAPES[20]], ids=shape_id)
def test_the_plain_tier_gives_the_bits_of_the_register_tier(ctx, monkeypatch, key):
    from ml_amd import _lib
    X, labels = on_device(ctx, key, labels=True)
    monkeypatch.setenv("MLHIP_CONDITION", "plain")
    c, model = conditioned(key)
    data = _lib.Data(ctx, c["X_observed"][:1])
    assert data.em_conditional_sample_route(len(c["mixing"]), model[3].shape[1]) == "plain"
    data.close()
    X_p, labels_p = on_device(ctx, key, labels=True)
    assert np.array_equal(bits(X_p), bits(X)) and np.array_equal(labels_p, labels)


# ---- definition checks ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tier", ["registers", "plain"])
def test_a_separated_mixture_draws_every_row_from_its_own_component(ctx, monkeypatch, tier):
    from ml_amd import _lib
    mixing, means, covs, X_o, observed = separated()
    K = len(mixing)
    mu_o, S_oo, A, mu_m = _lib.em_condition(means, covs, observed)
    _, G = _lib.em_condition_covariances(covs, observed)
    if tier == "plain":
        monkeypatch.setenv("MLHIP_CONDITION", "plain")
    data = _lib.Data(ctx, X_o)
    assert data.em_conditional_sample_route(K, A.shape[1]) == tier
    X, labels = data.em_conditional_samples(mixing, mu_o, S_oo, A, mu_m, G, n_draws=2, seed=3, labels=True)
    data.close()
    own = np.repeat(np.arange(K), len(X_o) // K).astype(np.uint32)
    assert np.array_equal(labels[0], own) and np.array_equal(labels[1], own)
    assert np.isfinite(X).all()


def test_one_diagonal_component_is_the_mean_plus_sigma_times_the_normals(ctx):
    from ml_amd import _lib
    rng = np.random.default_rng(51)
    d, observed, n = 9, [7, 2, 3, 0], 200
    means, variances = 2.5 * rng.standard_normal((1, d)), rng.uniform(0.5, 2.0, (1, d))
    X_o = np.ascontiguousarray((means + np.sqrt(variances) * rng.standard_normal((n, d)))[:, observed])
    mu_o, S_oo, A, mu_m = _lib.em_condition(means, variances, observed, diagonal=True)
    C_m, G = _lib.em_condition_covariances(variances, observed, diagonal=True)
    M = cref.missing_of(d, observed)
    assert np.array_equal(C_m[0], np.diag(variances[0, M])) and np.array_equal(G[0], np.diag(np.sqrt(variances[0, M])))
    data = _lib.Data(ctx, X_o)
    X, labels = data.em_conditional_samples(np.ones(1), mu_o, S_oo, A, mu_m, G, n_draws=2, seed=9, labels=True)
    data.close()
    assert not labels.any()
    rows = np.arange(n, dtype=np.uint64)
    for q in range(2):
        zeta, rad = ref.normals(9, rows, len(M), q, LD)
        want = mu_m[0].astype(LD) + np.sqrt(variances[0, M]).astype(LD) * zeta
        tol = ref.tolerance(labels[q], X_o, mu_o, A, mu_m, G, zeta, rad)
        assert np.all(np.abs(X[q].astype(LD) - want) <= tol)


def test_seeds_and_draws_differ_and_share_nothing_with_the_sampler(ctx):
    from ml_amd import _lib
    key = CHUNKED[1]
    c, (mu_o, S_oo, A, mu_m, G) = conditioned(key)
    X = on_device(ctx, key, seed=SEED, n_draws=2)
    assert not np.any(X[0] == X[1])
    assert not np.any(on_device(ctx, key, seed=SEED + 1, n_draws=1)[0] == X[0])
    # the normals behind draw 0, recovered from the device's rows, against those of EM.sample's rows under the same seed
    n, dM = X.shape[1], X.shape[2]
    rows = np.arange(n, dtype=np.uint64)
    ours = ref.normals(SEED, rows, dM, 0)[0]
    theirs = sref.normals(SEED, rows, dM)[0]
    assert not np.any(ours == theirs)
    _, labels = on_device(ctx, key, seed=SEED, n_draws=1, labels=True)
    back = np.stack([np.linalg.solve(np.tril(G[k]), X[0][i] - mu_m[k] - A[k] @ (c["X_observed"][i] - mu_o[k])) for i, k in enumerate(labels[0])])
    assert np.max(np.abs(back - ours)) <= 1e-9 and np.min(np.abs(back - theirs)) > 1e-9


# ---- statistical checks -----------------------------------------------------------------------------------------------------------------

def test_moments_of_the_completed_rows(ctx):
    key = ref.MOMENTS_CASE
    c = ref.case(*key)
    X = on_device(ctx, key, n_draws=1, seed=1)[0]
    x_m = c["X"][:, cref.missing_of(key[1], key[3])]
    score = ref.moment_scores(c["X_observed"], x_m, X)
    print("CONDITION SAMPLE moments: %.2f standard errors" % score)
    assert score <= ref.STATISTICAL_BOUND


def test_the_mean_over_draws_is_the_conditional_mean(ctx):
    from ml_amd import _lib
    key = ref.DRAWS_CASE
    c, (mu_o, S_oo, A, mu_m, G) = conditioned(key)
    data = _lib.Data(ctx, c["X_observed"])
    y = data.em_conditional_means(c["mixing"], mu_o, S_oo, A, mu_m)
    X = data.em_conditional_samples(c["mixing"], mu_o, S_oo, A, mu_m, G, n_draws=ref.DRAWS, seed=2)
    data.close()
    score = ref.draw_mean_scores(X, y)
    print("CONDITION SAMPLE mean over %d draws: %.2f standard errors" % (ref.DRAWS, score))
    assert score <= ref.STATISTICAL_BOUND


# ---- the model surface ------------------------------------------------------------------------------------------------------------------

def _mousie():
    from conftest import load_golden
    return np.ascontiguousarray(load_golden("mousie_sklearn.npz")["X"])


def _fitted(covariance_type="full"):
    from ml_amd.cppyml import clustering
    em = clustering.EM(3)
    em.set_seed(5)
    if covariance_type != "full":
        em.set_covariance_type(covariance_type)
    em.fit(_mousie())
    return em


def _parameters(em):
    K = em.number_components
    return em.mixing_probabilities, np.ascontiguousarray(em.means.T), np.stack([np.ascontiguousarray(em.covariance(k)) for k in range(K)])


@pytest.mark.parametrize("covariance_type", ["full", "tied", "diag"])
def test_the_model_surface(ctx, covariance_type):
    from ml_amd import _lib
    X = _mousie()
    em = _fitted(covariance_type)
    before = (em.log_likelihood, np.array(em.labels), em.responsibilities_rows(0, 64), em.score_samples(X))
    X_o = np.ascontiguousarray(X[:, [0]])
    draws, labels = em.conditional_sample(X_o, [0], n_draws=3, seed=4, return_labels=True)
    dM = X.shape[1] - 1
    assert draws.shape == (3, len(X), dM) and draws.flags.c_contiguous and draws.dtype == np.float64
    assert labels.shape == (3, len(X)) and labels.dtype == np.uint32 and labels.max() < 3
    assert np.isfinite(draws).all()
    assert np.array_equal(em.conditional_sample(X_o, [0], n_draws=3, seed=4), draws)
    assert np.array_equal(em.conditional_sample(X_o, [0], seed=4)[0], draws[0])
    after = (em.log_likelihood, np.array(em.labels), em.responsibilities_rows(0, 64), em.score_samples(X))
    for a, b in zip(before, after):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    # the handle-level call on the fitted parameters, on an unweighted and on a weighted handle
    mixing, means, covs = _parameters(em)
    mu_o, S_oo, A, mu_m = _lib.em_condition(means, covs, [0])
    C_m, G = _lib.em_condition_covariances(covs, [0])
    assert np.array_equal(em.conditional_covariances([0]), C_m)
    if covariance_type == "diag":
        assert all(np.array_equal(C_m[k], np.diag(np.diag(covs[k])[1:])) for k in range(3))
    if covariance_type == "tied":
        assert all(np.array_equal(bits(G[k]), bits(G[0])) for k in range(3))
    data = _lib.Data(ctx, X_o)
    X_h, labels_h = data.em_conditional_samples(mixing, mu_o, S_oo, A, mu_m, G, n_draws=3, seed=4, labels=True)
    data.set_weights(np.random.default_rng(1).uniform(0.5, 2.0, len(X)))
    X_w = data.em_conditional_samples(mixing, mu_o, S_oo, A, mu_m, G, n_draws=3, seed=4)
    data.close()
    assert np.array_equal(bits(X_h), bits(draws)) and np.array_equal(labels_h, labels) and np.array_equal(bits(X_w), bits(draws))
    # no rows, no draws
    empty, empty_labels = em.conditional_sample(np.empty((0, 1)), [0], n_draws=2, return_labels=True)
    assert empty.shape == (2, 0, dM) and empty.dtype == np.float64 and empty_labels.shape == (2, 0)
    assert em.conditional_sample(X_o, [0], n_draws=0).shape == (0, len(X), dM)
    with pytest.raises(ValueError):
        em.conditional_sample(X, list(range(X.shape[1])))
    with pytest.raises(ValueError):
        em.conditional_sample(X_o, [0], n_draws=-1)
    with pytest.raises(TypeError):
        em.conditional_sample(X_o.astype(np.float32), [0])
