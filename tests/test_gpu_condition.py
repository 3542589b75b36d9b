"""mlhip_em_conditional_means and EM.conditional_mean on the device against the numpy restatement of the definition
(tests/condition_reference.py). Parameters go in directly through Data.em_conditional_means; the models come from the restatement's
generator (mu_k = 2.5 N(0, I), Sigma_k = A A^T / d + 0.5 I, pi ~ Dirichlet(4), rows drawn from the model).

Accuracy: err = max |y - y_ld| / max |y_ld| against the longdouble restatement, held to
    4 max(err_f64, FLOOR) + max_i sum_k |r_ik^E - r_ik^ld| |m_ik^ld| / max |y_ld|
with err_f64 the float64 restatement's own error, FLOOR = 8 * 2^-53 (tests/hp_limits.py) and r^E the responsibilities the existing
E-step kernels give for the marginal parameters on the same handle (mlhip_em_expectation + mlhip_em_responsibilities; held by
tests/test_gpu_hp_error.py): the new kernel is not charged with their error. One line per case is printed.

Bitwise: chunks, a prefix of a longer block, device groups, the skip switch, the plain tier against the register tier (the two tiers
evaluate in the same order, so their bits are required to be equal), and log_density against mlhip_em_score's composed route.
Definition checks that do not go through the restatement: K = 1, diagonal mode, the tower property. Then the model surface."""
import numpy as np
import pytest

import condition_reference as ref
from hp_limits import FLOOR

pytestmark = pytest.mark.gpu

SWITCHES = ("MLHIP_CONDITION", "MLHIP_CONDITION_ROWS", "MLHIP_CONDITION_SKIP", "MLHIP_SCORE", "MLHIP_SCORE_ROWS")


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
    """The case of ref.case(*key) with the library's own conditioning of its model (mlhip_em_condition; held by
    tests/test_condition_host.py) beside it; computed once."""
    from ml_amd import _lib
    if key not in _CONDITIONED:
        c = ref.case(*key)
        _CONDITIONED[key] = (c, _lib.em_condition(c["means"], c["covs"], c["observed"]))
    return _CONDITIONED[key]


def on_device(context, key, rows=None, log_density=False):
    from ml_amd import _lib
    c, (mu_o, S_oo, A, mu_m) = conditioned(key)
    X = c["X_observed"] if rows is None else np.ascontiguousarray(c["X_observed"][:rows])
    data = _lib.Data(context, X)
    out = data.em_conditional_means(c["mixing"], mu_o, S_oo, A, mu_m, log_density=log_density)
    data.close()
    return out


def check_accuracy(ctx, key, y, name):
    """The module docstring's rule; returns err / limit."""
    from ml_amd import _lib
    c, (mu_o, S_oo, _, _) = conditioned(key)
    n, K = c["X_observed"].shape[0], len(c["mixing"])
    data = _lib.Data(ctx, c["X_observed"])
    data.em_expectation(c["mixing"], mu_o, S_oo)
    r_estep = data.em_responsibilities(K)
    data.close()
    ld = c["ld"]
    assert y.shape == ld["y"].shape and y.flags.c_contiguous and y.dtype == np.float64
    err, err_f64 = ref.error(y, ld["y"]), ref.error(c["f64"]["y"], ld["y"])
    lim = ref.limit(err_f64, FLOOR, r_estep, ld)
    print("CONDITION %s n %d K %d: err %.2e, float64 restatement %.2e, limit %.2e, ratio %.3f" % (name, n, K, err, err_f64, lim, err / lim))
    assert err <= lim, (name, err, lim)
    return err / lim


def route_of(ctx, key):
    from ml_amd import _lib
    c, (_, _, A, _) = conditioned(key)
    data = _lib.Data(ctx, c["X_observed"][:1])
    route = data.em_condition_route(len(c["mixing"]), A.shape[1])
    data.close()
    return route


def expected_route(dO, dM):
    return "registers" if dO <= 32 and dM <= 32 else "plain"


def first(n):
    return tuple(range(n))


# (seed, d, K, observed, n): the smallest shapes at which the kernel can go wrong
N = 321                                                          # five tiles of 64 rows and a ragged one
# a wave takes a second tile above grid x waves x 64 rows: the register kernel's grid is at most 4 workgroups per CU of 4 waves at
# dM <= 16 -- 262 144 rows on 256 CUs
SECOND_TILE = 256 * 4 * 4 * 64 + 65
SHAPES = ([(1, 3, 2, (2, 0), n) for n in (1, 63, 64, 65, 257)] +
          [(2, 8, K, (6, 1, 3, 4), N) for K in (1, 16, 17, 64, 65)] +
          [(3, dO + 3, 3, first(dO), N) for dO in (1, 5, 12, 31, 32, 33)] +
          [(4, 4 + dM, 3, (3, 0, 2, 1), N) for dM in (1, 7, 32, 33)] +
          [(5, 64, K, first(32), N) for K in (24, 40, 64)] +
          [(6, 130, 3, tuple(int(c) for c in np.random.default_rng(130).permutation(130)[:70]), N)] +
          [(7, 7, 2, (5, 0, 2, 6), SECOND_TILE)])


def shape_id(s):
    return "d%d-K%d-dO%d-n%d" % (s[1], s[2], len(s[3]), s[4])


@pytest.mark.parametrize("key", SHAPES, ids=shape_id)
def test_against_the_restatement(ctx, key):
    _, d, K, observed, n = key
    dO, dM = len(observed), d - len(observed)
    assert route_of(ctx, key) == expected_route(dO, dM)
    ctx.timing_enable(True)
    ctx.timing_reset()
    y, dens = on_device(ctx, key, log_density=True)
    launches = ctx.timing_get("em_condition")[1]
    ctx.timing_enable(False)
    assert launches == 1
    check_accuracy(ctx, key, y, shape_id(key))
    ld = conditioned(key)[0]["ld"]["log_density"]
    assert np.max(np.abs(dens.astype(np.longdouble) - ld)) <= 1e-12 * max(1.0, float(np.abs(ld).max()))


# ---- bitwise invariants -------------------------------------------------------------------------------------------------------------

CHUNKED = [(8, 3, 2, (2, 0), 1100), (8, 14, 5, (9, 0, 4, 13, 2, 7), 1100), (8, 36, 3, first(33), 700)]


@pytest.mark.parametrize("key", CHUNKED, ids=shape_id)
@pytest.mark.parametrize("rows", ["64", "192", "512"])
def test_chunk_rows_give_the_bits_of_one_chunk(ctx, monkeypatch, key, rows):
    """(the chunk is whole 256-row tiles: 64 and 192 both run 256 rows at a time, 512 two tiles)"""
    y, dens = on_device(ctx, key, log_density=True)
    monkeypatch.setenv("MLHIP_CONDITION_ROWS", rows)
    ctx.timing_enable(True)
    ctx.timing_reset()
    y_c, dens_c = on_device(ctx, key, log_density=True)
    launches = ctx.timing_get("em_condition")[1]
    ctx.timing_enable(False)
    chunk = -(-int(rows) // 256) * 256
    assert launches == -(-key[4] // chunk) and launches > 1
    assert np.array_equal(y_c.view(np.uint64), y.view(np.uint64)) and np.array_equal(dens_c.view(np.uint64), dens.view(np.uint64))


@pytest.mark.parametrize("key", CHUNKED, ids=shape_id)
def test_a_prefix_of_a_longer_block_gives_the_bits_of_the_short_block(ctx, key):
    y = on_device(ctx, key)
    for n in (1, 63, 300, 513):
        assert np.array_equal(on_device(ctx, key, rows=n).view(np.uint64), y[:n].view(np.uint64)), n


@pytest.mark.parametrize("shards", [2, 3])
@pytest.mark.parametrize("key", CHUNKED, ids=shape_id)
def test_a_device_group_gives_the_single_context_bits(ctx, key, shards):
    from ml_amd import _lib
    y, dens = on_device(ctx, key, log_density=True)
    group = _lib.Context.group(shards, device_ids=[0] * shards)
    try:
        y_g, dens_g = on_device(group, key, log_density=True)
    finally:
        group.close()
    assert np.array_equal(y_g.view(np.uint64), y.view(np.uint64)) and np.array_equal(dens_g.view(np.uint64), dens.view(np.uint64))


def separated(K=64, d=8, observed=(6, 1, 3, 4), per_component=40):
    """A mixture whose components are some 80 standard deviations apart, rows in the order of their components: most responsibilities
    underflow to exactly 0, and whole waves have no share in most components."""
    mixing, means, covs = ref.model(21, d, K)
    means = 30.0 * means
    rng = np.random.default_rng(22)
    L = np.linalg.cholesky(covs)
    labels = np.repeat(np.arange(K), per_component)
    X = means[labels] + np.einsum("nij,nj->ni", L[labels], rng.standard_normal((len(labels), d)))
    return mixing, means, covs, np.ascontiguousarray(X[:, list(observed)]), list(observed)


@pytest.mark.parametrize("tier", ["registers", "plain"])
def test_the_skip_changes_no_bit(ctx, monkeypatch, tier):
    from ml_amd import _lib
    mixing, means, covs, X_o, observed = separated()
    K = len(mixing)
    mu_o, S_oo, A, mu_m = _lib.em_condition(means, covs, observed)
    data = _lib.Data(ctx, X_o)
    data.em_expectation(mixing, mu_o, S_oo)
    R = data.em_responsibilities(K)
    assert np.count_nonzero(R == 0) >= R.size // 2, np.count_nonzero(R == 0) / R.size
    if tier == "plain":
        monkeypatch.setenv("MLHIP_CONDITION", "plain")
    assert data.em_condition_route(K, A.shape[1]) == tier
    y = data.em_conditional_means(mixing, mu_o, S_oo, A, mu_m)
    monkeypatch.setenv("MLHIP_CONDITION_SKIP", "0")
    y_all = data.em_conditional_means(mixing, mu_o, S_oo, A, mu_m)
    data.close()
    assert np.array_equal(y.view(np.uint64), y_all.view(np.uint64))
    # every row sits in its own component: the result is that component's prediction
    want = np.stack([mu_m[k] + (X_o[i] - mu_o[k]) @ A[k].T for i, k in enumerate(np.argmax(R, axis=1))])
    assert np.max(np.abs(y - want)) <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("key", [SHAPES[6], SHAPES[8], SHAPES[13], SHAPES[17], SHAPES[20]], ids=shape_id)
def test_the_plain_tier_gives_the_bits_of_the_register_tier(ctx, monkeypatch, key):
    """Both tiers evaluate the file header's order, so more than the accuracy rule is asked: equal bits."""
    assert route_of(ctx, key) == "registers"
    y = on_device(ctx, key)
    monkeypatch.setenv("MLHIP_CONDITION", "plain")
    assert route_of(ctx, key) == "plain"
    y_p = on_device(ctx, key)
    check_accuracy(ctx, key, y_p, "plain " + shape_id(key))
    assert np.array_equal(y_p.view(np.uint64), y.view(np.uint64))


@pytest.mark.parametrize("key", [SHAPES[4], SHAPES[8], SHAPES[12], SHAPES[20], SHAPES[22]], ids=shape_id)
def test_log_density_has_the_bits_of_the_composed_score(ctx, monkeypatch, key):
    from ml_amd import _lib
    c, (mu_o, S_oo, _, _) = conditioned(key)
    _, dens = on_device(ctx, key, log_density=True)
    monkeypatch.setenv("MLHIP_SCORE", "composed")
    data = _lib.Data(ctx, c["X_observed"])
    assert data.em_score_route(len(c["mixing"])) == "composed"
    want, _ = data.em_score(c["mixing"], mu_o, S_oo, labels=False)
    data.close()
    assert np.array_equal(dens.view(np.uint64), want.view(np.uint64))


# ---- definition checks that do not go through the restatement -------------------------------------------------------------------------

@pytest.mark.parametrize("d,observed", [(3, (2, 0)), (9, (7, 2, 3, 0)), (40, first(34))])
def test_one_component_is_the_affine_map_exactly(ctx, d, observed):
    """K = 1: r = exp(lw - lse) = exp(0) = 1 exactly, so y_j = fma(1, t_j, +0.0) = t_j: the header's fma chain over the library's own
    conditioning, checked in longdouble within one float64 rounding per step of the chain (dO of them) and three more for the start,
    r and the last fma."""
    from ml_amd import _lib
    mixing, means, covs = ref.model(31, d, 1)
    X_o = np.ascontiguousarray(ref.rows(mixing, means, covs, 200, 32)[:, list(observed)])
    mu_o, S_oo, A, mu_m = _lib.em_condition(means, covs, list(observed))
    data = _lib.Data(ctx, X_o)
    y = data.em_conditional_means(mixing, mu_o, S_oo, A, mu_m)
    data.close()
    LD = np.longdouble
    z = (X_o - mu_o[0]).astype(LD)                               # (the float64 subtraction, as the kernel does it first)
    terms = z[:, None, :] * A[0].astype(LD)[None, :, :]
    want = mu_m[0].astype(LD) + terms.sum(axis=2)
    slack = (np.abs(mu_m[0]) + np.abs(terms).sum(axis=2)) * (len(observed) + 3) * 2.0 ** -53
    assert np.all(np.abs(y.astype(LD) - want) <= slack)


def test_diagonal_mode_is_the_responsibilities_times_the_missing_means(ctx):
    from ml_amd import _lib
    rng = np.random.default_rng(41)
    K, d, observed = 6, 9, [7, 2, 3, 0]
    means, variances = 2.5 * rng.standard_normal((K, d)), rng.uniform(0.5, 2.0, (K, d))
    mixing = rng.dirichlet(np.full(K, 4.0))
    labels = rng.choice(K, size=N, p=mixing)
    X_o = np.ascontiguousarray((means[labels] + np.sqrt(variances[labels]) * rng.standard_normal((N, d)))[:, observed])
    mu_o, S_oo, A, mu_m = _lib.em_condition(means, variances, observed, diagonal=True)
    assert not A.any()
    data = _lib.Data(ctx, X_o)
    y = data.em_conditional_means(mixing, mu_o, S_oo, A, mu_m)
    data.em_expectation(mixing, mu_o, S_oo)
    R = data.em_responsibilities(K)
    data.close()
    LD = np.longdouble
    want = R.astype(LD) @ mu_m.astype(LD)
    # the accuracy rule with the E-step's own responsibilities on both sides: what is left is the K-term fma chain
    err = float(np.abs(y.astype(LD) - want).max() / np.abs(want).max())
    err_f64 = float(np.abs((R @ mu_m).astype(LD) - want).max() / np.abs(want).max())
    print("CONDITION diagonal: err %.2e, float64 product %.2e" % (err, err_f64))
    assert err <= 4 * max(err_f64, FLOOR)


def test_tower_property(ctx):
    """E[E[x_M | x_O]] = E[x_M]: over n = 200 000 rows drawn from the model, the mean of the output lies within 5 standard errors of the
    sample mean of x_M (its own: the rows' standard deviation over sqrt(n))."""
    key = (11, 6, 4, (4, 0, 1), 200000, 12)
    c = ref.case(*key)
    y = on_device(ctx, key)
    x_m = c["X"][:, ref.missing_of(6, key[3])]
    for name, values in (("device", y), ("float64 restatement", c["f64"]["y"])):
        z = np.abs(values.mean(axis=0) - x_m.mean(axis=0)) / (x_m.std(axis=0, ddof=1) / np.sqrt(len(x_m)))
        print("CONDITION tower %s: %s standard errors" % (name, np.round(z, 2)))
        assert np.all(z <= 5), (name, z)


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


def test_the_model_surface(ctx):
    from ml_amd import _lib
    X = _mousie()
    em = _fitted()
    before = (em.log_likelihood, np.array(em.labels), em.responsibilities_rows(0, 64), em.score_samples(X))
    X_o = np.ascontiguousarray(X[:, [0]])
    y, dens = em.conditional_mean(X_o, [0], return_log_density=True)
    assert y.shape == (len(X), X.shape[1] - 1) and y.flags.c_contiguous and y.dtype == np.float64 and dens.shape == (len(X),)
    assert np.array_equal(em.conditional_mean(X_o, [0]), y)
    after = (em.log_likelihood, np.array(em.labels), em.responsibilities_rows(0, 64), em.score_samples(X))
    for a, b in zip(before, after):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    # the handle-level call on the fitted parameters, on an unweighted and on a weighted handle
    mixing, means, covs = _parameters(em)
    mu_o, S_oo, A, mu_m = _lib.em_condition(means, covs, [0])
    data = _lib.Data(ctx, X_o)
    y_h, dens_h = data.em_conditional_means(mixing, mu_o, S_oo, A, mu_m, log_density=True)
    data.set_weights(np.random.default_rng(1).uniform(0.5, 2.0, len(X)))
    y_w, dens_w = data.em_conditional_means(mixing, mu_o, S_oo, A, mu_m, log_density=True)
    data.close()
    assert np.array_equal(y_h.view(np.uint64), y.view(np.uint64)) and np.array_equal(dens_h.view(np.uint64), dens.view(np.uint64))
    assert np.array_equal(y_w.view(np.uint64), y.view(np.uint64)) and np.array_equal(dens_w.view(np.uint64), dens.view(np.uint64))
    # a regression of the last coordinates on the first explains some of their variance
    assert np.mean((y - X[:, 1:]) ** 2) < np.var(X[:, 1:], axis=0).sum()
    # the other column, and no rows
    y1 = em.conditional_mean(np.ascontiguousarray(X[:, [1]]), [1])
    assert y1.shape == (len(X), 1) and np.isfinite(y1).all()
    empty, empty_dens = em.conditional_mean(np.empty((0, 1)), [0], return_log_density=True)
    assert empty.shape == (0, X.shape[1] - 1) and empty.dtype == np.float64 and empty_dens.shape == (0,)
    with pytest.raises(ValueError):
        em.conditional_mean(X, list(range(X.shape[1])))
    with pytest.raises(TypeError):
        em.conditional_mean(X_o.astype(np.float32), [0])


@pytest.mark.parametrize("covariance_type", ["tied", "diag"])
def test_tied_and_diagonal_fits_condition(ctx, covariance_type):
    from ml_amd import _lib
    X = _mousie()
    em = _fitted(covariance_type)
    X_o = np.ascontiguousarray(X[:, [0]])
    y = em.conditional_mean(X_o, [0])
    assert y.shape == (len(X), X.shape[1] - 1) and np.isfinite(y).all()
    mixing, means, covs = _parameters(em)
    mu_o, S_oo, A, mu_m = _lib.em_condition(means, covs, [0])
    if covariance_type == "diag":
        assert not A.any()
    else:
        assert all(np.array_equal(A[k], A[0]) for k in range(len(A)))
    data = _lib.Data(ctx, X_o)
    y_h = data.em_conditional_means(mixing, mu_o, S_oo, A, mu_m)
    data.close()
    assert np.array_equal(y_h.view(np.uint64), y.view(np.uint64))
