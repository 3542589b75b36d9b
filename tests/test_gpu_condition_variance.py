"""mlhip_em_conditional_variances and EM.conditional_variance on the device against the numpy restatement of the definition
(tests/condition_variance_reference.py). Parameters go in directly through _lib.em_conditional_variances; models and rows come from
tests/condition_reference.py's generator.

Accuracy, per form: err = max |v - v_ld| / max |v_ld| against the longdouble restatement, held to
    4 max(err_f64, FLOOR) + max_{i,a,b} sum_k |r_ik^E - r_ik^ld| |C_k,ab^ld + u_ika^ld u_ikb^ld| / max |v_ld|
with err_f64 the float64 restatement's own error, FLOOR = 8 * 2^-53 (tests/hp_limits.py) and r^E the responsibilities the existing
E-step kernels give for the marginal parameters on the same handle: the new kernel is not charged with their error, and no term comes
from the code under test. One line per case and form is printed. Every run also asserts what the definition's order implies: the mean
and the log-density have the bits of Data.em_conditional_means, the diagonal of the full form has the bits of the diagonal form, the
full form is exactly symmetric, no variance is negative, and one launch of the new kernel per chunk.

Bitwise: chunks, a prefix of a longer block, device groups, the skip switch on both tiers, the plain tier against the register tier.
Definition checks that do not go through the restatement: K = 1, a diagonal model, a row of NaN, the second moment of
conditional_sample's draws. Then the model surface and the handle's state."""
import numpy as np
import pytest

import condition_reference as cref
import condition_variance_reference as ref
from hp_limits import FLOOR

pytestmark = pytest.mark.gpu

SWITCHES = ("MLHIP_CONDITION", "MLHIP_CONDITION_ROWS", "MLHIP_CONDITION_SKIP", "MLHIP_SCORE", "MLHIP_SCORE_ROWS")
LD = np.longdouble


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


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def first(n):
    return tuple(range(n))


_CONDITIONED = {}


def conditioned(key):
    """ref.case(*key) with the library's own conditioning of its model beside it (mlhip_em_condition, mlhip_em_condition_covariances;
    held by tests/test_condition_host.py and tests/test_condition_sample_host.py): (case, (mu_o, S_oo, A, mu_m, C)); computed once."""
    from ml_amd import _lib
    if key not in _CONDITIONED:
        c = ref.case(*key)
        C_m, _ = _lib.em_condition_covariances(c["covs"], c["observed"])
        _CONDITIONED[key] = (c, _lib.em_condition(c["means"], c["covs"], c["observed"]) + (C_m,))
    return _CONDITIONED[key]


def run(context, X, mixing, parameters, expect_launches=None):
    """Both forms with the mean and the log-density on, on one handle, beside Data.em_conditional_means on the same handle -> dict. Asserts
    what every run must show (module docstring)."""
    from ml_amd import _lib
    mu_o, S_oo, A, mu_m, C_m = parameters
    data = _lib.Data(context, X)
    out = {}
    timed = expect_launches is not None
    try:
        if timed:
            context.timing_enable(True)
        for form, full in (("diag", False), ("full", True)):
            if timed:
                context.timing_reset()
            v, y, dens = _lib.em_conditional_variances(data, mixing, mu_o, S_oo, A, mu_m, C_m, full=full, means=True, log_density=True)
            out[form], out[form + "_y"], out[form + "_dens"] = v, y, dens
            if timed:
                out[form + "_launches"] = context.timing_get("em_condition_variance")[1]
        if timed:
            context.timing_enable(False)
        out["y"], out["dens"] = data.em_conditional_means(mixing, mu_o, S_oo, A, mu_m, log_density=True)
        out["alone"] = _lib.em_conditional_variances(data, mixing, mu_o, S_oo, A, mu_m, C_m)
    finally:
        if timed:
            context.timing_enable(False)
        data.close()
    n, dM = X.shape[0], mu_m.shape[1]
    assert out["diag"].shape == (n, dM) and out["full"].shape == (n, dM, dM)
    for form in ("diag", "full"):
        assert out[form].flags.c_contiguous and out[form].dtype == np.float64
        assert np.array_equal(bits(out[form + "_y"]), bits(out["y"])), form
        assert np.array_equal(bits(out[form + "_dens"]), bits(out["dens"])), form
        if timed:
            assert out[form + "_launches"] == expect_launches, (form, out[form + "_launches"])
    assert np.array_equal(bits(out["alone"]), bits(out["diag"]))                       # (asking for the mean changes no bit)
    assert np.array_equal(bits(np.diagonal(out["full"], axis1=1, axis2=2)), bits(out["diag"]))
    assert np.array_equal(bits(out["full"]), bits(np.swapaxes(out["full"], 1, 2)))
    ok = ~np.isnan(out["diag"])
    assert (out["diag"][ok] >= 0).all()
    return out


def on_device(context, key, rows=None, expect_launches=None):
    c, parameters = conditioned(key)
    X = c["X_observed"] if rows is None else np.ascontiguousarray(c["X_observed"][:rows])
    return run(context, X, c["mixing"], parameters, expect_launches)


def check_accuracy(ctx, key, out, name):
    """The module docstring's rule for both forms; returns the worse err / limit."""
    from ml_amd import _lib
    c, (mu_o, S_oo, _, _, _) = conditioned(key)
    n, K = c["X_observed"].shape[0], len(c["mixing"])
    data = _lib.Data(ctx, c["X_observed"])
    data.em_expectation(c["mixing"], mu_o, S_oo)
    r_estep = data.em_responsibilities(K)
    data.close()
    worst = 0.0
    for form in ("diag", "full"):
        v_ld = c["vld"][form]
        err, err_f64 = ref.error(out[form], v_ld), ref.error(c["v64"][form], v_ld)
        lim = ref.limit(err_f64, FLOOR, r_estep, c, form)
        print("VARIANCE %s %s n %d K %d: err %.2e, float64 restatement %.2e, limit %.2e, ratio %.3f" %
              (name, form, n, K, err, err_f64, lim, err / lim))
        assert err <= lim, (name, form, err, lim)
        worst = max(worst, err / lim)
    return worst


def route_of(ctx, key, full):
    from ml_amd import _lib
    c, parameters = conditioned(key)
    data = _lib.Data(ctx, c["X_observed"][:1])
    route = _lib.em_condition_variance_route(data, len(c["mixing"]), parameters[3].shape[1], full)
    data.close()
    return route


_BOUND = []


def full_bound(ctx):
    """The largest dM the full form's register tier serves, read from the route function at dO = 4 (nothing is launched)."""
    from ml_amd import _lib
    if not _BOUND:
        data = _lib.Data(ctx, np.zeros((1, 4)))
        routes = [_lib.em_condition_variance_route(data, 3, dM, True) for dM in range(1, 34)]
        data.close()
        _BOUND.append(max(dM for dM, route in zip(range(1, 34), routes) if route == "registers"))
    return _BOUND[0]


def expected_route(ctx, dO, dM, full):
    return "registers" if dO <= 32 and dM <= (full_bound(ctx) if full else 32) else "plain"


# (seed, d, K, observed, n): the smallest shapes at which the kernel can go wrong
N = 321                                                          # five tiles of 64 rows and a ragged one
# a wave takes a second tile above grid x waves x 64 rows: the register kernels' grid is at most 4 workgroups per CU, of 4 waves in
# the diagonal form at dM <= 16 (and in the full form at dM <= 4: this case has dM = 3) -- 256 CUs x 4 x 4 x 64 = 262 144 rows
SECOND_TILE = 256 * 4 * 4 * 64 + 65
SHAPES = ([(1, 3, 2, (2, 0), n) for n in (1, 63, 64, 65, 257)] +
          [(2, 8, K, (6, 1, 3, 4), N) for K in (1, 16, 17, 64, 65)] +
          [(3, dO + 3, 3, first(dO), N) for dO in (1, 5, 12, 31, 32, 33)] +
          [(4, 4 + dM, 3, (3, 0, 2, 1), N) for dM in (1, 7, 8, 32, 33)] +
          [(5, 64, 40, first(32), N)] +
          [(6, 130, 3, tuple(int(c) for c in np.random.default_rng(130).permutation(130)[:70]), N)] +
          [(7, 7, 2, (5, 0, 2, 6), SECOND_TILE)])
# the cases whose largest variance comes mostly from the spread of the component predictions (the u u^T path): asserted below
BETWEEN = [SHAPES[7], SHAPES[9], SHAPES[10], SHAPES[19], SHAPES[20]]


def shape_id(s):
    return "d%d-K%d-dO%d-n%d" % (s[1], s[2], len(s[3]), s[4])


def accuracy_case(ctx, key):
    _, d, K, observed, n = key
    dO, dM = len(observed), d - len(observed)
    for full in (False, True):
        assert route_of(ctx, key, full) == expected_route(ctx, dO, dM, full), full
    out = on_device(ctx, key, expect_launches=1)
    return check_accuracy(ctx, key, out, shape_id(key))


@pytest.mark.parametrize("key", SHAPES, ids=shape_id)
def test_against_the_restatement(ctx, key):
    accuracy_case(ctx, key)
    if key in BETWEEN:
        share = ref.between_share(conditioned(key)[0])
        print("VARIANCE %s: between-component share of the largest variance %.2f" % (shape_id(key), share))
        assert share > 0.5


@pytest.mark.parametrize("offset", [0, 1])
def test_against_the_restatement_at_the_full_forms_register_bound(ctx, offset):
    """dM = B and B + 1, B read from the route function: the last shape of the full form's register tier and the first of its plain one."""
    dM = full_bound(ctx) + offset
    key = (4, 4 + dM, 3, (3, 0, 2, 1), N)
    assert route_of(ctx, key, True) == ("plain" if offset else "registers")
    accuracy_case(ctx, key)


def test_the_route_function(ctx):
    from ml_amd import _lib
    data = _lib.Data(ctx, np.zeros((1, 4)))
    diag = [_lib.em_condition_variance_route(data, 3, dM, False) for dM in range(1, 34)]
    full = [_lib.em_condition_variance_route(data, 3, dM, True) for dM in range(1, 34)]
    data.close()
    assert diag == ["registers"] * 32 + ["plain"]
    B = full_bound(ctx)
    assert 8 <= B <= 32
    assert full == ["registers"] * B + ["plain"] * (33 - B)      # monotone
    wide = _lib.Data(ctx, np.zeros((1, 33)))
    assert _lib.em_condition_variance_route(wide, 3, 1, False) == "plain" and _lib.em_condition_variance_route(wide, 3, 1, True) == "plain"
    wide.close()


# ---- bitwise invariants -------------------------------------------------------------------------------------------------------------

CHUNKED = [(8, 3, 2, (2, 0), 1100), (8, 14, 5, (9, 0, 4, 13, 2, 7), 1100), (8, 36, 3, first(33), 700)]
FORMS = ("diag", "full", "y", "dens")


def same_bits(a, b):
    return all(np.array_equal(bits(a[f]), bits(b[f])) for f in FORMS)


@pytest.mark.parametrize("key", CHUNKED, ids=shape_id)
@pytest.mark.parametrize("rows", ["256", "512"])
def test_chunk_rows_give_the_bits_of_one_chunk(ctx, monkeypatch, key, rows):
    one = on_device(ctx, key, expect_launches=1)
    monkeypatch.setenv("MLHIP_CONDITION_ROWS", rows)
    chunks = -(-key[4] // int(rows))
    assert chunks > 1
    assert same_bits(on_device(ctx, key, expect_launches=chunks), one)


@pytest.mark.parametrize("key", CHUNKED, ids=shape_id)
def test_a_prefix_of_a_longer_block_gives_the_bits_of_the_short_block(ctx, key):
    whole = on_device(ctx, key)
    for n in (1, 63, 300, 513):
        part = on_device(ctx, key, rows=n)
        assert all(np.array_equal(bits(part[f]), bits(whole[f][:n])) for f in FORMS), n


@pytest.mark.parametrize("shards", [2, 3])
@pytest.mark.parametrize("key", CHUNKED, ids=shape_id)
def test_a_device_group_gives_the_single_context_bits(ctx, key, shards):
    from ml_amd import _lib
    single = on_device(ctx, key)
    group = _lib.Context.group(shards, device_ids=[0] * shards)
    try:
        grouped = on_device(group, key)
    finally:
        group.close()
    assert same_bits(grouped, single)


def separated(K=64, d=8, observed=(6, 1, 3, 4), per_component=40):
    """A mixture whose components are some 80 standard deviations apart, rows in the order of their components: most responsibilities
    underflow to exactly 0, and whole waves have no share in most components (the generator of tests/test_gpu_condition.py)."""
    mixing, means, covs = cref.model(21, d, K)
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
    parameters = _lib.em_condition(means, covs, observed) + (_lib.em_condition_covariances(covs, observed)[0],)
    data = _lib.Data(ctx, X_o)
    data.em_expectation(mixing, parameters[0], parameters[1])
    R = data.em_responsibilities(K)
    assert np.count_nonzero(R == 0) >= R.size // 2, np.count_nonzero(R == 0) / R.size
    if tier == "plain":
        monkeypatch.setenv("MLHIP_CONDITION", "plain")
    for full in (False, True):
        assert _lib.em_condition_variance_route(data, K, parameters[3].shape[1], full) == tier
    data.close()
    skipped = run(ctx, X_o, mixing, parameters, expect_launches=1)
    monkeypatch.setenv("MLHIP_CONDITION_SKIP", "0")
    assert same_bits(run(ctx, X_o, mixing, parameters, expect_launches=1), skipped)
    # every row sits in its own component: the result is that component's conditioned covariance
    want = parameters[4][np.argmax(R, axis=1)]
    assert np.max(np.abs(skipped["full"] - want)) <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("key", [SHAPES[6], SHAPES[8], SHAPES[13], SHAPES[17], SHAPES[19]], ids=shape_id)
def test_the_plain_tier_gives_the_bits_of_the_register_tier(ctx, monkeypatch, key):
    """Both tiers evaluate the header's order, so more than the accuracy rule is asked: equal bits."""
    assert route_of(ctx, key, False) == "registers"
    registers = on_device(ctx, key, expect_launches=1)
    monkeypatch.setenv("MLHIP_CONDITION", "plain")
    assert route_of(ctx, key, False) == "plain" and route_of(ctx, key, True) == "plain"
    plain = on_device(ctx, key, expect_launches=1)
    check_accuracy(ctx, key, plain, "plain " + shape_id(key))
    assert same_bits(plain, registers)


# ---- definition checks that do not go through the restatement -------------------------------------------------------------------------

@pytest.mark.parametrize("d,observed", [(3, (2, 0)), (9, (7, 2, 3, 0)), (40, first(34))])
def test_one_component_gives_its_conditioned_covariance_bit_for_bit(ctx, d, observed):
    """K = 1: r = exp(lw - lse) = exp(0) = 1 exactly (asserted first), so y = t, u = t - y = +0.0, s = fma(0, 0, C) = C and
    v = fma(1, C, +0.0) = C: every row returns C_1's bits, in both forms."""
    from ml_amd import _lib
    mixing, means, covs = cref.model(31, d, 1)
    X_o = np.ascontiguousarray(cref.rows(mixing, means, covs, 200, 32)[:, list(observed)])
    parameters = _lib.em_condition(means, covs, list(observed)) + (_lib.em_condition_covariances(covs, list(observed))[0],)
    data = _lib.Data(ctx, X_o)
    data.em_expectation(mixing, parameters[0], parameters[1])
    assert (data.em_responsibilities(1) == 1.0).all()
    data.close()
    out = run(ctx, X_o, mixing, parameters, expect_launches=1)
    C1 = parameters[4][0]
    assert np.array_equal(bits(out["full"]), bits(np.broadcast_to(C1, out["full"].shape)))
    assert np.array_equal(bits(out["diag"]), bits(np.broadcast_to(np.diag(C1), out["diag"].shape)))


def test_a_diagonal_model_is_the_mixture_of_its_variances_and_the_spread_of_its_means(ctx):
    """sum_k r_k (sigma^2_k,j + (mu_k,j - y_j)^2) from the E-step's own responsibilities, in longdouble; what is left is the K-term fma
    chain, held to 4 max(err_f64, FLOOR) with err_f64 the float64 evaluation's own error."""
    from ml_amd import _lib
    rng = np.random.default_rng(41)
    K, d, observed = 6, 9, [7, 2, 3, 0]
    M = cref.missing_of(d, observed)
    means, variances = 2.5 * rng.standard_normal((K, d)), rng.uniform(0.5, 2.0, (K, d))
    mixing = rng.dirichlet(np.full(K, 4.0))
    labels = rng.choice(K, size=N, p=mixing)
    X_o = np.ascontiguousarray((means[labels] + np.sqrt(variances[labels]) * rng.standard_normal((N, d)))[:, observed])
    parameters = _lib.em_condition(means, variances, observed, diagonal=True) + (
        _lib.em_condition_covariances(variances, observed, diagonal=True)[0],)
    assert not parameters[2].any()
    assert np.array_equal(parameters[4], np.stack([np.diag(v[M]) for v in variances]))
    out = run(ctx, X_o, mixing, parameters, expect_launches=1)
    data = _lib.Data(ctx, X_o)
    data.em_expectation(mixing, parameters[0], parameters[1])
    R = data.em_responsibilities(K)
    data.close()

    def evaluate(dtype):
        r, mu, s2 = R.astype(dtype), means[:, M].astype(dtype), variances[:, M].astype(dtype)
        y = r @ mu
        return (r[:, :, None] * (s2[None] + (mu[None] - y[:, None, :]) ** 2)).sum(axis=1)

    want = evaluate(LD)
    err = float(np.abs(out["diag"].astype(LD) - want).max() / np.abs(want).max())
    err_f64 = float(np.abs(evaluate(np.float64).astype(LD) - want).max() / np.abs(want).max())
    print("VARIANCE diagonal model: err %.2e, float64 evaluation %.2e" % (err, err_f64))
    assert err <= 4 * max(err_f64, FLOOR)
    off = out["full"].copy()
    off[:, np.arange(len(M)), np.arange(len(M))] = 0
    between = ((R[:, :, None, None] * (means[:, M][None, :, :, None] - out["y"][:, None, :, None])
                * (means[:, M][None, :, None, :] - out["y"][:, None, None, :])).sum(axis=1))
    between[:, np.arange(len(M)), np.arange(len(M))] = 0
    assert np.max(np.abs(off - between)) <= 1e-12 * np.abs(want).max()


def test_a_row_of_nan_gives_nan_and_leaves_its_neighbours_alone(ctx):
    key = (2, 8, 17, (6, 1, 3, 4), N)
    c, parameters = conditioned(key)
    clean = on_device(ctx, key)
    X = c["X_observed"].copy()
    X[70] = np.nan
    out = run(ctx, X, c["mixing"], parameters, expect_launches=1)
    others = np.arange(N) != 70
    for f in FORMS:
        assert np.isnan(out[f][70]).all(), f
        assert np.array_equal(bits(out[f][others]), bits(clean[f][others])), f


def test_the_second_moment_of_conditional_samples_draws(ctx):
    """For every (row, coordinate) the mean over 4096 draws of (x - y)^2 lies within 6 standard errors of v, the standard error from the
    draws themselves (sample std / sqrt(4096)): 192 comparisons. 6 holds a wrong formula out; it is not a measurement."""
    from ml_amd import _lib
    key = (9, 5, 3, (4, 1), 64)
    c, parameters = conditioned(key)
    mu_o, S_oo, A, mu_m, _ = parameters
    _, G = _lib.em_condition_covariances(c["covs"], c["observed"])
    out = on_device(ctx, key, expect_launches=1)
    draws = 4096
    data = _lib.Data(ctx, c["X_observed"])
    X = data.em_conditional_samples(c["mixing"], mu_o, S_oo, A, mu_m, G, n_draws=draws, seed=20261020)
    data.close()
    q = (X - out["y"][None]) ** 2
    se = q.std(axis=0, ddof=1) / np.sqrt(draws)
    z = np.abs(q.mean(axis=0) - out["diag"]) / se
    assert z.shape == (64, 3)
    print("VARIANCE against %d draws: worst %.2f standard errors" % (draws, z.max()))
    assert (z <= 6).all(), z.max()


# ---- the model surface ------------------------------------------------------------------------------------------------------------------

def _mousie():
    from conftest import load_golden
    return np.ascontiguousarray(load_golden("mousie_sklearn.npz")["X"])


def _fitted(covariance_type):
    from ml_amd.cppyml import clustering
    em = clustering.EM(3)
    em.set_seed(5)
    if covariance_type != "full":
        em.set_covariance_type(covariance_type)
    em.fit(_mousie())
    return em


@pytest.mark.parametrize("covariance_type", ["full", "diag", "tied"])
def test_the_model_surface(ctx, covariance_type):
    from ml_amd import _lib
    X = _mousie()
    em = _fitted(covariance_type)
    dM = X.shape[1] - 1
    X_o = np.ascontiguousarray(X[:, [0]])
    v = em.conditional_variance(X_o, [0])
    assert v.shape == (len(X), dM) and v.flags.c_contiguous and v.dtype == np.float64 and (v > 0).all()
    v2, y = em.conditional_variance(X_o, [0], return_mean=True)
    assert np.array_equal(bits(v2), bits(v)) and y.shape == (len(X), dM) and y.flags.c_contiguous
    assert np.array_equal(bits(y), bits(em.conditional_mean(X_o, [0])))
    V, y2 = em.conditional_variance(X_o, [0], covariance=True, return_mean=True)
    assert V.shape == (len(X), dM, dM) and V.flags.c_contiguous and np.array_equal(bits(y2), bits(y))
    assert np.array_equal(bits(np.diagonal(V, axis1=1, axis2=2)), bits(v))
    # the handle-level call on the fitted parameters
    K = em.number_components
    mixing, means = em.mixing_probabilities, np.ascontiguousarray(em.means.T)
    covs = np.stack([np.ascontiguousarray(em.covariance(k)) for k in range(K)])
    parameters = _lib.em_condition(means, covs, [0]) + (_lib.em_condition_covariances(covs, [0])[0],)
    out = run(ctx, X_o, mixing, parameters)
    assert np.array_equal(bits(out["diag"]), bits(v)) and np.array_equal(bits(out["full"]), bits(V)) and np.array_equal(bits(out["y"]), bits(y))
    # no rows
    empty, empty_y = em.conditional_variance(np.empty((0, 1)), [0], covariance=True, return_mean=True)
    assert empty.shape == (0, dM, dM) and empty_y.shape == (0, dM) and empty.dtype == np.float64


def test_the_first_handles_state_is_left_alone(ctx):
    from ml_amd import _lib
    key = (2, 8, 16, (6, 1, 3, 4), N)
    c, parameters = conditioned(key)
    K = len(c["mixing"])
    first_handle = _lib.Data(ctx, c["X"])
    first_handle.em_expectation(c["mixing"], c["means"], c["covs"])
    before = first_handle.em_responsibilities(K)
    second = _lib.Data(ctx, c["X_observed"])
    for full in (False, True):
        _lib.em_conditional_variances(second, c["mixing"], *parameters, full=full, means=True)
    second.close()
    after = first_handle.em_responsibilities(K)
    first_handle.close()
    assert np.array_equal(bits(after), bits(before))
