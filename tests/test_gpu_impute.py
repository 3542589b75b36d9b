"""mlhip_em_impute and EM.impute on the device: every NaN of a block replaced by its conditional expectation given the coordinates
its row has, every row its own pattern. Parameters go in directly through _lib.em_impute; the models come from
condition_reference.model (every principal block of Sigma_k = A A^T / d + 0.5 I has eigenvalues >= 0.5: every pattern is well
conditioned), the restatement is tests/impute_reference.py.

Bitwise: the purity of a row (a permutation of the rows, a table cut into two calls, the row chunk, a device group of three shards on
one GPU, the skip switch), observed entries and complete rows, the log-density of complete rows against mlhip_em_score, rows of all
NaN against the definition, and the composed route against Data.em_conditional_means on every pattern group with `observed` ascending.

Accuracy, on the default route (KERNEL at d <= 32), per pattern group against the longdouble restatement: the imputed values within
condition_reference.limit(err_f64, FLOOR, r_device, ld) with r_device the responsibilities the call returned -- the rule and the
floor of tests/test_gpu_condition.py: steps 1 and 6 are its chain, with maps from a factorization of the same backward error as the
float64 restatement's own; the responsibilities (absolute) and the log-densities (relative to
max(1, |log-density|)) within 4 max(err_f64, FLOOR), the rule tests/hp_limits.py holds the exact E-step to (steps 1 - 5 are its
statement). KERNEL against COMPOSED on the same rows: within the sum of the two limits. The device-built records against
condition_reference.condition in longdouble within the factorization bound of tests/test_condition_host.py. One line per case is
printed."""
import numpy as np
import pytest

import condition_reference as ref
import impute_reference as imp
from hp_limits import FLOOR, FOLD_BOUND

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = 2.0 ** -53
SWITCHES = ("MLHIP_IMPUTE", "MLHIP_IMPUTE_ROWS", "MLHIP_IMPUTE_PATTERNS", "MLHIP_IMPUTE_GRID", "MLHIP_CONDITION", "MLHIP_CONDITION_ROWS", "MLHIP_CONDITION_SKIP",
            "MLHIP_SCORE", "MLHIP_SCORE_ROWS")


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


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def run(context, c, X=None, **kw):
    from ml_amd import _lib
    return _lib.em_impute(context, c["mixing"], c["means"], c["given"], c["X"] if X is None else X, diagonal=c["covariance"] == "diag",
                          tied=c["covariance"] == "tied", log_density=True, responsibilities=True, **kw)


def missing_first(d, dM):
    return tuple(range(dM))


# (seed, d, K, n, kind[, covariance]): the smallest shapes at which a path can go wrong
SHAPES = ([(1, 2, 3, 1, "one"), (2, 3, 1, 63, "bernoulli"), (3, 5, 3, 300, "bernoulli"), (4, 9, 3, 64, "distinct"),
           (5, 3, 65, 65, "bernoulli"), (6, 5, 64, 65, "one"), (7, 17, 3, 65, "bernoulli"), (8, 32, 3, 65, "bernoulli"),
           (9, 2, 3, 2, "distinct")] +
          # dO | dM on each side of every padding edge: 4|5, 5|4, 8|9, 9|8, 16|16, 15|17, 17|15; then 31|1 and 1|31
          [(10, 9, 3, 65, missing_first(9, 5)), (11, 9, 3, 65, missing_first(9, 4)), (12, 17, 3, 65, missing_first(17, 9)),
           (13, 17, 3, 65, missing_first(17, 8)), (14, 32, 3, 65, missing_first(32, 16)), (15, 32, 3, 65, missing_first(32, 17)),
           (16, 32, 3, 65, missing_first(32, 15)), (17, 32, 3, 65, (7,)), (18, 32, 3, 65, tuple(c for c in range(32) if c != 20))] +
          [(19, 5, 3, 65, "bernoulli", "diag"), (20, 5, 3, 65, "bernoulli", "tied")])


def shape_id(s):
    kind = s[4] if isinstance(s[4], str) else "dM%d" % len(s[4])
    return "d%d-K%d-n%d-%s%s" % (s[1], s[2], s[3], kind, "-" + s[5] if len(s) > 5 else "")


@pytest.mark.parametrize("key", SHAPES, ids=shape_id)
def test_against_the_restatement(ctx, key):
    from ml_amd import _lib
    c = imp.case(*key)
    X, f64, ld = c["X"], c["f64"], c["ld"]
    n, d = X.shape
    assert _lib.em_impute_route(d, len(c["mixing"])) == "kernel"
    out, dens, resp = run(ctx, c)
    assert out.shape == (n, d) and dens.shape == (n,) and resp.shape == (n, len(c["mixing"]))
    assert out.flags.c_contiguous and resp.flags.c_contiguous and not np.isnan(out).any()
    gaps = np.isnan(X)
    # observed entries -- complete rows with them -- keep their bits
    assert np.array_equal(bits(out)[~gaps], bits(X)[~gaps])
    # rows of all NaN
    empty = gaps.all(axis=1)
    if empty.any():
        prior = imp.prior_mean(c["mixing"], c["means"])
        assert all(same_bits(row, prior) for row in out[empty])
        assert not dens[empty].any() and not np.signbit(dens[empty]).any()
        assert all(same_bits(row, c["mixing"]) for row in resp[empty])
    # responsibilities and log-densities of every row that has something: steps 1 - 5
    has = ~empty
    if has.any():
        e_r = float(np.abs(resp[has].astype(LD) - ld["r"][has]).max())
        e_r64 = float(np.abs(f64["r"][has].astype(LD) - ld["r"][has]).max())
        scale = np.maximum(1, np.abs(ld["log_density"][has]))
        e_d = float((np.abs(dens[has].astype(LD) - ld["log_density"][has]) / scale).max())
        e_d64 = float((np.abs(f64["log_density"][has].astype(LD) - ld["log_density"][has]) / scale).max())
        print("IMPUTE %s: resp %.2e (float64 %.2e), log-density %.2e (float64 %.2e), floor %.2e" % (shape_id(key), e_r, e_r64, e_d, e_d64, FLOOR))
        assert e_r <= 4 * max(e_r64, FLOOR) and e_d <= 4 * max(e_d64, FLOOR)
    # the imputed values, pattern by pattern: steps 1 and 6 with the responsibilities the call returned
    worst = 0.0
    for (observed, rows_of, g_ld), (_, _, g_64) in zip(ld["groups"], f64["groups"]):
        M = ref.missing_of(d, observed)
        y = out[rows_of][:, M]
        err, err64 = ref.error(y, g_ld["y"]), ref.error(g_64["y"], g_ld["y"])
        lim = ref.limit(err64, FLOOR, resp[rows_of], g_ld)
        worst = max(worst, err / lim)
        assert err <= lim, (observed, err, err64, lim)
    print("IMPUTE %s: %d patterns, worst err / limit of the imputed values %.3f" % (shape_id(key), len(imp.groups(X)), worst))


@pytest.mark.parametrize("key", [(3, 5, 3, 300, "bernoulli"), (8, 32, 3, 65, "bernoulli"), (21, 40, 3, 65, "bernoulli")], ids=shape_id)
def test_composed_is_the_conditional_means_pass_of_every_group(ctx, key, monkeypatch):
    from ml_amd import _lib
    monkeypatch.setenv("MLHIP_IMPUTE", "composed")
    c = imp.case(*key)
    X = c["X"]
    assert _lib.em_impute_route(X.shape[1], len(c["mixing"])) == "composed"
    out, dens, _ = run(ctx, c)
    checked = 0
    for observed, rows_of in imp.groups(X):
        if not 1 <= len(observed) <= X.shape[1] - 1:
            continue
        conditioned = _lib.em_condition(c["means"], c["covs"], observed)
        data = _lib.Data(ctx, np.ascontiguousarray(X[rows_of][:, list(observed)]))
        y, l = data.em_conditional_means(c["mixing"], *conditioned, log_density=True)
        data.close()
        M = ref.missing_of(X.shape[1], observed)
        assert same_bits(np.ascontiguousarray(out[rows_of][:, M]), y) and same_bits(dens[rows_of], l), observed
        checked += 1
    assert checked >= 10


def value_limits(c, resp):
    """Per pattern group (observed, rows, limit of the imputed values' error relative to max |y_ld|, max |y_ld|)."""
    d = c["X"].shape[1]
    limits = []
    for (observed, rows_of, g_ld), (_, _, g_64) in zip(c["ld"]["groups"], c["f64"]["groups"]):
        lim = ref.limit(ref.error(g_64["y"], g_ld["y"]), FLOOR, resp[rows_of], g_ld)
        limits.append((ref.missing_of(d, observed), rows_of, lim, float(np.abs(g_ld["y"]).max())))
    return limits


@pytest.mark.parametrize("key", [(3, 5, 3, 300, "bernoulli"), (7, 17, 3, 65, "bernoulli"), (8, 32, 3, 65, "bernoulli"), (5, 3, 65, 65, "bernoulli")],
                         ids=shape_id)
def test_kernel_against_composed(ctx, key, monkeypatch):
    """The two routes on the same rows: the imputed values within the sum of the two routes' limits (each route's own limit with the
    responsibilities it returned), responsibilities and log-densities within twice the steps 1 - 5 limit. Edge rows take the same path
    on both routes: equal bits."""
    c = imp.case(*key)
    X, f64, ld = c["X"], c["f64"], c["ld"]
    monkeypatch.setenv("MLHIP_IMPUTE", "kernel")
    out_k, dens_k, resp_k = run(ctx, c)
    monkeypatch.setenv("MLHIP_IMPUTE", "composed")
    out_c, dens_c, resp_c = run(ctx, c)
    partial = np.isnan(X).any(axis=1) & ~np.isnan(X).all(axis=1)
    assert same_bits(out_k[~partial], out_c[~partial]) and same_bits(dens_k[~partial], dens_c[~partial]) and same_bits(resp_k[~partial], resp_c[~partial])
    worst = 0.0
    for (M, rows_of, lim_k, scale), (_, _, lim_c, _) in zip(value_limits(c, resp_k), value_limits(c, resp_c)):
        gap = float(np.abs(out_k[rows_of][:, M] - out_c[rows_of][:, M]).max() / scale)
        worst = max(worst, gap / (lim_k + lim_c))
        assert gap <= lim_k + lim_c, (M, gap, lim_k, lim_c)
    has = ~np.isnan(X).all(axis=1)
    e_r64 = float(np.abs(f64["r"][has].astype(LD) - ld["r"][has]).max())
    scale = np.maximum(1, np.abs(np.asarray(ld["log_density"][has], dtype=np.float64)))
    e_d64 = float((np.abs(f64["log_density"][has].astype(LD) - ld["log_density"][has]) / scale).max())
    gap_r = float(np.abs(resp_k[has] - resp_c[has]).max())
    gap_d = float((np.abs(dens_k[has] - dens_c[has]) / scale).max())
    print("IMPUTE %s kernel against composed: values %.3f of the summed limits, resp %.2e, log-density %.2e" % (shape_id(key), worst, gap_r, gap_d))
    assert gap_r <= 8 * max(e_r64, FLOOR) and gap_d <= 8 * max(e_d64, FLOOR)


# (seed, d, K, observed): the patterns of the accuracy cases' paddings, dO = 31 and dO = 1 among them
RECORDS = [(10, 9, 3, tuple(range(5, 9))), (12, 17, 3, tuple(range(9, 17))), (14, 32, 3, tuple(range(16, 32))),
           (17, 32, 3, tuple(c for c in range(32) if c != 7)), (18, 32, 3, (20,)), (22, 5, 65, (0, 2, 3))]


@pytest.mark.parametrize("key", RECORDS, ids=lambda k: "d%d-K%d-dO%d" % (k[1], k[2], len(k[3])))
def test_device_built_records(ctx, key):
    """mlhip_em_impute_condition against the longdouble restatement. The selections are copies. Maps and whitening matrices: relative
    to their largest entry within 4 x the float64 restatement's own error or the backward-error bound of a factorization and its
    substitutions, 4 (dO + 1) eps cond(Sigma_OO) (tests/test_condition_host.py's rule, Higham thm 8.5 / 10.4). The coefficient
    log pi_k - sum_j log L_jj: every L_jj carries a relative error of at most (dO + 1) eps cond, a sum of dO logarithms dO times that,
    and the logarithms and the sum their own roundings relative to the terms: 4 (dO (dO + 1) cond + 2 dO max(1, |terms|)) eps absolute."""
    from ml_amd import _lib
    seed, d, K, observed = key
    mixing, means, covs = ref.model(seed, d, K)
    mu_o, W, coef, A, mu_m = _lib.em_impute_condition(ctx, mixing, means, covs, observed)
    O, M, dO = list(observed), ref.missing_of(d, observed), len(observed)
    assert same_bits(mu_o, np.ascontiguousarray(means[:, O])) and same_bits(mu_m, np.ascontiguousarray(means[:, M]))
    _, S_oo, A64, _, L64 = ref.condition(means, covs, observed)
    _, _, Ald, _, Lld = ref.condition(means, covs, observed, LD)
    worst = 0.0
    for k in range(K):
        cond = np.linalg.cond(S_oo[k])
        bound = 4 * (dO + 1) * EPS * cond
        Wld = ref.forward(Lld[k], np.eye(dO, dtype=LD))
        W64 = ref.forward(L64[k], np.eye(dO))
        for name, got, f64, ld in (("maps", A[k], A64[k], Ald[k]), ("whitening", W[k], W64, Wld)):
            scale = np.abs(ld).max()
            err = float(np.abs(got.astype(LD) - ld).max() / scale)
            err64 = float(np.abs(f64.astype(LD) - ld).max() / scale)
            worst = max(worst, err / max(4 * err64, bound))
            assert err <= max(4 * err64, bound), (name, k, err, err64, bound)
        assert not np.triu(W[k], 1).any()
        logs = np.log(np.diag(Lld[k]))
        coef_ld = np.log(LD(mixing[k])) - logs.sum()
        terms = max(1.0, float(np.abs(logs).max()), abs(float(np.log(mixing[k]))))
        err = abs(float(LD(coef[k]) - coef_ld))
        assert err <= 4 * (dO * (dO + 1) * cond + 2 * dO * terms) * EPS, (k, err)
    print("IMPUTE records d %d K %d dO %d: worst err / limit %.3f" % (d, K, dO, worst))


def test_a_wave_takes_a_second_tile(ctx, monkeypatch):
    """d = 3, K = 3, six patterns, 1500 rows under MLHIP_IMPUTE_GRID=1: the one class has more tiles than the grid holds waves, so every
    wave strides over several tiles. Against the same rows in calls of at most 64 rows on the default grid, bit for bit."""
    from ml_amd import _lib
    mixing, means, covs = ref.model(51, 3, 3)
    X = ref.rows(mixing, means, covs, 1500, 52)
    rng = np.random.default_rng(53)
    masks = np.array([[a, b, c] for a in (0, 1) for b in (0, 1) for c in (0, 1)][1:7], dtype=bool)
    G = imp.with_gaps(X, masks[rng.integers(0, 6, size=1500)])
    assert len(imp.groups(G)) == 6
    small = [_lib.em_impute(ctx, mixing, means, covs, np.ascontiguousarray(G[i:i + 50]), log_density=True, responsibilities=True)
             for i in range(0, 1500, 50)]
    monkeypatch.setenv("MLHIP_IMPUTE_GRID", "1")
    assert _lib.em_impute_route(3, 3, G) == ("kernel", 2)
    big = _lib.em_impute(ctx, mixing, means, covs, G, log_density=True, responsibilities=True)
    assert all_same(big, [np.concatenate(parts) for parts in zip(*small)])


PURITY = [(3, 5, 3, 300, "bernoulli"), (5, 3, 65, 65, "bernoulli"), (7, 17, 3, 65, "bernoulli"), (19, 5, 3, 65, "bernoulli", "diag")]


def all_same(a, b):
    return all(same_bits(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("key", PURITY, ids=shape_id)
def test_a_row_is_a_pure_function_of_the_row(ctx, key, monkeypatch):
    from ml_amd import _lib
    c = imp.case(*key)
    X = c["X"]
    n = X.shape[0]
    base = run(ctx, c)
    # a permutation of the rows permutes the results
    perm = np.random.default_rng(99).permutation(n)
    assert all_same(run(ctx, c, np.ascontiguousarray(X[perm])), [a[perm] for a in base])
    # one call against two calls on the halves
    h = n // 2
    halves = [run(ctx, c, np.ascontiguousarray(X[:h])), run(ctx, c, np.ascontiguousarray(X[h:]))]
    assert all_same([np.concatenate([a, b]) for a, b in zip(*halves)], base)
    # the row chunk, the pattern chunk, the component skip
    for name, value in (("MLHIP_IMPUTE_ROWS", "64"), ("MLHIP_IMPUTE_PATTERNS", "1"), ("MLHIP_IMPUTE_PATTERNS", "3"), ("MLHIP_CONDITION_SKIP", "0")):
        monkeypatch.setenv(name, value)
        assert all_same(run(ctx, c), base), name
        monkeypatch.delenv(name)
    # a device group of three shards on one GPU
    group = _lib.Context.group(3, device_ids=[0, 0, 0])
    try:
        assert all_same(run(group, c), base)
    finally:
        group.close()


def test_complete_rows_have_the_bits_of_the_scoring_pass(ctx):
    from ml_amd import _lib
    c = imp.case(3, 5, 3, 300, "bernoulli")
    X = c["X"]
    whole = ~np.isnan(X).any(axis=1)
    assert whole.sum() >= 2
    out, dens, _ = run(ctx, c)
    assert same_bits(out[whole], X[whole])
    data = _lib.Data(ctx, np.ascontiguousarray(X[whole]))
    scored, _ = data.em_score(c["mixing"], c["means"], c["covs"], labels=False)
    data.close()
    assert same_bits(dens[whole], scored)
    # a block of complete rows alone, and the outputs that are not asked for
    only = _lib.em_impute(ctx, c["mixing"], c["means"], c["covs"], np.ascontiguousarray(X[whole]))
    assert isinstance(only, np.ndarray) and same_bits(only, X[whole])
    assert _lib.em_impute(ctx, c["mixing"], c["means"], c["covs"], np.empty((0, 5))).shape == (0, 5)


@pytest.mark.parametrize("route", ["kernel", "composed"])
def test_a_singular_observed_block_of_one_pattern_is_a_domain_error(ctx, route, monkeypatch):
    """A zero variance on coordinate 1 of one component: every pattern that observes coordinate 1 has a singular Sigma_k,OO. The call
    returns mlhip_em_condition's domain error from finite arithmetic, writes nothing, and the context goes on working."""
    from ml_amd import _lib
    C = _lib.C
    monkeypatch.setenv("MLHIP_IMPUTE", route)
    assert _lib.em_impute_route(4, 3) == route
    mixing, means, covs = ref.model(31, 4, 3)
    variances = np.ascontiguousarray(np.stack([np.diag(s) for s in covs]))
    variances[1, 1] = 0.0
    X = ref.rows(mixing, means, covs, 40, 32)
    G = X.copy()
    G[:, 1] = np.nan                                             # coordinate 1 missing everywhere: fine
    G[::3, 3] = np.nan
    bad = G.copy()
    bad[17, 1] = X[17, 1]                                        # ONE row, one pattern, observes it
    bad[17, 0] = np.nan
    out, dens, resp = np.full((40, 4), 7.0), np.full(40, 7.0), np.full((40, 3), 7.0)
    rc = _lib.lib.mlhip_em_impute(ctx.handle, C.c_uint32(4), C.c_uint32(3), 1, _lib.dptr(mixing), _lib.dptr(means), _lib.dptr(variances),
                                  _lib.dptr(bad), C.c_uint64(40), _lib.dptr(out), _lib.dptr(dens), _lib.dptr(resp))
    assert rc == _lib.E_DOMAIN and b"positive definite" in _lib.lib.mlhip_last_error()
    assert (out == 7).all() and (dens == 7).all() and (resp == 7).all()
    with pytest.raises(ValueError, match="positive definite"):
        _lib.em_impute(ctx, mixing, means, variances, bad, diagonal=True)
    good = _lib.em_impute(ctx, mixing, means, variances, G, diagonal=True)
    assert not np.isnan(good).any() and np.array_equal(bits(good)[~np.isnan(G)], bits(G)[~np.isnan(G)])


def test_model_surface_is_the_handle_function_on_the_fitted_parameters(ctx):
    from ml_amd import _lib
    from ml_amd.cppyml import clustering
    mixing, means, covs = ref.model(41, 4, 2)
    X = ref.rows(mixing, means, covs, 400, 42)
    em = clustering.EM(2)
    em.set_seed(3)
    em.set_maximum_steps(20)
    em.fit(X)
    G = imp.bernoulli_gaps(X[:120], 0.3, 43, complete=[0, 5], empty=[1])
    out, dens, resp = em.impute(G, return_log_density=True, return_responsibilities=True)
    fitted_means = np.ascontiguousarray(em.means.T)
    fitted_covs = np.stack([em.covariance(k) for k in range(2)])
    want = _lib.em_impute(ctx, np.asarray(em.mixing_probabilities), fitted_means, fitted_covs, G, log_density=True, responsibilities=True)
    assert all_same((out, dens, resp), want)
    assert same_bits(em.impute(G), out)
    only_r = em.impute(G, return_responsibilities=True)
    assert len(only_r) == 2 and same_bits(only_r[1], resp)
    # what predict_proba gives where it can: the complete rows. Its E-step may take a fast density form (tests/hp_limits.py: an absolute
    # FOLD_BOUND in a log-responsibility, so in a responsibility), so it is held to that bound's rule, not to equal bits
    whole = ~np.isnan(G).any(axis=1)
    assert np.abs(em.predict_proba(np.ascontiguousarray(G[whole])) - resp[whole]).max() <= 4 * max(FOLD_BOUND, FLOOR)
    assert same_bits(dens[whole], em.score_samples(np.ascontiguousarray(G[whole])))
