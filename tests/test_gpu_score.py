"""mlhip_em_score and the batch queries built on it (EM.score_samples / score / predict / predict_proba, KMeans.predict) against the
CPU oracle and the extended-precision reference, on the held-out cases of tests/test_score_cases.py (which shows on the CPU that no
row of them is near a tie or underflows in the reference: every row is compared here).

The log-density rule is DESIGN.md section 4.1's: err = max_i |v_i - hp_i| / max(1, |hp_i|) against the extended-precision values,
err_gpu over all rows, err_cpu over 256 rows of the oracle, and err_gpu <= 4 max(err_cpu, 8 * 2^-53)."""
import numpy as np
import pytest

from oracle import hp_reference as hp
from test_score_cases import SHAPES, density_error, held_out, oracle_density_rows, oracle_labels, sample_rows

pytestmark = pytest.mark.gpu

FLOOR = 8 * 2.0 ** -53


@pytest.fixture(scope="module")
def ctx():
    from ml_amd import _lib
    c = _lib.Context()
    yield c
    c.close()


def _expected_route(d):
    return "scalar_fed" if d < 12 else "matrix4" if d <= 128 else "composed"


def _scored(ctx, Y, pi, mu, S, route, diagonal=False):
    """em_score on a fresh handle with the launch counters checked against `route`."""
    from ml_amd import _lib
    dt = _lib.Data(ctx, Y)
    assert dt.em_score_route(len(pi)) == route
    ctx.timing_enable(True)
    ctx.timing_reset()
    dens, labels = dt.em_score(pi, mu, S, diagonal=diagonal)
    n_score, n_estep = ctx.timing_get("em_score")[1], ctx.timing_get("em_estep")[1]
    ctx.timing_enable(False)
    dt.close()
    assert n_score >= 1
    assert (n_estep >= 1) if route == "composed" else (n_estep == 0)
    return dens, labels


def _check_against_references(oracle, Y, pi, mu, S, dens, labels, what, diagonal=False):
    want_labels, _ = oracle_labels(oracle, Y, pi, mu, S, diagonal)
    Sfull = S
    lw = hp.log_weights(Y, pi, mu, Sfull)
    _, lse = hp._normalise(lw)
    rows = sample_rows(len(Y))
    err_cpu = density_error(oracle_density_rows(oracle, Y, pi, mu, S, rows, diagonal), lse[rows])
    err_gpu = density_error(dens, lse)
    print("%s: err_gpu %.3g err_cpu %.3g (bound %.3g)" % (what, err_gpu, err_cpu, 4 * max(err_cpu, FLOOR)))
    assert np.array_equal(labels, want_labels), np.nonzero(labels != want_labels)[0][:10]
    assert np.all(np.isfinite(dens))
    assert err_gpu <= 4 * max(err_cpu, FLOOR), (err_gpu, err_cpu)


@pytest.mark.parametrize("d,K,n,offset", SHAPES)
def test_labels_and_log_densities(ctx, oracle, d, K, n, offset):
    Y, pi, mu, S = held_out(oracle, d, K, n, offset)
    dens, labels = _scored(ctx, Y, pi, mu, S, _expected_route(d))
    _check_against_references(oracle, Y, pi, mu, S, dens, labels, "score d=%d K=%d" % (d, K))


@pytest.mark.parametrize("d,K,n,offset", [s for s in SHAPES if s[0] <= 128])
def test_composed_route_agrees(ctx, oracle, monkeypatch, d, K, n, offset):
    Y, pi, mu, S = held_out(oracle, d, K, n, offset)
    monkeypatch.setenv("MLHIP_SCORE", "composed")
    dens, labels = _scored(ctx, Y, pi, mu, S, "composed")
    _check_against_references(oracle, Y, pi, mu, S, dens, labels, "composed d=%d K=%d" % (d, K))
    # many chunks give the bits of one chunk: the pass is per row
    monkeypatch.setenv("MLHIP_SCORE_ROWS", "256")
    dens_c, labels_c = _scored(ctx, Y, pi, mu, S, "composed")
    assert np.array_equal(dens_c, dens) and np.array_equal(labels_c, labels)


@pytest.mark.parametrize("d,K,n,offset", [s for s in SHAPES if s[0] in (16, 32)])
def test_scalar_fed_kernel_up_to_32_dimensions(ctx, oracle, monkeypatch, d, K, n, offset):
    Y, pi, mu, S = held_out(oracle, d, K, n, offset)
    monkeypatch.setenv("MLHIP_ESTEP", "valu")
    dens, labels = _scored(ctx, Y, pi, mu, S, "scalar_fed")
    _check_against_references(oracle, Y, pi, mu, S, dens, labels, "valu d=%d K=%d" % (d, K))


@pytest.mark.parametrize("d,K,n,offset", [SHAPES[0], SHAPES[4], SHAPES[6], SHAPES[9], SHAPES[11]])
def test_chunk_rows_and_device_group_give_the_same_bits(ctx, oracle, monkeypatch, d, K, n, offset):
    from ml_amd import _lib
    Y, pi, mu, S = held_out(oracle, d, K, n, offset)
    dens, labels = _scored(ctx, Y, pi, mu, S, _expected_route(d))
    group = _lib.Context.group(2, device_ids=[0, 0])
    gd = _lib.Data(group, Y)
    dens_g, labels_g = gd.em_score(pi, mu, S)
    gd.close()
    group.close()
    assert np.array_equal(dens_g, dens) and np.array_equal(labels_g, labels)
    monkeypatch.setenv("MLHIP_SCORE_ROWS", "256")
    dens_r, labels_r = _scored(ctx, Y, pi, mu, S, _expected_route(d))
    assert np.array_equal(dens_r, dens) and np.array_equal(labels_r, labels)


# ---- the handle is left alone (the construction of tests/test_gpu_handle_state.py) ----

def _mixture(d, n, seed):
    rng = np.random.default_rng(seed)
    centres = 3.0 * rng.standard_normal((8, d))
    return np.ascontiguousarray(centres[rng.integers(0, 8, n)] + rng.standard_normal((n, d)) + 5.0), centres + 5.0


def _start(X, centres, K, seed):
    rng = np.random.default_rng(seed)
    mu = centres[np.arange(K) % len(centres)] + 0.1 * rng.standard_normal((K, X.shape[1]))
    return np.full(K, 1.0 / K), mu, np.stack([np.diag(np.var(X, axis=0))] * K)


@pytest.mark.parametrize("d,n,K,switches", [
    (2, 12000, 3, {}),                                   # fused step: records only on the handle
    (8, 9000, 5, {}),                                    # scalar-fed E-step + statistics kernel
    (16, 20000, 8, {"MLHIP_MSTATS_SPARSE": "0"}),        # matrix-core E-step, self-normalising statistics (call history)
    (16, 20000, 8, {"MLHIP_MSTATS_SPARSE": "1"}),
    (16, 20000, 8, {}),                                  # ... with the sparse / dense choice left to the call history
    (192, 3000, 2, {}),                                  # composed scoring route
])
def test_a_score_call_leaves_the_handle_alone(ctx, monkeypatch, d, n, K, switches):
    from ml_amd import _lib
    for name, value in switches.items():
        monkeypatch.setenv(name, value)
    X, centres = _mixture(d, n, 1000 + d)
    pi, mu, S = _start(X, centres, K, 17 + K)
    pi2, mu2, S2 = _start(X, centres, K + 2, 5)           # other parameters, another K

    def run(with_score):
        dt = _lib.Data(ctx, X)
        out = []
        p = (pi, mu, S)
        for _ in range(4):                                # (four steps: the sparse kernel's choice reads the pass two back)
            ll, *p = dt.em_step(*p)
            out += [ll, *p]
            if with_score:
                dt.em_score(pi2, mu2, S2)
        out += [dt.em_labels(K), dt.em_responsibilities(K)]
        if with_score:
            dt.em_score(pi2, mu2, S2)
        out += [dt.em_labels(K), *dt.em_maximisation(K), *dt.em_step(*p)]
        dt.kmeans_step(centres[:3])
        if with_score:
            dt.em_score(pi2, mu2, S2)
        out += [dt.kmeans_labels(), dt.kmeans_step(centres[:3])[1]]     # the label history: nothing changed since
        dt.close()
        return out

    want, got = run(False), run(True)
    differing = [j for j, (a, b) in enumerate(zip(got, want)) if not np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)]
    assert len(got) == len(want) and not differing, differing


# ---- edges ----

def test_zero_weight_component_is_never_the_label(ctx, oracle):
    d, K, n, offset = SHAPES[4]
    Y, pi, mu, S = held_out(oracle, d, K, n, offset)
    pi = pi.copy()
    mu = mu.copy()
    mu[1] = Y.mean(axis=0)                                # it would win many rows if it had any weight
    pi[1] = 0.0
    pi /= pi.sum()
    for route, env in (("scalar_fed", {}), ("composed", {"MLHIP_SCORE": "composed"})):
        with pytest.MonkeyPatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            dens, labels = _scored(ctx, Y, pi, mu, S, route)
        assert not np.any(labels == 1)
        _check_against_references(oracle, Y, pi, mu, S, dens, labels, "zero weight (%s)" % route)


@pytest.mark.parametrize("d,K,n,offset", [SHAPES[4], SHAPES[6], SHAPES[11]])
@pytest.mark.parametrize("what", ["mean", "covariance"])
def test_nan_parameters_poison_the_density(ctx, oracle, d, K, n, offset, what):
    Y, pi, mu, S = held_out(oracle, d, K, n, offset)
    mu, S = mu.copy(), S.copy()
    if what == "mean":
        mu[K - 1, 0] = np.nan
    else:
        S[K - 1, 0, 0] = np.nan
    dens, labels = _scored(ctx, Y, pi, mu, S, _expected_route(d))
    assert np.all(np.isnan(dens))
    assert np.all(labels == 0xffffffff)                   # a NaN row has no maximum (em_resp_kernel leaves the same)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MLHIP_SCORE", "composed")
        dens_c, labels_c = _scored(ctx, Y, pi, mu, S, "composed")
    assert np.all(np.isnan(dens_c)) and np.all(labels_c == 0xffffffff)
    em = oracle.EM(K)
    em.set_parameters(mu, S, pi)
    em.expectation_step(Y)
    assert np.isnan(em.log_likelihood)


@pytest.mark.parametrize("d,K,n,offset", [SHAPES[1], SHAPES[6]])
def test_far_outlier_stays_finite(ctx, oracle, d, K, n, offset):
    Y, pi, mu, S = held_out(oracle, d, K, n, offset)
    Y = Y.copy()
    Y[7] = Y[7] + 400.0                                   # the reference's exp(-q / 2) underflows for every component
    em = oracle.EM(K)
    em.set_parameters(mu, S, pi)
    em.expectation_step(np.ascontiguousarray(Y[7:8]))
    assert em.log_likelihood == -np.inf or np.isnan(em.log_likelihood)
    dens, labels = _scored(ctx, Y, pi, mu, S, _expected_route(d))
    lw = hp.log_weights(Y, pi, mu, S)
    _, lse = hp._normalise(lw)
    assert np.isfinite(dens[7]) and labels[7] == int(lw[:, 7].argmax())
    err = density_error(dens, lse)
    print("outlier d=%d: log-density %.6g, err_gpu %.3g" % (d, dens[7], err))
    assert err <= 4 * FLOOR


@pytest.mark.parametrize("d,K,n,offset", [(4, 3, 3001, 3.0), (16, 8, 4001, 2.0), (40, 3, 2001, 0.0)])
def test_diagonal_model(ctx, oracle, d, K, n, offset):
    from oracle import hp_cases
    X, pi0, mu0, var0 = hp_cases.problem(d, K, n, offset, diagonal=True)
    half = n // 2
    em = oracle.EM(K)
    em.set_covariance_type("diag")
    em.set_parameters(mu0, np.stack([np.diag(v) for v in var0]), pi0)
    em.expectation_step(np.ascontiguousarray(X[:half]))
    em.maximisation_step(np.ascontiguousarray(X[:half]))
    pi, mu, S = em.mixing_probabilities.copy(), em.means.copy(), em.covariances.copy()
    var = np.stack([np.diag(s) for s in S])
    Y = np.ascontiguousarray(X[half:])
    dens, labels = _scored(ctx, Y, pi, mu, var, _expected_route(d), diagonal=True)
    want_labels, _ = oracle_labels(oracle, Y, pi, mu, S, diagonal=True)
    _, lse = hp._normalise(hp.log_weights_diag(Y, pi, mu, var))
    rows = sample_rows(len(Y))
    err_cpu = density_error(oracle_density_rows(oracle, Y, pi, mu, S, rows, diagonal=True), lse[rows])
    err_gpu = density_error(dens, lse)
    print("diagonal d=%d K=%d: err_gpu %.3g err_cpu %.3g" % (d, K, err_gpu, err_cpu))
    assert np.array_equal(labels, want_labels)
    assert err_gpu <= 4 * max(err_cpu, FLOOR)


@pytest.mark.parametrize("d", [3, 16, 192])
@pytest.mark.parametrize("K,n", [(1, 300), (3, 1), (4, 255)])
def test_small_blocks_and_one_component(ctx, oracle, d, K, n):
    Y, pi, mu, S = held_out(oracle, d, max(K, 2), 3001 if d < 100 else 8001, 1.0)   # (enough rows per component for d = 192)
    pi, mu, S = pi[:K] / pi[:K].sum(), mu[:K], S[:K]
    Y = np.ascontiguousarray(Y[:n])
    dens, labels = _scored(ctx, Y, pi, mu, S, _expected_route(d))
    assert dens.shape == (n,) and labels.shape == (n,)
    lw = hp.log_weights(Y, pi, mu, S)
    _, lse = hp._normalise(lw)
    assert np.array_equal(labels, lw.argmax(axis=0).astype(np.uint32))
    assert density_error(dens, lse) <= 4 * max(density_error(oracle_density_rows(oracle, Y, pi, mu, S, sample_rows(n)), lse[sample_rows(n)]), FLOOR)


def test_only_one_output_and_argument_checks(ctx, oracle):
    from ml_amd import _lib
    d, K, n, offset = SHAPES[2]
    Y, pi, mu, S = held_out(oracle, d, K, n, offset)
    dt = _lib.Data(ctx, Y)
    dens, labels = dt.em_score(pi, mu, S)
    assert dt.em_score(pi, mu, S, labels=False)[1] is None and np.array_equal(dt.em_score(pi, mu, S, labels=False)[0], dens)
    assert dt.em_score(pi, mu, S, densities=False)[0] is None and np.array_equal(dt.em_score(pi, mu, S, densities=False)[1], labels)
    with pytest.raises(ValueError, match="no E-step results"):
        dt.em_labels(K)                                   # scoring left no E-step results behind
    ll = _lib.C.c_double()
    rc_e = _lib.lib.mlhip_em_expectation(ctx.handle, dt.handle, 0, _lib.dptr(pi), _lib.dptr(mu), _lib.dptr(S), _lib.C.byref(ll))
    rc_s = _lib.lib.mlhip_em_score(ctx.handle, dt.handle, 0, 0, _lib.dptr(pi), _lib.dptr(mu), _lib.dptr(S), _lib.dptr(dens), None)
    assert rc_s == rc_e == _lib.E_INVALID_ARGUMENT
    rc_e = _lib.lib.mlhip_em_expectation(ctx.handle, dt.handle, K, None, _lib.dptr(mu), _lib.dptr(S), _lib.C.byref(ll))
    rc_s = _lib.lib.mlhip_em_score(ctx.handle, dt.handle, K, 0, None, _lib.dptr(mu), _lib.dptr(S), _lib.dptr(dens), None)
    assert rc_s == rc_e == _lib.E_INVALID_ARGUMENT
    bad = S.copy()
    bad[0] = -np.eye(d)                                   # a covariance that cannot be factored: whatever the E-step answers
    rc_e = _lib.lib.mlhip_em_expectation(ctx.handle, dt.handle, K, _lib.dptr(pi), _lib.dptr(mu), _lib.dptr(bad), _lib.C.byref(ll))
    rc_s = _lib.lib.mlhip_em_score(ctx.handle, dt.handle, K, 0, _lib.dptr(pi), _lib.dptr(mu), _lib.dptr(bad), _lib.dptr(dens), None)
    assert rc_s == rc_e
    dt.close()


# ---- the model classes ----

def _fitted(K, X):
    from ml_amd.cppyml import clustering
    em = clustering.EM(K)
    em.set_seed(5)
    em.set_maximum_steps(300)
    em.set_absolute_tolerance(1e-10)
    em.set_relative_tolerance(1e-10)
    em.fit(X)
    return em


@pytest.mark.parametrize("d,K,n,offset", [SHAPES[0], SHAPES[4], SHAPES[6], SHAPES[9]])
def test_model_methods_against_the_oracle(oracle, monkeypatch, d, K, n, offset):
    from oracle import hp_cases
    X, *_ = hp_cases.problem(d, K, n, offset)
    half = n // 2
    Xtrain, Xtest = np.ascontiguousarray(X[:half]), np.ascontiguousarray(X[half:])
    em = _fitted(K, Xtrain)
    pi, mu = em.mixing_probabilities, np.ascontiguousarray(em.means.T)
    S = np.stack([np.ascontiguousarray(em.covariance(k)) for k in range(K)])
    dens, labels, proba = em.score_samples(Xtest), em.predict(Xtest), em.predict_proba(Xtest)
    assert labels.dtype == np.uint32 and proba.shape == (len(Xtest), K) and proba.flags.f_contiguous
    want_labels, want_resp = oracle_labels(oracle, Xtest, pi, mu, S)
    lw = hp.log_weights(Xtest, pi, mu, S)
    _, lse = hp._normalise(lw)
    order = np.sort(lw, axis=0)
    tie_free = np.asarray((order[-1] - order[-2]) > 1e-9) if K > 1 else np.ones(len(Xtest), bool)
    assert tie_free.all()                                 # (a fitted model's held-out rows: none within rounding of a tie)
    assert np.array_equal(labels, want_labels)
    rows = sample_rows(len(Xtest))
    err_cpu = density_error(oracle_density_rows(oracle, Xtest, pi, mu, S, rows), lse[rows])
    err_gpu = density_error(dens, lse)
    print("model d=%d K=%d: err_gpu %.3g err_cpu %.3g" % (d, K, err_gpu, err_cpu))
    assert err_gpu <= 4 * max(err_cpu, FLOOR)
    assert np.max(np.abs(proba - want_resp)) <= 1e-12
    assert np.max(np.abs(proba.sum(axis=1) - 1)) <= 4 * 2.0 ** -53 * K
    # score: the sequential mean; on the training block the log-likelihood of one more E-step at the final parameters
    total = 0.0
    for v in dens.tolist():
        total += v
    assert em.score(Xtest) == total / len(dens)
    e2 = oracle.EM(K)
    e2.set_parameters(mu, S, pi)
    e2.expectation_step(Xtrain)
    assert abs(em.score(Xtrain) - e2.log_likelihood) <= 1e-12 * abs(e2.log_likelihood)
    assert em.converged                                   # (the cases converge: the label comparison below always runs)
    lw_train = hp.log_weights(Xtrain, pi, mu, S)
    o = np.sort(lw_train, axis=0)
    assert float((o[-1] - o[-2]).min()) > 1e-9
    e2.calculate_labels()
    assert np.array_equal(em.predict(Xtrain), np.asarray(e2.labels).astype(np.uint32))
    assert np.array_equal(em.predict(Xtrain), em.labels)
    for i in range(64):
        assert labels[i] == int(np.argmax(em.assign_responsibilities(Xtest[i])))
    # many uploads give the same bits
    monkeypatch.setenv("MLHIP_SCORE_ROWS", "256")
    assert np.array_equal(em.score_samples(Xtest), dens) and np.array_equal(em.predict(Xtest), labels)
    # (predict_proba runs the fit's E-step per batch, whose FOLD form works about each batch's own mean: DESIGN.md section 4's 1e-12)
    assert np.max(np.abs(em.predict_proba(Xtest) - proba)) <= 1e-12
    monkeypatch.delenv("MLHIP_SCORE_ROWS")
    # what fit refuses, these refuse
    for bad in (Xtest.astype(np.float32), np.asfortranarray(Xtest), Xtest[:, 0], Xtest.tolist()):
        for method in (em.score_samples, em.score, em.predict, em.predict_proba):
            with pytest.raises(TypeError):
                method(bad)
    wrong = np.ascontiguousarray(np.hstack([Xtest, Xtest[:, :1]]))
    for method in (em.score_samples, em.predict, em.predict_proba):
        with pytest.raises(ValueError):
            method(wrong)
    from ml_amd.cppyml import clustering
    with pytest.raises(ValueError):
        clustering.EM(K).score_samples(Xtest)             # not fitted: as assign_responsibilities
    empty = np.empty((0, d))
    assert em.score_samples(empty).shape == (0,) and em.predict(empty).shape == (0,) and em.predict_proba(empty).shape == (0, K)
    assert np.isnan(em.score(empty))                      # the mean of nothing


@pytest.mark.parametrize("d,K,n", [(2, 5, 3001), (16, 10, 3001), (72, 6, 2001)])
def test_kmeans_predict(oracle, monkeypatch, d, K, n):
    from ml_amd.cppyml import clustering
    from oracle import hp_cases
    X, *_ = hp_cases.problem(d, K, n, 1.0)
    half = n // 2
    Xtrain, Xtest = np.ascontiguousarray(X[:half]), np.ascontiguousarray(X[half:])
    km = clustering.KMeans(K)
    km.set_seed(3)
    km.fit(Xtrain)
    labels, dist = km.predict(Xtest, return_distances=True)
    assert labels.dtype == np.uint32 and np.array_equal(km.predict(Xtest), labels)
    for i in sample_rows(len(Xtest)):
        assert km.assign_label(Xtest[i]) == (int(labels[i]), float(dist[i]))
    ref = oracle.KMeans(K)
    ref.set_centroids(km.centroids, len(Xtest))
    ref.assignment_step(Xtest)
    assert np.array_equal(labels, np.asarray(ref.labels).astype(np.uint32))
    monkeypatch.setenv("MLHIP_SCORE_ROWS", "256")
    l2, d2 = km.predict(Xtest, return_distances=True)
    assert np.array_equal(l2, labels) and np.array_equal(d2, dist)
    with pytest.raises(TypeError):
        km.predict(Xtest.astype(np.float32))
    with pytest.raises(ValueError):
        km.predict(np.ascontiguousarray(Xtest[:, :-1]) if d > 1 else np.ascontiguousarray(np.hstack([Xtest, Xtest])))


def test_sklearn_fixture(ctx):
    """tests/golden/score_mousie_sklearn.npz (tests/test_score_golden.py: the oracle's side): the model classes take no parameters
    from outside, so the pinned parameters go through the C ABI the model methods are built on."""
    from conftest import load_golden
    from ml_amd import _lib
    g, s = load_golden("mousie_sklearn.npz"), load_golden("score_mousie_sklearn.npz")
    pi, mu, S, Y = g["sklearn_weights"], g["sklearn_means"], g["sklearn_covariances"], np.ascontiguousarray(s["Y"])
    dt = _lib.Data(ctx, Y)
    dens, labels = dt.em_score(pi, mu, S)
    dt.em_expectation(pi, mu, S)
    proba = dt.em_responsibilities(3)
    dt.close()
    assert np.max(np.abs(dens - s["sklearn_score_samples"]) / np.abs(s["sklearn_score_samples"])) <= 1e-12
    assert np.max(np.abs(proba - s["sklearn_predict_proba"])) <= 1e-12
    assert np.array_equal(labels, s["sklearn_predict"])
