"""Tied-covariance EM (one covariance shared by all components; an extension -- the reference is full-covariance only,
ML/EM.hpp:175) on the GPU: the fused HIP kernel (device/em_tied.hip) and the composed route (the full-covariance kernels on K copies
of the covariance, pooled) through the C ABI, the device group and the Python facade, against the scikit-learn
covariance_type='tied' fixtures and a numpy restatement. Tolerances as in tests/test_gpu_diag.py: log-likelihood 1e-12 relative,
mixing / means 1e-11, covariance 1e-10 (max-norm relative), responsibilities 1e-12 absolute, labels exact, histories 1e-11."""
import glob
import os

import numpy as np
import pytest
import scipy.linalg
import scipy.special
import scipy.stats

from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

TIED_CASES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "em_tied_onestep_*.npz")))


def relerr(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, np.max(np.abs(b)))


@pytest.fixture(scope="module")
def ctx():
    from ml_amd import _lib
    c = _lib.Context()
    yield c
    c.close()


def _data(ctx, X):
    from ml_amd import _lib
    return _lib.Data(ctx, np.ascontiguousarray(X, dtype=np.float64))


def tied_step(X, pi, mu, S, w=None):
    """One tied EM step in numpy: (ll, log-responsibilities, R, pi1, mu1, Sigma1). The covariance in its two-pass form
    sum_k sum_i w_i r_ik (x_i - mu_k)(x_i - mu_k)^T / W + 1e-15 I about the NEW means (no cancellation)."""
    n, d = X.shape
    K = len(pi)
    w = np.ones(n) if w is None else w
    L = np.linalg.cholesky(S)
    Z = (X[:, None, :] - mu[None, :, :]).reshape(n * K, d)
    Y = scipy.linalg.solve_triangular(L, Z.T, lower=True)
    q = np.sum(Y * Y, axis=0).reshape(n, K)
    logw = np.log(pi)[None, :] - np.sum(np.log(np.diag(L))) - 0.5 * q - 0.5 * d * np.log(2 * np.pi)
    lse = scipy.special.logsumexp(logw, axis=1)
    R = np.exp(logw - lse[:, None])
    W = w.sum()
    ll = np.sum(w * lse) / W
    wr = R * w[:, None]
    S0 = wr.sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        mu1 = wr.T @ X / S0[:, None]
    S1 = np.zeros((d, d))
    for k in range(K):
        D = X - mu1[k]
        S1 += (D * wr[:, k][:, None]).T @ D
    return ll, logw, R, S0 / W, mu1, S1 / W + 1e-15 * np.eye(d)


def tied_sample(seed, n, d, K, sep=2.5):
    """A tied mixture sample and a perturbed start (pi0, mu0, Sigma0)."""
    rng = np.random.default_rng(seed)
    means = sep * rng.standard_normal((K, d))
    A = rng.standard_normal((d, d))
    Sigma = A @ A.T / d + 0.5 * np.eye(d)
    X = means[rng.integers(0, K, n)] + rng.standard_normal((n, d)) @ np.linalg.cholesky(Sigma).T
    B = 0.1 * rng.standard_normal((d, d))
    return np.ascontiguousarray(X), rng.dirichlet(4 * np.ones(K)), means + 0.2 * rng.standard_normal((K, d)), Sigma + B @ B.T + 0.1 * np.eye(d)


def check_step(out, ref):
    ll, pi1, mu1, S1 = out
    ll_r, _, _, pi_r, mu_r, S_r = ref
    assert abs(ll - ll_r) <= 1e-12 * abs(ll_r), (ll, ll_r)
    assert relerr(pi1, pi_r) < 1e-11
    assert relerr(mu1, mu_r) < 1e-11
    assert relerr(S1, S_r) < 1e-10
    assert np.array_equal(S1, S1.T)


@pytest.mark.parametrize("case", TIED_CASES)
def test_tied_step_matches_sklearn_fixture_on_both_routes(ctx, case, monkeypatch):
    g = load_golden(case)
    K = g["pi0"].size
    dt = _data(ctx, g["X"])
    results = {}
    for route in ("kernel", "composed"):
        monkeypatch.setenv("MLHIP_TIED", route)                   # (by default d4_K3 runs composed: see test_tied_default_route)
        assert dt.em_tied_route(K) == route
        ll, pi1, mu1, S1 = dt.em_step_tied(g["pi0"], g["mu0"], g["Sigma0"])
        assert abs(ll - float(g["ll0"])) <= 1e-12 * abs(float(g["ll0"]))
        assert relerr(pi1, g["pi1"]) < 1e-11
        assert relerr(mu1, g["mu1"]) < 1e-11
        assert relerr(S1, g["Sigma1"]) < 1e-10
        # the N x K block is rebuilt on demand from the same parameters
        assert np.max(np.abs(dt.em_responsibilities(K) - g["R0"])) < 1e-12
        assert np.array_equal(dt.em_labels(K), g["labels0"])
        results[route] = (ll, pi1, mu1, S1)
    a, b = results["kernel"], results["composed"]
    assert abs(a[0] - b[0]) <= 1e-12 * abs(b[0])
    assert relerr(a[1], b[1]) < 1e-11 and relerr(a[2], b[2]) < 1e-11 and relerr(a[3], b[3]) < 1e-10
    dt.close()


EDGE_SHAPES = ([(n, 3, 2) for n in (1, 63, 64, 65, 257)] + [(300, 8, K) for K in (1, 16, 17, 64)] +
               [(300, d, 3) for d in (1, 5, 12, 31, 32)] + [(300, 33, 3), (300, 8, 65)] +
               # d = 32 with 2, 3 and 4 row blocks of components: the largest LDS footprints; K = 40 also at d = 16 (two workgroups per CU below)
               [(300, 32, 24), (300, 32, 40), (300, 32, 64), (300, 16, 40)] +
               # enough samples that a wave re-stages its LDS tile for a second trip of the tile loop (above grid x 4 x 64 samples:
               # 131 072 with two workgroups per CU on 256 CUs, 32 768 with one per CU and two row-block groups)
               [(140001, 8, 17), (40001, 32, 40)])


@pytest.mark.parametrize("n,d,K", EDGE_SHAPES)
def test_tied_step_edge_shapes(ctx, n, d, K, monkeypatch):
    monkeypatch.setenv("MLHIP_TIED", "kernel")                    # the kernel wherever it exists, also where composed is the default
    X, pi0, mu0, S0 = tied_sample(100 * d + K + n, n, d, K)
    ref = tied_step(X, pi0, mu0, S0)
    dt = _data(ctx, X)
    assert dt.em_tied_route(K) == ("kernel" if d <= 32 and K <= 64 else "composed")
    out = dt.em_step_tied(pi0, mu0, S0)
    check_step(out, ref)
    assert np.max(np.abs(dt.em_responsibilities(K) - ref[2])) < 1e-12
    srt = np.sort(ref[2], axis=1)
    assert K == 1 or np.min(srt[:, -1] - srt[:, -2]) > 1e-9                     # no near-tie in these samples: every label is compared
    assert np.array_equal(dt.em_labels(K), np.argmax(ref[1], axis=1))
    dt.close()


def test_tied_default_route(ctx, monkeypatch):
    """Without the switch: composed where the full-covariance step is the vector-unit fused kernel (measured faster), else the kernel."""
    monkeypatch.delenv("MLHIP_TIED", raising=False)
    for d, K, want in ((4, 3, "composed"), (2, 3, "composed"), (8, 5, "kernel"), (16, 16, "kernel"), (32, 64, "kernel"), (33, 3, "composed")):
        dt = _data(ctx, np.random.default_rng(d).standard_normal((300, d)))
        if d <= 32:
            assert (dt.em_route(K)["fused_form"] == "valu") == (want == "composed")
        assert dt.em_tied_route(K) == want
        dt.close()


def test_tied_iterate(ctx):
    n, d, K, steps = 2000, 6, 4, 6
    X, pi0, mu0, S0 = tied_sample(77, n, d, K)
    pi, mu, S, hist_ref = pi0, mu0, S0, []
    for _ in range(steps):
        ll, _, _, pi, mu, S = tied_step(X, pi, mu, S)
        hist_ref.append(ll)
    dt = _data(ctx, X)
    assert dt.em_tied_route(K) == "kernel"
    done, conv, ll, pi1, mu1, S1, hist = dt.em_iterate(pi0, mu0, S0, steps, tied=True)
    assert done == steps and not conv and ll == hist[-1]
    assert relerr(hist, np.array(hist_ref)) < 1e-11
    assert np.all(np.diff(hist) >= -1e-12 * np.abs(hist[1:]))
    assert relerr(pi1, pi) < 1e-11 and relerr(mu1, mu) < 1e-11 and relerr(S1, S) < 1e-10
    assert np.array_equal(S1, S1.T)
    np.linalg.cholesky(S1)
    assert abs(pi1.sum() - 1) < 1e-12
    shift = dt.shift
    Xt = X - shift
    T = Xt.T @ Xt / n
    M = mu1 - shift
    assert np.max(np.abs(S1 - 1e-15 * np.eye(d) + (M * pi1[:, None]).T @ M - T)) <= 1e-11 * np.max(np.abs(T))
    again = dt.em_iterate(pi0, mu0, S0, steps, tied=True)
    assert again[2] == ll and np.array_equal(again[3], pi1) and np.array_equal(again[4], mu1) and np.array_equal(again[5], S1)
    assert np.array_equal(again[6], hist)
    dt.close()


def _numpy_fit(X, pi, mu, S, steps):
    ll = None
    for _ in range(steps):
        ll, _, _, pi, mu, S = tied_step(X, pi, mu, S)
    return ll, pi, mu, S


@pytest.mark.parametrize("maximise_first", [False, True], ids=["means_start", "maximise_first"])
def test_python_facade_tied(ctx, maximise_first):
    from ml_amd.cppyml import clustering as cl
    Xall = np.ascontiguousarray(load_golden("mousie_sklearn.npz")["X"])
    held = Xall[::5].copy()
    X = np.ascontiguousarray(np.delete(Xall, np.s_[::5], axis=0))
    n, d = X.shape
    K, steps = 3, 6
    c0 = np.ascontiguousarray(X[[0, n // 2, n - 1]])
    em = cl.EM(K)
    em.set_covariance_type("tied")
    em.set_maximum_steps(steps)
    em.set_absolute_tolerance(0)
    em.set_relative_tolerance(0)
    if maximise_first:
        em.set_maximise_first(True)
        em.set_responsibilities_initialiser(cl.ClosestCentroid(cl.FixedCentroids(c0)))
        # the facade's first parameters: the one-hot M-step of the nearest-centroid labels, its covariances pooled
        lab = np.argmin(((X[:, None, :] - c0[None, :, :]) ** 2).sum(axis=2), axis=1)
        pi0 = np.bincount(lab, minlength=K) / n
        mu0 = np.stack([X[lab == k].mean(axis=0) for k in range(K)])
        S0 = sum(pi0[k] * (np.cov(X[lab == k].T, bias=True) + 1e-15 * np.eye(d)) for k in range(K))
    else:
        em.set_means_initialiser(cl.FixedCentroids(c0))
        pi0, mu0, S0 = np.full(K, 1.0 / K), c0, np.cov(X.T)          # (the pooled start: K copies of the sample covariance)
    em.fit(X)
    assert em.steps_done == steps
    ll, pi, mu, S = _numpy_fit(X, pi0, mu0, S0, steps)
    assert abs(em.log_likelihood - ll) <= 1e-11 * abs(ll)
    assert relerr(em.mixing_probabilities, pi) < 1e-11 and relerr(em.means.T, mu) < 1e-11
    assert relerr(em.covariance(0), S) < 1e-10
    assert np.array_equal(em.covariance(0), em.covariance(2)) and np.array_equal(em.covariance(0), em.covariance(1))
    # batch queries on held-out rows == mlhip_em_score with the tied type and the fitted parameters
    pi_f, mu_f, S_f = em.mixing_probabilities, np.ascontiguousarray(em.means.T), np.ascontiguousarray(em.covariance(0))
    hd = _data(ctx, held)
    dens, lab = hd.em_score(pi_f, mu_f, S_f, tied=True)
    hd.close()
    assert np.array_equal(em.score_samples(held), dens)
    assert np.array_equal(em.predict(held), lab)
    logw = np.stack([scipy.stats.multivariate_normal(mu_f[k], S_f).logpdf(held) + np.log(pi_f[k]) for k in range(K)], axis=1)
    lse = scipy.special.logsumexp(logw, axis=1)
    assert np.max(np.abs(dens - lse) / np.abs(lse)) < 1e-12
    assert np.max(np.abs(em.predict_proba(held) - np.exp(logw - lse[:, None]))) < 1e-12


def test_tied_weighted_matches_replicated_rows(ctx):
    n, d, K = 400, 5, 3
    X, pi0, mu0, S0 = tied_sample(9, n, d, K)
    w = np.random.default_rng(10).integers(0, 4, n).astype(np.float64)
    rep = _data(ctx, np.repeat(X, w.astype(int), axis=0))
    assert rep.em_tied_route(K) == "kernel"
    ref = rep.em_step_tied(pi0, mu0, S0)
    rep.close()
    dt = _data(ctx, X)
    dt.set_weights(w)
    assert dt.em_tied_route(K) == "composed"
    ll, pi1, mu1, S1 = dt.em_step_tied(pi0, mu0, S0)
    assert abs(ll - ref[0]) <= 1e-12 * abs(ref[0])
    assert relerr(pi1, ref[1]) < 1e-11 and relerr(mu1, ref[2]) < 1e-11 and relerr(S1, ref[3]) < 1e-10
    check_step((ll, pi1, mu1, S1), tied_step(X, pi0, mu0, S0, w))
    dt.set_weights(None)
    assert dt.em_tied_route(K) == "kernel"
    check_step(dt.em_step_tied(pi0, mu0, S0), tied_step(X, pi0, mu0, S0))     # (the total scatter is formed again, unweighted)
    dt.close()


def test_tied_device_group(ctx):
    from ml_amd import _lib
    n, d, K, steps = 1000, 8, 5, 4
    X, pi0, mu0, S0 = tied_sample(21, n, d, K)
    dt = _data(ctx, X)
    one = dt.em_iterate(pi0, mu0, S0, steps, tied=True)
    labels = dt.em_labels(K)
    dt.close()
    group = _lib.Context.group(3, device_ids=[0, 0, 0])
    gd = _lib.Data(group, X)
    assert gd.em_tied_route(K) == "kernel"
    got = gd.em_iterate(pi0, mu0, S0, steps, tied=True)
    assert got[0] == steps and relerr(got[6], one[6]) < 1e-12
    assert relerr(got[3], one[3]) < 1e-11 and relerr(got[4], one[4]) < 1e-11 and relerr(got[5], one[5]) < 1e-10
    assert np.array_equal(gd.em_labels(K), labels)
    ll, pi1, mu1, S1 = gd.em_step_tied(pi0, mu0, S0)
    check_step((ll, pi1, mu1, S1), tied_step(X, pi0, mu0, S0))
    gd.close()
    group.close()


def test_a_tied_step_leaves_the_handle_as_it_found_it(ctx):
    n, d, K = 3000, 8, 5
    X, pi0, mu0, S0 = tied_sample(33, n, d, K)
    full = np.stack([S0] * K)
    dt = _data(ctx, X)
    assert dt.em_tied_route(K) == "kernel"
    first = dt.em_step(pi0, mu0, full)
    dt.em_step_tied(pi0, mu0, S0)
    third = dt.em_step(pi0, mu0, full)
    assert first[0] == third[0] and all(np.array_equal(a, b) for a, b in zip(first[1:], third[1:]))
    km1 = dt.kmeans_step(mu0)
    dt.em_step_tied(pi0, mu0, S0)
    km2 = dt.kmeans_step(mu0)
    assert km1[0] == km2[0] and np.array_equal(km1[2], km2[2]) and np.array_equal(km1[3], km2[3])
    assert km2[1] == 0                                                        # (the labels of the first assignment are still there)
    dt.close()
