"""tests/test_gpu_handle_state.py, continued through every call a data handle has learnt since: row weights, the settable ridge, tied
covariances, restarts, em_score, the conditional calls, weighted K-means and the screened E-step. The rule is that test's rule: ONE
`used` handle runs a list of self-contained calls in order; after each, a `fresh` handle on the same context and the same X runs that
call alone, and every scalar and array the call returns must have the same BITS on both. No tolerance anywhere: the yardstick is the
library itself on a handle without a past, which the extended-precision suites hold to the true value. All differing
"call name [output index]" strings are collected and asserted once at the end of a case.

What outlives a call on a handle (runtime/internal.hpp, mlhip_data and EstepState) and could leak into the
next one: estep.what / kept / screenable, the screened E-step's records and pass history (screen: ScreenState), the statistics
pass's history (stats_history: StatsHistory), total_scatter, km_wfactors_valid / km_colmax, weighted / weight_sum / ridge, rs_kept and
the params_dev / params_next / params_prev ring.

Settings that are MEANT to persist. Weights and ridge are handle settings, not leaks: every compared call declares the weights (None
or a named vector) and the ridge (None: the default) it runs under. The fresh handle is always given them; the used handle only when
they differ from what it has, so consecutive calls under the same settings really run on a handle nobody reset. After every call the
two handles must also agree on weight_sum and covariance_ridge.

A call marked `direct` follows its predecessor with nothing in between; elsewhere an uncompared call (BETWEEN, in rotation) moves
the K-means label history, borrows the log-responsibility block as scratch, resizes the workspace or moves blocks through the
context's pool.

Pinned switches. The self-normalising statistics pass picks its sparse / dense kernel from the handle's call history and the two are
not bit-identical, so MLHIP_MSTATS_SPARSE is pinned on every shape that takes that pass, as in
tests/test_gpu_handle_state.py (d = 72 takes the pass too, but the sparse kernel ends at d = 32: nothing to pin). Screened and dense
E-steps are bit-identical by contract, so MLHIP_ESTEP_SCREEN is a case, not a pin. The one output left out of the comparison is a
K-means step's n_changed: it counts against the labels the last assignment on the handle left, which is what it is for.

Skipped (call, context) pairs: none -- every entry point in the list accepts a device group's context.

The name lists COMPARED / BETWEEN / EXCLUDED at the end are the ledger tests/test_handle_call_ledger.py holds against _lib.Data."""
import time

import numpy as np
import pytest

from test_gpu_estep_screen import mixture, nudged
from test_gpu_handle_state import NO_RESULTS, _mixture, _same

pytestmark = pytest.mark.gpu


# ---- data, starts, weights --------------------------------------------------------------------------------------------------

def _screen_mixture(d, n, seed, K):
    """tests/test_gpu_estep_screen.py's data: unit-covariance clusters 8 standard deviations apart, so that most pairs are screened."""
    X, _, means, _ = mixture(d, K, n, seed)
    return X, means


def _start(X, centres, K, seed):
    """tests/test_gpu_handle_state.py's start: centres with a little noise, the sample's variances on every diagonal."""
    rng = np.random.default_rng(seed)
    mu = centres[np.arange(K) % len(centres)] + 0.1 * rng.standard_normal((K, X.shape[1]))
    var = np.var(X, axis=0)
    return np.full(K, 1.0 / K), mu, np.stack([np.diag(var)] * K), np.stack([var] * K)


def _unit_start(X, centres, K, seed):
    """The same with unit covariances (the clusters' own): the start of the screen shapes."""
    pi, mu, _, _ = _start(X, centres, K, seed)
    d = X.shape[1]
    return pi, mu, np.stack([np.eye(d)] * K), np.ones((K, d))


def _weights(n, seed):
    """w1: frequencies in [0.5, 2) with exact zeros. w2: another draw 2^-70 times as large -- the power-of-two factors of the weighted
    K-means sums (km_wfactors) follow the largest weight, and factors kept from w1 would cut w2's sums off 70 bits too high."""
    rng = np.random.default_rng(seed)
    w1 = rng.uniform(0.5, 2.0, n)
    w1[rng.integers(0, n, n // 20)] = 0.0
    w2 = rng.uniform(0.5, 2.0, n)
    w2[rng.integers(0, n, n // 20)] = 0.0
    return {None: None, "w1": np.ascontiguousarray(w1), "w2": np.ascontiguousarray(np.ldexp(w2, -70))}


def _conditioned(K, d, mu, seed):
    """A mixture over d + 3 coordinates whose first d are the handle's columns, conditioned on those: the arguments of the two
    conditional calls."""
    from ml_amd import _lib
    rng = np.random.default_rng(seed)
    full = d + 3
    means = np.concatenate([mu, rng.standard_normal((K, 3))], axis=1)
    covs = np.empty((K, full, full))
    for k in range(K):
        A = rng.standard_normal((full, full))
        covs[k] = A @ A.T / full + np.eye(full)
    observed = np.arange(d, dtype=np.uint32)
    mu_o, S_oo, maps, mu_m = _lib.em_condition(means, covs, observed)
    _, factors = _lib.em_condition_covariances(covs, observed)
    return mu_o, S_oo, maps, mu_m, factors


# ---- the compared calls -----------------------------------------------------------------------------------------------------

class Call:
    def __init__(self, name, fn, weights=None, ridge=None, direct=False):
        self.name, self.fn, self.weights, self.ridge, self.direct = name, fn, weights, ridge, direct


def _queries(dt, K):
    return [dt.em_labels(K), dt.em_responsibilities(K), *dt.em_maximisation(K), dt.em_labels(K)]


def _flat_restarts(result):
    restarts, best = result
    return [x for r in restarts for x in r] + [best]


def _calls(X, centres, start, Ks, tied_kernel, seed):
    """(name, function of a handle -> list of scalars and arrays, settings) for every K of the shape. tied_kernel: K -> whether a
    tied step of K components on this (unweighted) block is the one-kernel iteration."""
    n, d = X.shape
    calls = []
    for K in Ks:                                    # (the second K: the workspace is resized, scr_K / sn_K start again)
        pi, mu, S, var = start(X, centres, K, 17 + K)
        T = S[0]
        p = (pi, mu, S)
        rng = np.random.default_rng(seed + K)
        # unrelated parameters of the same K: every component somewhere else and tighter, so that a block of theirs calls pairs far
        # that are near under p -- a pass that screened from it would zero responsibilities that are not zero
        other = (np.full(K, 1.0 / K), np.roll(mu, 1, axis=0) + 1.0, S * 0.25)
        R = 3
        starts = [start(X, np.roll(centres, r + 1, axis=0), K, 100 + 7 * r + K) for r in range(R)]
        rs_pi, rs_mu = np.stack([s[0] for s in starts]), np.stack([s[1] for s in starts])
        rs_S, rs_var, rs_T = np.stack([s[2] for s in starts]), np.stack([s[3] for s in starts]), np.stack([s[2][0] for s in starts])
        cond = _conditioned(K, d, mu, seed + 31 * K)
        resp = rng.dirichlet(np.full(K, 0.3), n)

        def add(name, fn, weights=None, ridge=None, direct=False, K=K):
            calls.append(Call("%s K=%d" % (name, K), fn, weights, ridge, direct))

        # full-covariance passes one after the other: the second and third may screen
        def three_steps(dt, K=K, p=p):
            out, q = [], p
            for _ in range(3):
                res = dt.em_step(*q)
                out += res
                q = res[1:]
            return out + _queries(dt, K)
        add("em_step x3 fed back", three_steps)

        # ... and with the queries between two passes of the same K
        def step_queries_step(dt, K=K, p=p):
            return [*dt.em_step(*p), *_queries(dt, K), *dt.em_step(*nudged(*p)), *_queries(dt, K)]
        add("em_step, queries, em_step nudged", step_queries_step)

        # tied covariances: the total scatter is formed by the first kernel step, kept, and formed again after a change of weights
        def tied_step(dt, K=K, pi=pi, mu=mu, T=T):
            return [*dt.em_step_tied(pi, mu, T), *_queries(dt, K)]

        def tied_iterate(dt, K=K, pi=pi, mu=mu, T=T):
            return [*dt.em_iterate(pi, mu, T, 6, 1e-9, 1e-9, tied=True), *_queries(dt, K)]
        add("em_step_tied", tied_step)
        add("em_iterate tied", tied_iterate)
        add("em_step_tied again", tied_step)
        add("em_step_tied", tied_step, weights="w1")
        add("em_step_tied", tied_step, weights="w2")
        add("em_step_tied unweighted again", tied_step)

        def full_step(dt, K=K, p=p):
            return [*dt.em_step(*p), *_queries(dt, K)]

        def full_iterate(dt, K=K, p=p):
            return [*dt.em_iterate(*p, 5), *_queries(dt, K)]
        add("em_step", full_step, weights="w1")
        add("em_maximisation_from", lambda dt, resp=resp: [*dt.em_maximisation_from(resp)], weights="w1")
        add("em_step unweighted after weighted", full_step, direct=True)
        add("em_step", full_step, ridge=1e-3)
        add("em_iterate", full_iterate, ridge=1e-3)
        add("em_step default ridge again", full_step)
        add("em_iterate default ridge again", full_iterate)

        # restarts park and restore the E-step state around every restart
        def restarts_full(dt, K=K, rs_pi=rs_pi, rs_mu=rs_mu, rs_S=rs_S):
            return [*_flat_restarts(dt.em_iterate_restarts(rs_pi, rs_mu, rs_S, 5, 1e-9, 1e-9)), *_queries(dt, K)]

        def restarts_diag(dt, K=K, rs_pi=rs_pi, rs_mu=rs_mu, rs_var=rs_var):
            return [*_flat_restarts(dt.em_iterate_restarts(rs_pi, rs_mu, rs_var, 5, 1e-9, 1e-9, diagonal=True)), *_queries(dt, K)]

        def restarts_tied(dt, K=K, rs_pi=rs_pi, rs_mu=rs_mu, rs_T=rs_T):
            return [*_flat_restarts(dt.em_iterate_restarts(rs_pi, rs_mu, rs_T, 5, 1e-9, 1e-9, tied=True)), *_queries(dt, K)]

        def restarts_then_step(dt, K=K, p=p, rs_pi=rs_pi, rs_mu=rs_mu, rs_S=rs_S):
            # (no query between them: the step meets the state as the restarts put it back)
            return [*_flat_restarts(dt.em_iterate_restarts(rs_pi, rs_mu, rs_S, 5, 1e-9, 1e-9)), *dt.em_step(*p), *_queries(dt, K)]
        add("em_iterate_restarts", restarts_full)
        add("em_iterate_restarts diag", restarts_diag)
        if tied_kernel(K):
            add("em_iterate_restarts tied", restarts_tied)
        add("em_iterate_restarts, em_step", restarts_then_step)
        add("em_step after restarts", full_step, direct=True)

        # scoring must leave the last E-step's results alone, whichever parameters it scores
        def step_score(dt, K=K, p=p, other=other):
            out = [*dt.em_step(*p)]
            for q in (p, other):
                out += [*dt.em_score(*q), dt.em_labels(K), dt.em_responsibilities(K)]
            return out
        add("em_step, em_score", step_score)

        # an E-step of other parameters between two passes of a fit: the block is no longer the one the last pass left
        def expectation_step(dt, K=K, p=p, other=other):
            return [dt.em_expectation(*other), *dt.em_step(*nudged(*p)), *_queries(dt, K)]
        add("em_expectation of other parameters, em_step", expectation_step, direct=True)

        def step_conditional(dt, K=K, p=p, pi=pi, cond=cond):
            mu_o, S_oo, maps, mu_m, factors = cond
            return [*dt.em_step(*p), *dt.em_conditional_means(pi, mu_o, S_oo, maps, mu_m, log_density=True),
                    *dt.em_conditional_samples(pi, mu_o, S_oo, maps, mu_m, factors, n_draws=2, seed=5, labels=True), dt.em_labels(K)]
        add("em_step, conditional calls", step_conditional)
        add("em_step after conditional calls", full_step, direct=True)

        # K-means: the weighted sums' factors follow the weight vector
        def kmeans(dt, mu=mu, weighted=True):
            # (without the step's n_changed: it counts against the labels the LAST assignment on the handle left, by design)
            inertia, _, counts, centroids = dt.kmeans_step(mu, weighted=weighted)
            return [inertia, counts, centroids, dt.kmeans_labels(), dt.kmeans_distances(),
                    *dt.kmeans_iterate(mu, 8, 0.0, weighted=weighted), dt.kmeans_labels(), dt.kmeans_distances()]
        add("kmeans weighted", kmeans, weights="w1")
        add("kmeans weighted", kmeans, weights="w2")
        add("kmeans unweighted", lambda dt, kmeans=kmeans: kmeans(dt, weighted=False))
        add("kmeans weighted again", kmeans, weights="w1")
        add("em_step after K-means, weighted", full_step, weights="w1", direct=True)

        # diagonal and tied one-kernel passes straight after each other: the kept records change their mode
        def diag_step(dt, K=K, pi=pi, mu=mu, var=var):
            return [*dt.em_step_diag(pi, mu, var), *_queries(dt, K)]

        def diag_iterate(dt, K=K, pi=pi, mu=mu, var=var):
            return [*dt.em_iterate(pi, mu, var, 6, 1e-9, 1e-9, diagonal=True), *_queries(dt, K)]
        add("em_step_tied before diagonal", tied_step)
        add("em_step_diag after tied", diag_step, direct=True)
        add("em_step_tied after diagonal", tied_step, direct=True)
        add("em_iterate diag after tied", diag_iterate, direct=True)
        add("em_iterate tied after diagonal", tied_iterate, direct=True)
        add("em_step after tied", full_step, direct=True)
    return calls


def _between(dt, ctx, X, centres, start, K, i):
    """Calls whose results are not compared, made between the compared ones, in rotation."""
    kind = i % 7
    if kind == 0:
        dt.min_squared_distances(centres[:2])
    elif kind == 1:
        dt.kmeans_assign(centres[:4])
    elif kind == 2:
        dt.em_maximisation_from_labels(np.arange(len(X), dtype=np.uint32) % 2, 2)
        with pytest.raises(ValueError, match=NO_RESULTS):
            dt.em_labels(2)
    elif kind == 3:
        dt.sample_covariance()                      # (it borrowed the block of the last E-step)
        with pytest.raises(ValueError, match=NO_RESULTS):
            dt.em_labels(1)
    elif kind == 4:
        dt.em_score(*start(X, centres, K + 1, 300 + i)[:3])
    elif kind == 5:
        ctx.em_sample(*start(X, centres, K, 400 + i)[:3], 500, seed=i)      # (blocks move through the context's pool)
    else:
        try:
            dt.em_responsibilities_rows(K, 7, 100)
        except ValueError as e:                     # (only where results exist)
            assert NO_RESULTS in str(e)


def _bits(a, b):
    """Equal bits: scalars through their float64 bytes, arrays with np.array_equal (NaNs equal)."""
    if np.ndim(a) == 0 and np.ndim(b) == 0:
        return np.float64(a).tobytes() == np.float64(b).tobytes()
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and _same(a, b)


def _apply(dt, weights, ridge, W):
    from ml_amd import _lib
    dt.set_weights(W[weights])
    dt.set_covariance_ridge(_lib.DEFAULT_COVARIANCE_RIDGE if ridge is None else ridge)


def _subset(route, want):
    got = {k: route[k] for k in want}
    assert got == want, (got, want)


SCREEN_ON = {"MLHIP_ESTEP_SCREEN": "1", "MLHIP_MSTATS_SPARSE": "1"}
FOLD_SELF_NORM = {"estep": "matrix4", "fold_allowed": True, "fused": False, "self_norm": True}
SHAPES = {
    # name: (screen data?, d, N, component counts, switches, the route of the first K the shape is written for, its K-means kernel)
    "screen-forced":  (True, 16, 3001, (8, 5), SCREEN_ON, dict(FOLD_SELF_NORM, sparse=True), None),
    "screen-forced-dense-stats": (True, 24, 2001, (6,), {"MLHIP_ESTEP_SCREEN": "1", "MLHIP_MSTATS_SPARSE": "0"}, dict(FOLD_SELF_NORM, sparse=False), None),
    "screen-auto":    (True, 32, 2001, (64,), {"MLHIP_MSTATS_SPARSE": "1"}, dict(FOLD_SELF_NORM, sparse=True), None),
    "screen-off":     (True, 16, 3001, (8, 5), {"MLHIP_ESTEP_SCREEN": "0", "MLHIP_MSTATS_SPARSE": "1"}, dict(FOLD_SELF_NORM, sparse=True), None),
    "fused":          (False, 6, 3001, (8, 3), {}, {"fused": True, "fused_form": "lds_feed", "device_close": True}, "direct"),
    "resident":       (False, 2, 3001, (3, 5), {}, {"fused": True, "fused_form": "valu", "device_close": True}, "direct"),
    "scalar-fed":     (False, 8, 3001, (5, 12), {"MLHIP_FUSED": "0"}, {"estep": "scalar_fed", "fused": False, "self_norm": False}, None),
    "panelled":       (False, 72, 1501, (2,), {}, {"estep": "matrix4", "fused": False, "device_close": True, "records_on_device": True}, "matrix"),
}


@pytest.fixture(scope="module", params=["single", "group3"])
def ctx(request):
    from ml_amd import _lib
    c = _lib.Context() if request.param == "single" else _lib.Context.group(3, device_ids=[0, 0, 0])
    c.kind = request.param
    yield c
    c.close()


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_a_call_returns_what_it_returns_on_a_fresh_handle(ctx, monkeypatch, shape):
    from ml_amd import _lib
    t0 = time.perf_counter()
    screen_data, d, n, Ks, switches, route, km_kernel = SHAPES[shape]
    for name, value in switches.items():
        monkeypatch.setenv(name, value)
    if screen_data:
        X, centres = _screen_mixture(d, n, 2000 + d, Ks[0])
        start = _unit_start
    else:
        X, centres = _mixture(d, n, 2000 + d)
        start = _start
    W = _weights(n, 3000 + d)
    used = _lib.Data(ctx, X)
    # the route the shape is written for, once (the one-launch loop exists on a single rank only)
    _subset(used.em_route(Ks[0]), route)
    if shape == "resident":
        assert used.em_route(Ks[0])["resident"] == (ctx.kind == "single")
        assert used.em_route(Ks[0], "diag")["diag_kernel"]
    if shape == "fused":
        assert used.em_tied_route(Ks[0]) == "kernel"
    if km_kernel:
        assert used.kmeans_route(Ks[0])["kernel"] == km_kernel
    calls = _calls(X, centres, start, Ks, lambda K: used.em_tied_route(K) == "kernel", 4000 + d)
    with pytest.raises(ValueError, match=NO_RESULTS):
        used.em_labels(Ks[0])
    have = (None, None)
    differing = []
    for i, c in enumerate(calls):
        K = int(c.name.rsplit("=", 1)[1])
        if i and not c.direct:
            _between(used, ctx, X, centres, start, K, i)
        if c.weights != have[0]:
            used.set_weights(W[c.weights])
        if c.ridge != have[1]:
            used.set_covariance_ridge(_lib.DEFAULT_COVARIANCE_RIDGE if c.ridge is None else c.ridge)
        have = (c.weights, c.ridge)
        got = c.fn(used) + [used.weight_sum, used.covariance_ridge]
        fresh = _lib.Data(ctx, X)
        _apply(fresh, c.weights, c.ridge, W)
        want = c.fn(fresh) + [fresh.weight_sum, fresh.covariance_ridge]
        fresh.close()
        assert len(got) == len(want)
        label = "%s [weights %s, ridge %s]" % (c.name, c.weights, c.ridge)
        differing += ["%s [%d]" % (label, j) for j, (a, b) in enumerate(zip(got, want)) if not _bits(a, b)]
    counts = used.em_screen_counts()
    used.close()
    print("\n%s on %s: %d compared calls, %.2f s, screen counts %s" % (shape, ctx.kind, len(calls), time.perf_counter() - t0, counts))
    assert not differing, differing
    # (a group's counts are summed over its shards)
    if shape == "screen-forced":
        assert counts["screened"] >= 4, counts      # otherwise the chain could pass without ever screening
    if shape == "screen-off":
        assert counts["screened"] == 0, counts


# ---- the ledger: every public name of _lib.Data is in exactly one of these (tests/test_handle_call_ledger.py) -------------------

COMPARED = [
    "set_weights", "weight_sum", "set_covariance_ridge", "covariance_ridge",
    "em_step", "em_step_diag", "em_step_tied", "em_iterate", "em_iterate_restarts", "em_expectation", "em_maximisation",
    "em_maximisation_from", "em_responsibilities", "em_labels", "em_score", "em_conditional_means", "em_conditional_samples",
    "kmeans_step", "kmeans_iterate", "kmeans_labels", "kmeans_distances",
]
BETWEEN = ["min_squared_distances", "kmeans_assign", "em_maximisation_from_labels", "sample_covariance", "em_responsibilities_rows"]
EXCLUDED = {
    "close": "ends the handle: nothing follows it",
    "adopt": "a constructor (Context.em_sample_data's block), not a call on a handle",
    "handle": "the raw pointer, no device work",
    "n_global": "a constant of the upload",
    "shard_rows": "a constant of the upload",
    "shift": "a constant of the upload",
    "em_route": "a query of the shape and the switches, reads no call history",
    "em_plan": "a query of the shape and the switches, reads no call history",
    "em_tied_route": "a query of the shape, the switches and the weights setting",
    "em_restarts_route": "a query of the shape, the switches and the weights setting",
    "em_score_route": "a query of the shape and the switches",
    "em_condition_route": "a query of the shape and the switches",
    "em_conditional_sample_route": "a query of the shape and the switches",
    "kmeans_route": "a query of the shape and the switches",
    "em_screen_counts": "reports the call history on purpose: asserted at the end of the chain instead",
}
