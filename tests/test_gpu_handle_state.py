"""What a call leaves on a data handle (runtime/internal.hpp EstepState: nothing / the N x K block / full records only / diagonal
records only; the K-means label history; the workspace sized for the last K) must not leak into the next call: ONE handle is driven
through every transition -- resident, lagged and synchronous mlhip_em_iterate, fused and two-kernel mlhip_em_step, diagonal steps
and loops, the refinement pass, a change of K, calls that borrow the block as scratch, K-means in between -- and each self-contained
call (em_step, em_step_diag, em_iterate, kmeans_iterate, sample_covariance) with the queries that follow it returns the same BITS as
on a fresh handle given only that call. tests/test_gpu_pool.py checks this across handles; this one within a handle.

The self-normalising statistics pass picks its sparse / dense kernel from the handle's call history, so shapes
that take it run with MLHIP_MSTATS_SPARSE forced to 0 and to 1."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NO_RESULTS = "no E-step results on the device for this K"


def _mixture(d, n, seed):
    rng = np.random.default_rng(seed)
    centres = 3.0 * rng.standard_normal((8, d))
    X = np.ascontiguousarray(centres[rng.integers(0, 8, n)] + rng.standard_normal((n, d)) + 5.0)
    return X, centres + 5.0


def _far_tight(d, n, seed):
    """A component 300 units from the origin with sigma 1e-3 (tests/test_gpu_iterate.py): flagged for the refinement pass."""
    rng = np.random.default_rng(seed)
    centres = np.array([[0.0] * d, [300.0] * d, [-200.0] * d])
    sig = np.array([1.0, 1e-3, 1e-2])
    comp = rng.integers(0, 3, n)
    X = np.ascontiguousarray(centres[comp] + rng.standard_normal((n, d)) * sig[comp][:, None])
    return X, centres


def _start(X, centres, K, seed):
    rng = np.random.default_rng(seed)
    mu = centres[np.arange(K) % len(centres)] + 0.1 * rng.standard_normal((K, X.shape[1]))
    var = np.var(X, axis=0)
    return np.full(K, 1.0 / K), mu, np.stack([np.diag(var)] * K), np.stack([var] * K)


def _far_start(X, centres, K, seed):
    assert K == 3
    d = X.shape[1]
    sig = np.array([1.0, 1e-3, 1e-2])
    mu = centres + 0.1 * sig[:, None] * np.random.default_rng(seed).standard_normal((3, d))
    var = np.repeat((sig ** 2)[:, None], d, axis=1) * 1.5
    return np.full(3, 1.0 / 3), mu, np.stack([np.diag(v) for v in var]), var


def _queries(dt, K):
    return [dt.em_labels(K), dt.em_responsibilities(K), *dt.em_maximisation(K), dt.em_labels(K)]


def _calls(X, centres, start, Ks):
    """The self-contained calls, each with the queries that follow it: (name, function of a handle -> list of arrays)."""
    calls = []

    def add(name, fn):
        calls.append((name, fn))

    for K in Ks:                                    # (the second K: the workspace is resized on the same handle)
        pi, mu, S, var = start(X, centres, K, 17 + K)
        add("em_iterate K=%d" % K, lambda dt, K=K, pi=pi, mu=mu, S=S: [*dt.em_iterate(pi, mu, S, 10, 1e-9, 1e-9), *_queries(dt, K)])
        add("em_step K=%d" % K, lambda dt, K=K, pi=pi, mu=mu, S=S: [*dt.em_step(pi, mu, S), *_queries(dt, K)])
        add("em_iterate one step K=%d" % K, lambda dt, K=K, pi=pi, mu=mu, S=S: [*dt.em_iterate(pi, mu, S, 1), *_queries(dt, K)])
        add("sample_covariance", lambda dt: [*dt.sample_covariance()])
        add("em_step_diag K=%d" % K, lambda dt, K=K, pi=pi, mu=mu, var=var, S=S:
            [*dt.em_step_diag(pi, mu, var), dt.em_labels(K), *dt.em_step(pi, mu, S), dt.em_labels(K)])
        add("kmeans_iterate K=%d" % K, lambda dt, mu=mu: [*dt.kmeans_iterate(mu, 12, 0.0), dt.kmeans_labels(), dt.kmeans_distances()])
        add("em_iterate diag K=%d" % K, lambda dt, K=K, pi=pi, mu=mu, var=var:
            [*dt.em_iterate(pi, mu, var, 8, 1e-9, 1e-9, True), dt.em_labels(K), dt.em_responsibilities(K)])
        add("em_iterate exact steps K=%d" % K, lambda dt, K=K, pi=pi, mu=mu, S=S: [*dt.em_iterate(pi, mu, S, 4), *_queries(dt, K)])
        add("em_step_diag then queries K=%d" % K, lambda dt, K=K, pi=pi, mu=mu, var=var: [*dt.em_step_diag(pi, mu, var), *_queries(dt, K)])
        add("em_step again K=%d" % K, lambda dt, K=K, pi=pi, mu=mu, S=S: [*dt.em_step(pi, mu, S), dt.em_responsibilities(K)])
    return calls


def _between(dt, X, centres, i):
    """Calls whose results are not compared, made between the compared ones: they move the K-means label history, borrow the
    log-responsibility block as scratch, or resize the workspace."""
    if i % 3 == 0:
        dt.min_squared_distances(centres[:2])
        dt.kmeans_step(centres[:3])
    elif i % 3 == 1:
        dt.em_maximisation_from_labels(np.arange(len(X), dtype=np.uint32) % 2, 2)
        with pytest.raises(ValueError, match=NO_RESULTS):
            dt.em_labels(2)
    else:
        dt.kmeans_assign(centres[:4])


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


SHAPES = {
    # name: (data, start parameters, d, N, component counts, switches)
    "resident":        (_mixture, _start, 2, 12000, (3, 5), {}),                         # d = 2, K = 3: the whole loop in one launch
    "launched":        (_mixture, _start, 2, 12000, (3, 5), {"MLHIP_RESIDENT": "0"}),    # ... as the lagged loop of fused steps
    "fused-refined":   (_far_tight, _far_start, 4, 24000, (3,), {}),                     # refinement after a fused step, inside the loops
    "fused-refined-launched": (_far_tight, _far_start, 4, 24000, (3,), {"MLHIP_RESIDENT": "0"}),
    "matrix-dense":    (_mixture, _start, 16, 20000, (8, 5), {"MLHIP_MSTATS_SPARSE": "0"}),   # matrix-core E-step, self-normalising
    "matrix-sparse":   (_mixture, _start, 16, 20000, (8, 5), {"MLHIP_MSTATS_SPARSE": "1"}),   # statistics, lagged loop
    "matrix-refined":  (_far_tight, _far_start, 12, 24000, (3,), {"MLHIP_MSTATS_SPARSE": "0"}),   # synchronous loop, host closing
    "scalar-fed":      (_mixture, _start, 8, 9000, (5, 12), {}),                         # scalar-fed E-step + wide statistics kernel
}


@pytest.fixture(scope="module", params=["single", "group3"])
def ctx(request):
    from ml_amd import _lib
    c = _lib.Context() if request.param == "single" else _lib.Context.group(3, device_ids=[0, 0, 0])
    yield c
    c.close()


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_results_do_not_depend_on_what_the_handle_did_before(ctx, monkeypatch, shape):
    from ml_amd import _lib
    data, start, d, n, Ks, switches = SHAPES[shape]
    for name, value in switches.items():
        monkeypatch.setenv(name, value)
    X, centres = data(d, n, 1000 + d)
    calls = _calls(X, centres, start, Ks)
    used = _lib.Data(ctx, X)
    with pytest.raises(ValueError, match=NO_RESULTS):
        used.em_labels(Ks[0])
    differing = []
    for i, (name, call) in enumerate(calls):
        got = call(used)
        fresh = _lib.Data(ctx, X)
        want = call(fresh)
        fresh.close()
        assert len(got) == len(want)
        differing += ["%s [%d]" % (name, j) for j, (a, b) in enumerate(zip(got, want)) if not _same(a, b)]
        if name == "sample_covariance":             # it borrowed the block of the last E-step
            with pytest.raises(ValueError, match=NO_RESULTS):
                used.em_labels(1)
        _between(used, X, centres, i)
    used.close()
    assert not differing, differing
