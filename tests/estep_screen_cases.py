"""Data and the screened-against-dense comparison shared by the tests of the screened E-step's tile forms (not a test module).
A case runs the same passes with MLHIP_ESTEP_SCREEN=1 and =0 on fresh handles -- the given parameters twice, then a small step away --
and compares, bit for bit, everything em_step returns, the responsibilities and the labels; it returns the screened run's route counts
(Data.em_screen_counts; 'candidates' is the last screened pass's count) for the caller to assert."""
import os

import numpy as np


def set_screen(mode):
    """MLHIP_ESTEP_SCREEN for the calls that follow (read per call by the runtime); None: unset."""
    if mode is None:
        os.environ.pop("MLHIP_ESTEP_SCREEN", None)
    else:
        os.environ["MLHIP_ESTEP_SCREEN"] = mode


def bits(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64)).tobytes()


def same(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert bits(u) == bits(v)


def mixture(d, K, n, seed, spread=8.0):
    """n rows of K unit-covariance clusters `spread` apart, and the mixture's own parameters."""
    rng = np.random.default_rng(seed)
    means = spread * rng.standard_normal((K, d))
    X = np.ascontiguousarray(means[rng.integers(0, K, n)] + rng.standard_normal((n, d)))
    return X, (np.full(K, 1.0 / K), means, np.stack([np.eye(d)] * K))


def placed(means, comp, seed):
    """One row per entry of `comp`, a unit-variance draw around that component's mean; unit covariances, equal weights."""
    K, d = means.shape
    rng = np.random.default_rng(seed)
    X = np.ascontiguousarray(means[comp] + rng.standard_normal((len(comp), d)))
    return X, (np.full(K, 1.0 / K), means, np.stack([np.eye(d)] * K))


def axis_means(K, d):
    """K means 40 standard deviations out on the axes (+ e_j, then - e_j): 56 or 80 apart, so that a row's only candidate is the
    component it was drawn from (and whatever coincides with it)."""
    assert K <= 2 * d
    m = np.zeros((K, d))
    for k in range(K):
        m[k, k % d] = 40.0 if k < d else -40.0
    return m


def nudged(p, eps=1e-3):
    """Parameters a small step away: every bound constant changes, none loses its information."""
    return p[0], p[1] + eps, p[2] * (1.0 + eps)


def three_passes(p):
    return [p, p, nudged(p)]


def run_passes(ctx, mode, X, params):
    """One em_step per parameter set on one handle: the results and the route counts after every pass, then responsibilities, labels."""
    from ml_amd import _lib
    set_screen(mode)
    dt = _lib.Data(ctx, X)
    outs, trail = [], []
    for p in params:
        outs.append(dt.em_step(*p))
        trail.append(dt.em_screen_counts())
    K = len(params[0][0])
    resp, labels = dt.em_responsibilities(K), dt.em_labels(K)
    dt.close()
    return outs, resp, labels, trail


def both(ctx, X, params, shards=1):
    """The passes screened and dense; equal bits everywhere. Returns the screened run's counts after every pass (a device group's
    are summed over its shards)."""
    on = run_passes(ctx, "1", X, params)
    off = run_passes(ctx, "0", X, params)
    for a, b in zip(on[0], off[0]):
        same(a, b)
    assert bits(on[1]) == bits(off[1])
    assert np.array_equal(on[2], off[2])
    for t, c in enumerate(off[3]):
        assert c == {"screened": 0, "dense": shards * (t + 1), "no_information": 0, "candidates": 0}
    return on[3]


def routes(trail):
    return [(c["screened"], c["dense"], c["no_information"]) for c in trail]


THREE = [(0, 1, 0), (1, 1, 0), (2, 1, 0)]
