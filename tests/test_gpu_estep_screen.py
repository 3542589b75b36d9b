"""The screened E-step (device/em_estep_screen.hip) against the dense one it stands in for: MLHIP_ESTEP_SCREEN=1 must give, bit for
bit, what MLHIP_ESTEP_SCREEN=0 gives on everything mlhip_em_step / mlhip_em_iterate return and on responsibilities and labels -- a
pair the screen does not evaluate has a responsibility of exactly 0.0 either way, a pair it evaluates gets the dense kernel's bits.
Every case also asserts the route it expects (Data.em_screen_counts): the first pass on a handle is dense (there is no block to
start from), a later pass of the kernel's domain (full covariances, FOLD form, 12 <= d <= 32, K <= 64, no row weights) is screened
unless a component's bound carries no information -- then the dense kernel runs and the pass is counted under 'no_information'."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from ml_amd import _lib
    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture
def screen():
    old = os.environ.get("MLHIP_ESTEP_SCREEN")

    def set_mode(m):
        if m is None:
            os.environ.pop("MLHIP_ESTEP_SCREEN", None)
        else:
            os.environ["MLHIP_ESTEP_SCREEN"] = m
    yield set_mode
    set_mode(old)


def bits(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64)).tobytes()


def same(a, b):
    """Two results of em_step / em_iterate (tuples of scalars and arrays), bit for bit (NaNs included)."""
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert bits(u) == bits(v)


def mixture(d, K, n, seed, spread=8.0):
    """n rows of K unit-covariance clusters `spread` apart; the parameters of the mixture itself."""
    rng = np.random.default_rng(seed)
    means = spread * rng.standard_normal((K, d))
    comp = rng.integers(0, K, n)
    X = np.ascontiguousarray(means[comp] + rng.standard_normal((n, d)))
    return X, np.full(K, 1.0 / K), means, np.stack([np.eye(d)] * K)


def nudged(pi, mu, S, eps=1e-3):
    """Parameters a small step away: every bound constant changes, none loses its information."""
    return pi, mu + eps, S * (1.0 + eps)


def run_steps(ctx, screen, mode, X, params, weights=None):
    """One em_step per parameter set of `params` on one handle; every pass's results, then responsibilities, labels, counts."""
    from ml_amd import _lib
    screen(mode)
    dt = _lib.Data(ctx, X)
    if weights is not None:
        dt.set_weights(weights)
    outs = [dt.em_step(*p) for p in params]
    K = len(params[0][0])
    resp, labels, counts = dt.em_responsibilities(K), dt.em_labels(K), dt.em_screen_counts()
    dt.close()
    return outs, resp, labels, counts


def both(ctx, screen, X, params, weights=None):
    """The same passes with the screen forced on and off; asserts equal bits everywhere, returns (counts of '1', counts of '0')."""
    on = run_steps(ctx, screen, "1", X, params, weights)
    off = run_steps(ctx, screen, "0", X, params, weights)
    for a, b in zip(on[0], off[0]):
        same(a, b)
    assert bits(on[1]) == bits(off[1])
    assert np.array_equal(on[2], off[2])
    assert off[3]["screened"] == 0 and off[3]["no_information"] == 0
    return on[3], off[3]


def three_passes(p):
    """The given parameters twice (the second pass starts from the first one's block), then a small step away."""
    return [p, p, nudged(*p)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 3000, 100_000])
def test_row_counts(ctx, screen, n):
    # 100 000 rows: more 128-sample tiles than resident workgroups, every workgroup's tile loop goes round
    d, K = (12, 3) if n == 100_000 else (32, 5)
    X, pi, mu, S = mixture(d, K, n, seed=n)
    on, _ = both(ctx, screen, X, three_passes((pi, mu, S)))
    assert (on["screened"], on["dense"], on["no_information"]) == (2, 1, 0)
    assert n <= on["candidates"] <= K * n


@pytest.mark.parametrize("d", [12, 21, 24, 32])
@pytest.mark.parametrize("K", [1, 3, 63, 64])
def test_shapes(ctx, screen, d, K):
    X, pi, mu, S = mixture(d, K, 700, seed=100 * d + K)
    on, _ = both(ctx, screen, X, three_passes((pi, mu, S)))
    assert (on["screened"], on["dense"], on["no_information"]) == (2, 1, 0)


def test_bucket_sizes(ctx, screen):
    """Clusters 40 standard deviations out on the axes, so a sample's only candidate is its own component: in the first 128-sample tile the buckets of
    components 0 .. 6 hold 1, 15, 16, 17, 33, 46 and 0 samples (no group, one partly filled, one full, two, three), in the second
    tile component 6 holds all 128 and the others none."""
    d, K = 12, 7
    sizes = [1, 15, 16, 17, 33, 46, 0]
    comp = np.concatenate([np.repeat(np.arange(K), sizes), np.full(128, 6)])
    rng = np.random.default_rng(7)
    comp[:128] = rng.permutation(comp[:128])
    means = 40.0 * np.eye(K, d)
    X = np.ascontiguousarray(means[comp] + rng.standard_normal((256, d)))
    on, _ = both(ctx, screen, X, three_passes((np.full(K, 1.0 / K), means, np.stack([np.eye(d)] * K))))
    assert (on["screened"], on["dense"], on["no_information"]) == (2, 1, 0)
    assert on["candidates"] == 256


def test_every_component_a_candidate(ctx, screen):
    # two coincident components: every sample keeps both
    d, n = 12, 300
    X, _, mu, _ = mixture(d, 1, n, seed=11)
    p = (np.array([0.5, 0.5]), np.vstack([mu, mu]), np.stack([np.eye(d)] * 2))
    on, _ = both(ctx, screen, X, three_passes(p))
    assert (on["screened"], on["dense"], on["no_information"]) == (2, 1, 0)
    assert on["candidates"] == 2 * n


def test_mixing_weight_zero(ctx, screen):
    # log 0 in a record: that component's bound carries no information, every later pass is sent back to the dense kernel
    X, pi, mu, S = mixture(16, 4, 500, seed=13)
    pi = np.array([0.0, 0.5, 0.25, 0.25])
    on, _ = both(ctx, screen, X, three_passes((pi, mu, S)))
    assert (on["screened"], on["dense"], on["no_information"]) == (0, 3, 2)


def test_far_rows_and_empty_component(ctx, screen):
    # rows hundreds of standard deviations from every component (stored values of -1e5 and below), and a component whose start is
    # far from every row: none of its pairs is a candidate, except on rows for which it gives the largest lower bound
    X, pi, mu, S = mixture(24, 6, 1000, seed=17)
    X[::97] += 400.0
    X[5] += 4.0e5                      # |lw| beyond 2^40: never bounded from (two rows, so that the data's centre stays put)
    X[6] -= 4.0e5
    mu = mu.copy()
    mu[0] = 50.0
    on, _ = both(ctx, screen, X, three_passes((pi, mu, S)))
    assert (on["screened"], on["dense"], on["no_information"]) == (2, 1, 0)


def test_drifting_fit(ctx, screen):
    """Twelve passes of a fit from a perturbed start, each pass fed with the last one's result and compared. The passes whose step is
    too large for the bound run dense and are counted; from the second half on the fit moves little and every pass is screened."""
    from ml_amd import _lib
    d, K, n = 16, 8, 3000
    X, pi, mu, S = mixture(d, K, n, seed=19, spread=5.0)
    rng = np.random.default_rng(23)
    start = (pi, mu + 0.3 * rng.standard_normal(mu.shape), S)
    runs = {}
    for m in ("1", "0"):
        screen(m)
        dt = _lib.Data(ctx, X)
        p, outs, trail = start, [], []
        for _ in range(12):
            out = dt.em_step(*p)
            outs.append(out)
            trail.append(dt.em_screen_counts())
            p = out[1:]
        runs[m] = (outs, dt.em_responsibilities(K), dt.em_labels(K), trail)
        dt.close()
    for a, b in zip(runs["1"][0], runs["0"][0]):
        same(a, b)
    assert bits(runs["1"][1]) == bits(runs["0"][1])
    assert np.array_equal(runs["1"][2], runs["0"][2])
    trail = runs["1"][3]
    assert trail[0]["screened"] == 0 and trail[0]["dense"] == 1
    assert trail[-1]["screened"] + trail[-1]["dense"] == 12
    assert trail[-1]["screened"] - trail[5]["screened"] == 6            # passes 7 .. 12
    assert runs["0"][3][-1] == {"screened": 0, "dense": 12, "no_information": 0, "candidates": 0}


def test_unrelated_parameters_fall_back(ctx, screen):
    X, pi, mu, S = mixture(32, 6, 900, seed=29)
    rng = np.random.default_rng(31)
    other = (pi, rng.permutation(mu) + 1.0, S * 9.0)
    on, _ = both(ctx, screen, X, [(pi, mu, S), (pi, mu, S), other, other])
    # pass 3 cannot be bounded from pass 2's block; pass 4 starts from pass 3's dense block
    assert (on["screened"], on["dense"], on["no_information"]) == (2, 2, 1)


def test_fold_rejected(ctx, screen):
    # components 1000 standard deviations from the data's centre: the E-step takes its exact form, which is never screened
    d, K = 16, 2
    rng = np.random.default_rng(37)
    means = np.zeros((K, d))
    means[0, 0], means[1, 0] = -1000.0, 1000.0
    X = np.ascontiguousarray(means[rng.integers(0, K, 600)] + rng.standard_normal((600, d)))
    on, _ = both(ctx, screen, X, three_passes((np.full(K, 0.5), means, np.stack([np.eye(d)] * K))))
    assert (on["screened"], on["dense"], on["no_information"]) == (0, 0, 0)


def test_row_weights(ctx, screen):
    X, pi, mu, S = mixture(16, 5, 800, seed=41)
    w = np.random.default_rng(43).uniform(0.5, 2.0, 800)
    on, _ = both(ctx, screen, X, three_passes((pi, mu, S)), weights=w)
    assert (on["screened"], on["dense"], on["no_information"]) == (0, 0, 0)


def test_two_shard_group(ctx, screen):
    from ml_amd import _lib
    X, pi, mu, S = mixture(24, 6, 1500, seed=47)
    grp = _lib.Context.group(2, device_ids=[0, 0])
    try:
        on, _ = both(grp, screen, X, three_passes((pi, mu, S)))
    finally:
        grp.close()
    assert (on["screened"], on["dense"], on["no_information"]) == (4, 2, 0)   # summed over the shards
    single = run_steps(ctx, screen, "1", X, three_passes((pi, mu, S)))
    assert on["candidates"] == single[3]["candidates"]


def test_iterate_screened(ctx, screen):
    """mlhip_em_iterate at a size whose loop waits for every iteration (the FOLD form, the screened kernel's domain): eight
    iterations; then labels and responsibilities from the block the last, screened pass left."""
    from ml_amd import _lib
    d, K, n = 32, 64, 40_000
    X, pi, mu, S = mixture(d, K, n, seed=53)
    res = {}
    for m in ("1", "0"):
        screen(m)
        dt = _lib.Data(ctx, X)
        first = dt.em_iterate(pi, mu, S, 3)
        second = dt.em_iterate(first[3], first[4], first[5], 5)       # (starts from the block the first call left)
        res[m] = (first, second, dt.em_responsibilities(K), dt.em_labels(K), dt.em_screen_counts())
        dt.close()
    same(res["1"][0], res["0"][0])
    same(res["1"][1], res["0"][1])
    assert bits(res["1"][2]) == bits(res["0"][2])
    assert np.array_equal(res["1"][3], res["0"][3])
    on = res["1"][4]
    assert on["screened"] + on["dense"] == 8 and on["dense"] >= 1
    assert on["screened"] >= 5                                        # every pass of the second call
    assert n <= on["candidates"] <= 16 * n


def test_iterate_ending_by_tolerance(ctx, screen):
    """A small fit: mlhip_em_iterate runs one iteration ahead of its convergence test, in the E-step's exact form -- never screened --,
    and the speculative pass overwrites the block. The steps that follow on the same handle start from a block of their own."""
    from ml_amd import _lib
    X, pi, mu, S = mixture(16, 4, 2000, seed=59)
    res = {}
    for m in ("1", "0"):
        screen(m)
        dt = _lib.Data(ctx, X)
        fit = dt.em_iterate(pi, mu, S, 50, 0.0, 1e-9)
        labels = dt.em_labels(4)
        after_fit = dt.em_screen_counts()
        p = fit[3:6]
        steps = [dt.em_step(*p), dt.em_step(*p)]
        res[m] = (fit, labels, steps, after_fit, dt.em_screen_counts())
        dt.close()
    assert res["1"][0][1] and res["1"][0][0] < 50                     # converged before the step limit
    same(res["1"][0], res["0"][0])
    assert np.array_equal(res["1"][1], res["0"][1])
    for a, b in zip(res["1"][2], res["0"][2]):
        same(a, b)
    assert res["1"][3]["screened"] == 0 and res["1"][3]["dense"] == 0
    assert (res["1"][4]["screened"], res["1"][4]["dense"]) == (1, 1)


@pytest.mark.parametrize("d,K,expected", [(32, 64, 3), (32, 32, 0), (32, 16, 0), (24, 64, 0)])
def test_automatic_route(ctx, screen, d, K, expected):
    """Without the switch: the first two passes on a handle are dense (the rule reads the counts of pass t - 2), later ones are screened
    at the shape where that was measured faster on repeated runs (D = 32, K = 64) and dense elsewhere; the results are those of the dense kernel."""
    X, pi, mu, S = mixture(d, K, 2000, seed=61 + d + K)
    auto = run_steps(ctx, screen, None, X, [(pi, mu, S)] * 5)
    off = run_steps(ctx, screen, "0", X, [(pi, mu, S)] * 5)
    for a, b in zip(auto[0], off[0]):
        same(a, b)
    assert bits(auto[1]) == bits(off[1])
    assert np.array_equal(auto[2], off[2])
    assert (auto[3]["screened"], auto[3]["dense"], auto[3]["no_information"]) == (expected, 5 - expected, 0)
