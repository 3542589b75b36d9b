"""The screened E-step's tile structure (device/em_estep_screen.hip: 256 samples per tile, two threads per sample -- components
0 .. 31 and 32 .. 63 --, four 64-sample segments per component's bucket, eight waves that take the components w, w + 8, ...) at the
smallest shapes where each piece of it can go wrong. Every case runs the same passes with MLHIP_ESTEP_SCREEN=1 and =0 on fresh handles
-- the given parameters twice, then a small step away -- and compares, bit for bit, everything em_step returns, the responsibilities
and the labels, and asserts the route counts it expects (Data.em_screen_counts; 'candidates' is the last screened pass's count)."""
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


def run_passes(ctx, screen, mode, X, params):
    """One em_step per parameter set on one handle: the results and the route counts after every pass, then responsibilities, labels."""
    from ml_amd import _lib
    screen(mode)
    dt = _lib.Data(ctx, X)
    outs, trail = [], []
    for p in params:
        outs.append(dt.em_step(*p))
        trail.append(dt.em_screen_counts())
    K = len(params[0][0])
    resp, labels = dt.em_responsibilities(K), dt.em_labels(K)
    dt.close()
    return outs, resp, labels, trail


def both(ctx, screen, X, params, shards=1):
    """The passes screened and dense; equal bits everywhere. Returns the screened run's counts after every pass (a device group's
    are summed over its shards)."""
    on = run_passes(ctx, screen, "1", X, params)
    off = run_passes(ctx, screen, "0", X, params)
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


@pytest.mark.parametrize("n,d,K", [(257, 32, 5), (511, 32, 5), (512, 32, 5), (513, 32, 5), (70_000, 12, 3)])
def test_tile_edges(ctx, screen, n, d, K):
    # one row into the second tile, one short of two tiles, two whole tiles, one row into the third; 70 000 rows are 274 tiles: some
    # workgroups take two tiles (the second one staged from the loads issued under the first), most take one
    X, p = mixture(d, K, n, seed=n)
    trail = both(ctx, screen, X, three_passes(p))
    assert routes(trail) == THREE
    assert n <= trail[-1]["candidates"] <= K * n


@pytest.mark.parametrize("d", [12, 32])
@pytest.mark.parametrize("K", [1, 7, 8, 9, 15, 17, 31, 32, 33, 40, 63, 64])
def test_components_against_waves_and_halves(ctx, screen, d, K):
    # waves with no component (K < 8), one (8), one or two (9, 15), several; the upper half empty (K <= 32), holding one component
    # (33), partly and wholly filled
    X, p = mixture(d, K, 700, seed=1000 * d + K)
    trail = both(ctx, screen, X, three_passes(p))
    assert routes(trail) == THREE
    assert 700 <= trail[-1]["candidates"] <= K * 700


def test_bucket_shapes(ctx, screen):
    """Per-segment counts of a component's bucket inside one 256-sample tile (a row's only candidate is its own component):
    component 0 (0, 0, 0, 1) and component 1 (64, 0, 0, 0) in the first tile; component 4 (64, 64, 64, 64), a full bucket, in the
    second; component 2 (10, 10, 0, 0) -- a group of 16 that spans two segments -- and component 3 (16, 0, 17, 0) in the third;
    component 5 empty; component 6 fills the rest."""
    d, K, fill = 12, 7, 6
    tile0 = [[1] * 64, [fill] * 64, [fill] * 64, [0] + [fill] * 63]
    tile1 = [[4] * 64] * 4
    tile2 = [[2] * 10 + [3] * 16 + [fill] * 38, [2] * 10 + [fill] * 54, [3] * 17 + [fill] * 47, [fill] * 64]
    rng = np.random.default_rng(7)
    comp = np.concatenate([rng.permutation(np.array(seg)) for tile in (tile0, tile1, tile2) for seg in tile])
    assert comp.shape == (768,) and not np.any(comp == 5)
    X, p = placed(axis_means(K, d), comp, seed=8)
    trail = both(ctx, screen, X, three_passes(p))
    assert routes(trail) == THREE
    assert trail[1]["candidates"] == 768 and trail[2]["candidates"] == 768


def test_every_pair_a_candidate(ctx, screen):
    # 16 coincident components: every bucket of the first tile holds 256 entries, of the second 44
    d, n, K = 12, 300, 16
    rng = np.random.default_rng(11)
    mu = 8.0 * rng.standard_normal((1, d))
    X = np.ascontiguousarray(mu + rng.standard_normal((n, d)))
    p = (np.full(K, 1.0 / K), np.repeat(mu, K, axis=0), np.stack([np.eye(d)] * K))
    trail = both(ctx, screen, X, three_passes(p))
    assert routes(trail) == THREE
    assert trail[1]["candidates"] == K * n and trail[2]["candidates"] == K * n


def test_ties_across_the_halves(ctx, screen):
    """K = 64, components 3 and 40 coincident (a tie between the halves: the lower one gives the maximum) and 35 and 36 coincident (a
    tie inside the upper half). A row of one of the four keeps its pair, every other row its own component alone."""
    d, K, n = 32, 64, 600
    means = axis_means(K, d)
    means[40] = means[3]
    means[36] = means[35]
    rng = np.random.default_rng(13)
    comp = rng.integers(0, K, n)
    comp[:8] = [3, 40, 35, 36, 3, 40, 35, 36]                        # (each of the four has rows whatever the draw gave)
    X, p = placed(means, comp, seed=14)
    trail = both(ctx, screen, X, three_passes(p))
    assert routes(trail) == THREE
    by_hand = n + int(np.sum(np.isin(comp, [3, 40, 35, 36])))
    assert trail[1]["candidates"] == by_hand and trail[2]["candidates"] == by_hand


def test_maximum_from_the_upper_half(ctx, screen):
    # every row belongs to a component >= 32: the sample's maximum always comes across from the upper half
    d, K, n = 32, 64, 600
    comp = np.random.default_rng(15).integers(32, K, n)
    X, p = placed(axis_means(K, d), comp, seed=16)
    trail = both(ctx, screen, X, three_passes(p))
    assert routes(trail) == THREE
    assert trail[1]["candidates"] == n and trail[2]["candidates"] == n


def test_unusable_stored_values_in_both_halves(ctx, screen):
    # rows hundreds of standard deviations from every component, two rows whose stored values are beyond 2^40 in all 40 components
    # (never bounded from, in either half), and a component far from every row
    X, p = mixture(24, 40, 1000, seed=17)
    X[::97] += 400.0
    X[5] += 4.0e5
    X[6] -= 4.0e5
    mu = p[1].copy()
    mu[0] = 50.0
    trail = both(ctx, screen, X, three_passes((p[0], mu, p[2])))
    assert routes(trail) == THREE


def test_exactness_words_across_passes(ctx, screen):
    # five passes on one handle: from the second on each starts from the words (two 32-bit halves a sample) the last one wrote
    X, p = mixture(16, 40, 900, seed=19)
    q = nudged(p)
    trail = both(ctx, screen, X, [p, p, q, q, nudged(q)])
    assert routes(trail) == [(0, 1, 0), (1, 1, 0), (2, 1, 0), (3, 1, 0), (4, 1, 0)]
    for c in trail[1:]:
        assert 900 <= c["candidates"] <= 40 * 900


def test_two_shard_group(ctx, screen):
    from ml_amd import _lib
    X, p = mixture(24, 40, 1500, seed=23)
    grp = _lib.Context.group(2, device_ids=[0, 0])
    try:
        trail = both(grp, screen, X, three_passes(p), shards=2)
    finally:
        grp.close()
    assert routes(trail) == [(0, 2, 0), (2, 2, 0), (4, 2, 0)]           # summed over the shards
    single = run_passes(ctx, screen, "1", X, three_passes(p))
    assert trail[-1]["candidates"] == single[3][-1]["candidates"]


def test_automatic_route_d28(ctx, screen):
    """Without the switch, D = 28 with K = 64 is screened from the third pass on, as D = 32 is (em_estep_screen_preferred: both were
    measured faster screened); the results are the dense kernel's."""
    X, p = mixture(28, 64, 2000, seed=29)
    auto = run_passes(ctx, screen, None, X, [p] * 5)
    off = run_passes(ctx, screen, "0", X, [p] * 5)
    for a, b in zip(auto[0], off[0]):
        same(a, b)
    assert bits(auto[1]) == bits(off[1])
    assert np.array_equal(auto[2], off[2])
    assert routes(auto[3]) == [(0, 1, 0), (0, 2, 0), (1, 2, 0), (2, 2, 0), (3, 2, 0)]
