"""The bucket loop of the sparse statistics kernel (device/em_mstats_sparse.hip): buckets are formed from the staging ballots
(one 64-bit sample mask per component and tile), walked four entries per step by scalar bit scans, with the next step's operands
loaded behind the current step's MFMAs -- across component boundaries. Every case runs ONE em_step with the sparse kernel forced
(MLHIP_MSTATS_SPARSE=1) against the dense one (=0), on a few hundred rows, with the tolerances of test_gpu_mstats_sparse.py:
log-likelihood bit-equal, mixing and means <= 1e-13, covariances <= 1e-12 relative. Shapes: bucket sizes around the step of four
and the extremes (0, 1, 3, 4, 5, 8, 9, 64), every bucket full, ragged ends, component slots (K = 64, 40, 9, the smallest), the
quad wrap-around of the sample row (d = 12, 20, 32, one d that is no multiple of 4), one bit in every byte of a mask."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 64


def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b))          # (a component without rows: the same non-numbers from both kernels)
    a, b = np.nan_to_num(a), np.nan_to_num(b)
    return np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b)))


@pytest.fixture(scope="module")
def ctx():
    from ml_amd import _lib
    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture
def mode():
    old = os.environ.get("MLHIP_MSTATS_SPARSE")

    def set_mode(m):
        if m is None:
            os.environ.pop("MLHIP_MSTATS_SPARSE", None)
        else:
            os.environ["MLHIP_MSTATS_SPARSE"] = m
    yield set_mode
    set_mode(old)


def _step(ctx, X, pi, mu, S, m, mode):
    """One em_step with the statistics kernel forced; asserts that the self-normalising route with that kernel is the one taken."""
    from ml_amd import _lib
    mode(m)
    dt = _lib.Data(ctx, X)
    route = dt.em_route(len(pi))
    assert route["self_norm"] and route["sparse"] is (m == "1") and X.shape[1] <= 32 and len(pi) <= 64, route
    out = dt.em_step(pi, mu, S)
    dt.close()
    return out


def _compare(ctx, mode, problem):
    X, pi0, mu0, S0 = problem
    a, b = _step(ctx, X, pi0, mu0, S0, "1", mode), _step(ctx, X, pi0, mu0, S0, "0", mode)
    assert a[0] == b[0]                     # (max, sum of exponentials) come from the same staging code: bit-identical
    assert np.isfinite(a[0])
    assert relerr(a[1], b[1]) <= 1e-13
    assert relerr(a[2], b[2]) <= 1e-13
    assert relerr(a[3], b[3]) <= 1e-12
    return a, b


def _overlapping(d, K, n, seed, spread):
    """The generator of test_gpu_mstats_sparse.py: spread = 0.05 leaves every responsibility nonzero, 6 a few per row."""
    rng = np.random.default_rng(seed)
    means = spread * rng.standard_normal((K, d))
    comp = rng.integers(0, K, n)
    X = np.ascontiguousarray(means[comp] + rng.standard_normal((n, d)))
    return X, np.full(K, 1.0 / K), means + 0.2 * rng.standard_normal((K, d)), np.stack([np.eye(d)] * K)


def _owned(d, K, comp, seed):
    """Rows that belong to exactly one component each: row i is a draw (sigma = 3) around the mean of comp[i], the means drawn
    with |mu|^2 ~ 10 800 whatever d, so |delta|^2 ~ 21 600 between two of them. Checked here in float64 from the parameters the
    kernels get (unit covariances, equal weights: the log-weights differ by -|x - mu_k|^2 / 2 only): every row's second-largest
    log-weight lies more than 800 below its largest, where exp_nonpos returns exactly 0 (it does from -745.2 on), and every pair
    of means is more than |delta|^2 = 1500 apart. (The sums hold terms of size |x - shift|^2 ~ 1e4 and the covariances come out
    of their difference: two summation orders differ by ~1e4 eps there, which the tolerance measures against max |S| ~ 9.)"""
    rng = np.random.default_rng(seed)
    means = 104.0 / np.sqrt(d) * rng.standard_normal((K, d))
    comp = np.asarray(comp)
    X = np.ascontiguousarray(means[comp] + 3.0 * rng.standard_normal((len(comp), d)))
    mu0 = means + 0.2 * rng.standard_normal((K, d))
    gaps = ((mu0[:, None, :] - mu0[None, :, :]) ** 2).sum(-1) + 1e9 * np.eye(K)
    assert gaps.min() > 1500.0
    lw = -0.5 * ((X[:, None, :] - mu0[None, :, :]) ** 2).sum(-1)
    below = np.sort(lw - lw.max(axis=1, keepdims=True), axis=1)
    assert np.all(below[:, -1] == 0.0) and (K == 1 or np.all(below[:, -2] < -800.0))
    assert np.array_equal(lw.argmax(axis=1), comp)
    return X, np.full(K, 1.0 / K), mu0, np.stack([np.eye(d)] * K)


def _check_owned(out, comp, K):
    """Exactly the rows of comp behind every component: the mixing weights are counts / n, to rounding."""
    counts = np.bincount(comp, minlength=K)
    assert np.max(np.abs(np.asarray(out[1]) - counts / len(comp))) <= 1e-15
    assert np.all(np.asarray(out[1])[counts == 0] == 0.0)


@pytest.mark.parametrize("d", [12, 20, 32])
def test_bucket_sizes_around_a_step(ctx, mode, d):
    # one tile; components in different waves and slots own 0 (all the others), 1, 3, 4, 5, 8, 9 and the remaining 34 rows
    K = 64
    sizes = {3: 1, 10: 3, 17: 4, 24: 5, 33: 8, 42: 9, 60: 34}
    comp = np.concatenate([np.full(m, c) for c, m in sizes.items()])
    assert len(comp) == TILE
    comp = np.random.default_rng(1).permutation(comp)
    a, b = _compare(ctx, mode, _owned(d, K, comp, seed=10 + d))
    _check_owned(a, comp, K)
    _check_owned(b, comp, K)


def test_whole_tiles_of_one_component(ctx, mode):
    # rows sorted by component: a bucket of 64 (16 steps) and 63 empty ones per tile; the last tile is partial
    K, d = 64, 20
    comp = np.concatenate([np.full(2 * TILE, 5), np.full(TILE, 62), np.full(TILE, 20), np.full(7, 63)])
    a, _ = _compare(ctx, mode, _owned(d, K, comp, seed=2))
    _check_owned(a, comp, K)


def test_one_bit_in_every_mask_byte(ctx, mode):
    # component 37 owns exactly one row in each group of 8 consecutive rows of the tile (another position in each group)
    K, d = 64, 12
    rng = np.random.default_rng(3)
    comp = rng.choice([c for c in range(K) if c != 37], TILE)
    comp[8 * np.arange(8) + np.array([0, 7, 3, 5, 1, 6, 2, 4])] = 37
    a, _ = _compare(ctx, mode, _owned(d, K, comp, seed=4))
    _check_owned(a, comp, K)


@pytest.mark.parametrize("d,K", [(32, 64), (20, 40), (12, 9)])
def test_every_bucket_full(ctx, mode, d, K):
    # all 64 x K pairs of a tile nonzero: 16 steps for each of a wave's components, the loads pipelined across every boundary
    _compare(ctx, mode, _overlapping(d, K, 3 * TILE + 5, seed=d + K, spread=0.05))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 3 * TILE + 5])
@pytest.mark.parametrize("d,K,spread", [(32, 64, 0.05), (12, 9, 6.0)])
def test_ragged_ends(ctx, mode, n, d, K, spread):
    # a partial last tile, padding rows that must contribute nothing, more CUs than tiles; every bucket full, and a few entries per
    # bucket (there with 9 components: with as many components as rows every covariance is the rounding noise of a difference
    # that cancels, and an error relative to max |S| measures nothing)
    _compare(ctx, mode, _overlapping(d, K, n, seed=100 + n, spread=spread))


@pytest.mark.parametrize("d,K", [(32, 64), (20, 40), (12, 9), (12, None), (13, 40)])
def test_component_slots_and_dimensions(ctx, mode, d, K):
    # K = 40: waves with 5 slots, mask bytes beyond K must read as empty; K = 9: slot 1 used by one wave only; K = None: the
    # smallest K the route admits; d = 13: no multiple of 4, where the route admits it
    from ml_amd import _lib
    mode("1")
    probe = _lib.Data(ctx, np.zeros((TILE, d)))
    admitted = [k for k in range(1, 65) if probe.em_route(k)["self_norm"]]
    probe.close()
    if K is None:
        assert admitted
        K = admitted[0]
    elif K not in admitted:
        pytest.skip(f"the self-normalising route does not take d = {d}, K = {K}")
    n = 5 * TILE + 11
    comp = np.random.default_rng(d * K).integers(0, K, n)
    a, _ = _compare(ctx, mode, _owned(d, K, comp, seed=7 * d + K))
    _check_owned(a, comp, K)
    _compare(ctx, mode, _overlapping(d, K, n, seed=d + 3 * K, spread=6.0))


def test_reproducible(ctx, mode):
    for problem in (_overlapping(32, 64, 5 * TILE + 11, seed=21, spread=0.05), _overlapping(20, 40, 5 * TILE + 11, seed=22, spread=6.0)):
        a = _step(ctx, *problem, "1", mode)
        b = _step(ctx, *problem, "1", mode)
        for u, v in zip(a, b):
            assert np.array_equal(np.asarray(u), np.asarray(v), equal_nan=True)
