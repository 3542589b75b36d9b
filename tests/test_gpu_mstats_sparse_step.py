"""One step of the sparse statistics kernel's bucket loop (device/em_mstats_sparse.hip), case by case for what the step is made of:
sum r and sum r x~ accumulated per lane group on the vector unit and added across the four groups at the end; the sentinel row
(sample index 64: r = 0, x~ = 0) that the entries past a bucket's end read -- what the cases can show is a wrong r there: an x~ row
read by mistake is multiplied by r = 0 and leaves no trace with finite data; the single scan of a bucket's mask, four entries taken
per step; the shift values read once per launch and the "component >= K" masks behind a wave-uniform test.

Every case is ONE em_step with the sparse kernel forced (MLHIP_MSTATS_SPARSE=1) against the dense one (=0) on at most a few hundred
rows, with the tolerances of test_gpu_mstats_sparse.py: log-likelihood bit-equal, mixing and means <= 1e-13, covariances <= 1e-12
relative. On rows that one component owns r is exactly 1.0 or 0.0, so the statistics are plain sums of the owned rows: the mixing
weights are counts / n, and means and covariances go against numpy as well (`_numpy_step`), with the same tolerances."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 64
TOL_LIN, TOL_COV = 1e-13, 1e-12


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
    assert relerr(a[1], b[1]) <= TOL_LIN
    assert relerr(a[2], b[2]) <= TOL_LIN
    assert relerr(a[3], b[3]) <= TOL_COV
    return a, b


def _admitted(ctx, mode, d, K):
    from ml_amd import _lib
    mode("1")
    probe = _lib.Data(ctx, np.zeros((TILE, d)))
    ok = probe.em_route(K)["self_norm"]
    probe.close()
    if not ok:
        pytest.skip(f"the self-normalising route does not take d = {d}, K = {K}")


def _overlapping(d, K, n, seed, spread, offset=0.0):
    """The generator of test_gpu_mstats_sparse.py (spread = 6: a few nonzero responsibilities per row), every coordinate moved by
    `offset`: the column means, hence `shift`, are then ~offset while the spread of the rows stays what it was."""
    rng = np.random.default_rng(seed)
    means = spread * rng.standard_normal((K, d))
    comp = rng.integers(0, K, n)
    X = np.ascontiguousarray(means[comp] + rng.standard_normal((n, d)) + offset)
    return X, np.full(K, 1.0 / K), means + 0.2 * rng.standard_normal((K, d)) + offset, np.stack([np.eye(d)] * K)


def _owned(d, K, comp, seed, scale=None):
    """Rows that belong to exactly one component each (the construction of test_gpu_mstats_sparse_buckets.py): row i is a draw
    (sigma = 3) around the mean of comp[i], the means drawn with |mu|^2 ~ 10 800 whatever d, so |delta|^2 ~ 21 600 between two of
    them. Checked here in float64 from the parameters the kernels get (unit covariances, equal weights: the log-weights differ by
    -|x - mu_k|^2 / 2 only): every row's second-largest log-weight lies more than 800 below its largest, where exp_nonpos returns
    exactly 0 (it does from -745.2 on), and every pair of means is more than |delta|^2 = 1500 apart. (The sums hold terms of size
    |x - shift|^2 ~ 1e4 and the covariances come out of their difference: two summation orders differ by ~1e4 eps there, which the
    tolerance measures against max |S| ~ 9.) Every mean lies ~100 from the column means, so no cloud is centred on `shift`: a term
    dropped from sum r x~ moves the mean by ~100 / count. `scale` = (component, factor) multiplies that component's mean."""
    rng = np.random.default_rng(seed)
    means = 104.0 / np.sqrt(d) * rng.standard_normal((K, d))
    if scale is not None:
        means[scale[0]] *= scale[1]
    comp = np.asarray(comp)
    X = np.ascontiguousarray(means[comp] + 3.0 * rng.standard_normal((len(comp), d)))
    mu0 = means + 0.2 * rng.standard_normal((K, d))
    _assert_owned(X, mu0, comp)
    return X, np.full(K, 1.0 / K), mu0, np.stack([np.eye(d)] * K)


def _assert_owned(X, mu0, comp):
    K = len(mu0)
    gaps = ((mu0[:, None, :] - mu0[None, :, :]) ** 2).sum(-1) + 1e9 * np.eye(K)
    assert gaps.min() > 1500.0
    lw = -0.5 * ((X[:, None, :] - mu0[None, :, :]) ** 2).sum(-1)
    below = np.sort(lw - lw.max(axis=1, keepdims=True), axis=1)
    assert np.all(below[:, -1] == 0.0) and (K == 1 or np.all(below[:, -2] < -800.0))
    assert np.array_equal(lw.argmax(axis=1), comp)


def _check_owned(out, comp, K):
    """Exactly the rows of comp behind every component: the mixing weights are counts / n, to rounding."""
    counts = np.bincount(comp, minlength=K)
    assert np.max(np.abs(np.asarray(out[1]) - counts / len(comp))) <= 1e-15
    assert np.all(np.asarray(out[1])[counts == 0] == 0.0)


_numpy_cache = {}


def _numpy_step(X, comp, K, key):
    """Mixing weights, means and covariances of owned rows (r exactly 1 or 0) from numpy, for the components that own a row.
    The reference is the centred two-pass form in extended precision. The kernels form sum x~ and sum x~ x~^T, x~ = x - column
    mean, and close with cov = (M2 - S1 (S1 / S0)^T) / S0 + 1e-15 I; that form is evaluated here in float64 with the sums taken in
    numpy's forward order (cumsum) and in its pairwise order (a sum along the contiguous axis), and both must stay within a
    QUARTER of the tolerances from the reference: two orders of these inputs differ by ~|x~|^2 eps ~ 1e4 eps in a covariance entry,
    measured against max |S| ~ 9 (the generator's docstring), an order of magnitude inside 1e-12. A kernel that sums in a third
    order then has the rest of the tolerance for itself. Computed once per `key` and shared."""
    if key in _numpy_cache:
        return _numpy_cache[key]
    n, d = X.shape
    counts = np.bincount(comp, minlength=K)
    own = np.flatnonzero(counts)
    shift = X.mean(axis=0)
    Xl = X.astype(np.longdouble)
    mu_ref, S_ref = np.empty((len(own), d)), np.empty((len(own), d, d))
    for t, c in enumerate(own):
        rows = Xl[comp == c]
        m = rows.sum(axis=0) / len(rows)
        mu_ref[t] = m
        S_ref[t] = (rows - m).T @ (rows - m) / len(rows) + np.longdouble(1e-15) * np.eye(d)

    def closed(total):
        mu, S = np.empty_like(mu_ref), np.empty_like(S_ref)
        for t, c in enumerate(own):
            xt = X[comp == c] - shift
            s0 = float(len(xt))
            s1 = total(xt)
            m2 = total((xt[:, :, None] * xt[:, None, :]).reshape(len(xt), d * d)).reshape(d, d)
            mu[t] = shift + s1 / s0
            S[t] = (m2 - np.outer(s1, s1 / s0)) / s0 + 1e-15 * np.eye(d)
        return mu, S

    forward = closed(lambda a: np.cumsum(a, axis=0)[-1])
    pairwise = closed(lambda a: np.sum(np.ascontiguousarray(a.T), axis=1))
    for mu, S in (forward, pairwise):
        assert relerr(mu, mu_ref) <= TOL_LIN / 4
        assert relerr(S, S_ref) <= TOL_COV / 4
    _numpy_cache[key] = (own, counts[own] / n, mu_ref, S_ref)
    return _numpy_cache[key]


def _check_numpy(out, X, comp, K, key):
    own, pi, mu, S = _numpy_step(X, comp, K, key)
    assert relerr(np.asarray(out[1])[own], pi) <= TOL_LIN
    assert relerr(np.asarray(out[2])[own], mu) <= TOL_LIN
    assert relerr(np.asarray(out[3])[own], S) <= TOL_COV


def _owned_case(ctx, mode, d, K, comp, seed, key, scale=None):
    problem = _owned(d, K, comp, seed, scale)
    a, b = _compare(ctx, mode, problem)
    for out in (a, b):
        _check_owned(out, comp, K)
        _check_numpy(out, problem[0], comp, K, key)
    return problem, a


# ---- sum r and sum r x~ per lane group --------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [12, 13, 32])
def test_lane_group_partial_sums(ctx, mode, d):
    # one tile; components in different waves and slots own exactly 1 .. 7 rows, so the last entry used of a step is entry 0, 1,
    # 2, 3 (sizes 1 / 5, 2 / 6, 3 / 7, 4) and the lane groups behind it add zeros; one cloud of 36 rows (9 full steps). No cloud
    # is centred on `shift`: the small ones lie ~100 from it, the large one (which pulls the column means towards itself) more
    # than 20, seven times its own spread -- a lane group dropped from the final sum moves its mean by a quarter of that
    K = 64
    _admitted(ctx, mode, d, K)
    sizes = {9: 1, 18: 2, 27: 3, 36: 4, 45: 5, 54: 6, 63: 7, 2: 36}
    comp = np.concatenate([np.full(m, c) for c, m in sizes.items()])
    assert len(comp) == TILE
    comp = np.random.default_rng(5).permutation(comp)
    problem, a = _owned_case(ctx, mode, d, K, comp, seed=30 + d, key=("groups", d))
    shift = problem[0].mean(axis=0)
    assert np.min(np.linalg.norm(np.asarray(a[2])[list(sizes)] - shift, axis=1)) > 20.0


# ---- the sentinel row -------------------------------------------------------------------------------------------------------
def test_sentinel_behind_the_last_bucket(ctx, mode):
    # wave 2: component 2 (slot 0) owns 5 rows, component 10 (slot 1) one row, its slots 2 .. 7 nothing: the last step of the wave
    # has one entry and three sentinel reads, and the step loaded behind it is all sentinel. Wave 5 owns nothing in the tile at
    # all. Row 0 belongs to component 7 (wave 7), whose mean is scaled so that row 0 has the largest coordinates of the tile: an
    # entry past a bucket's end that read sample row 0 instead of the sentinel row would bring them in
    K, d = 64, 12
    sizes = {2: 5, 10: 1, 0: 9, 33: 14, 20: 11, 62: 23}
    rest = np.random.default_rng(6).permutation(np.concatenate([np.full(m, c) for c, m in sizes.items()]))
    comp = np.concatenate([[7], rest])
    assert len(comp) == TILE and not np.any(comp % 8 == 5)
    problem, _ = _owned_case(ctx, mode, d, K, comp, seed=41, key="sentinel", scale=(7, 3.0))
    X = problem[0]
    assert np.max(np.abs(X[0])) == np.max(np.abs(X)) and np.max(np.abs(X[0])) > 1.5 * np.max(np.abs(X[1:]))


@pytest.mark.parametrize("n", [1, 65])
def test_sentinel_smallest_tiles(ctx, mode, n):
    # n = 1: one entry in the whole launch; n = 65: the second tile holds one row, seven of its eight waves have no entry
    K, d = 64, 20
    comp = np.random.default_rng(n).choice([3, 10, 17, 24, 45, 62], n)
    _owned_case(ctx, mode, d, K, comp, seed=50 + n, key=("small", n))


# ---- every mask bit scanned once --------------------------------------------------------------------------------------------
def test_single_scan_bucket_sizes(ctx, mode):
    # tile 0: buckets of 4, 8 and 12 (the remainder is exactly empty at a step boundary), of 5, 9 and 13 (one entry past it), one
    # bucket with bits in the top byte of its mask only (rows 57, 60, 62), one with bit 63 only; tile 1: a bucket of 64
    K, d = 64, 20
    sizes = {1: 4, 18: 8, 35: 12, 4: 5, 21: 9, 62: 13, 11: 5}
    low = np.random.default_rng(7).permutation(np.concatenate([np.full(m, c) for c, m in sizes.items()]))
    top = np.array([11, 7, 11, 11, 7, 11, 7, 40])             # rows 56 .. 63
    comp = np.concatenate([low, top, np.full(TILE, 54)])
    assert len(low) == 56 and len(comp) == 2 * TILE
    assert np.array_equal(np.flatnonzero(comp == 7), [57, 60, 62]) and np.array_equal(np.flatnonzero(comp == 40), [63])
    _owned_case(ctx, mode, d, K, comp, seed=61, key="scan")


# ---- shift read once, the K masks behind a wave-uniform test ------------------------------------------------------------------
@pytest.mark.parametrize("K", [64, 40, 9])
@pytest.mark.parametrize("d", [13, 20])
def test_shift_and_component_masks(ctx, mode, d, K):
    # d = 13, 20: x rows >= d (written as 0), the repeated first 12 coordinates, waves whose later x rows are all padding. The same
    # rows under K = 64 (no component masked), 40 and 9 (masked): owned rows of the first nine components, then rows with a few
    # nonzero responsibilities each whose column means, hence shift, are ~1e3 with unit spread around their components
    _admitted(ctx, mode, d, K)
    n = 3 * TILE + 5
    comp = np.random.default_rng(d).integers(0, 9, n)
    X, _, mu0, S0 = _owned(d, 64, comp, seed=70 + d)
    _assert_owned(X, mu0[:K], comp)
    a, b = _compare(ctx, mode, (X, np.full(K, 1.0 / K), mu0[:K], S0[:K]))
    for out in (a, b):
        _check_owned(out, comp, K)
        _check_numpy(out, X, comp, K, ("masks", d))
    X, _, mu0, S0 = _overlapping(d, 64, n, seed=80 + d, spread=6.0, offset=1e3)
    assert np.all(np.abs(X.mean(axis=0) - 1e3) < 5.0)
    _compare(ctx, mode, (X, np.full(K, 1.0 / K), mu0[:K], S0[:K]))


def test_reproducible(ctx, mode):
    comp = np.random.default_rng(8).integers(0, 64, 3 * TILE + 5)
    problem = _owned(32, 64, comp, seed=90)
    a = _step(ctx, *problem, "1", mode)
    b = _step(ctx, *problem, "1", mode)
    for u, v in zip(a, b):
        assert np.array_equal(np.asarray(u), np.asarray(v), equal_nan=True)
