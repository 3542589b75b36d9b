"""Weighted K-means on the GPU (mlhip_kmeans_step_weighted / _iterate_weighted / _assign_weighted, KMeans.fit(X, sample_weight=w)).

The yardstick of the exact cases is the UNWEIGHTED library on the replicated sample (row i repeated w_i times): X lies on the grid
2^-10 * integers with |x| < 16 and the weights are small integers, so every product w x, every coordinate sum, every count and (with
centroids on the grid) every squared distance and its weighted sum is exact in double -- whatever the order of summation. Those
quantities are compared with np.array_equal. The real-weight cases are held to math.fsum over the GPU's own labels.
Needs a GPU: `timeout -k 10 900 pytest tests/test_gpu_kmeans_weights.py -m gpu -x`."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from ml_amd import _lib
    c = _lib.Context()
    yield c
    c.close()


def _block(ctx, X, w=None):
    from ml_amd import _lib
    dt = _lib.Data(ctx, np.ascontiguousarray(X, dtype=np.float64))
    if w is not None:
        dt.set_weights(w)
    return dt


def grid_case(n, d, K, seed=0, low=0):
    """X on 2^-10 Z, |x| < 16; integer weights low..7; K centroids on the grid: distinct-index rows of X."""
    rng = np.random.default_rng(1000 * seed + 7 * n + 3 * d + K)
    X = rng.integers(-16 * 1024 + 1, 16 * 1024, size=(n, d)).astype(np.float64) / 1024.0
    w = rng.integers(low, 8, size=n).astype(np.float64)
    w[0] = 7.0                                              # (the largest weight is 7 in every case)
    C0 = X[rng.choice(n, size=min(K, n), replace=False)].copy()
    if K > n:                                               # (more clusters than rows: the rest are further grid points)
        C0 = np.vstack([C0, rng.integers(-16 * 1024 + 1, 16 * 1024, size=(K - n, d)).astype(np.float64) / 1024.0])
    return X, w, C0


def replicate(X, w):
    return np.ascontiguousarray(np.repeat(X, w.astype(np.int64), axis=0))


def check_replicated_step(ctx, n, d, K, expect_route=None):
    X, w, C0 = grid_case(n, d, K)
    R = replicate(X, w)
    dw, dr, du = _block(ctx, X, w), _block(ctx, R), _block(ctx, X)
    try:
        if expect_route:
            route = dw.kmeans_route(K)
            for key, value in expect_route.items():
                assert route[key] == value, (key, route)
        iw, changed_w, counts_w, cent_w = dw.kmeans_step(C0, weighted=True)
        labels_w, dist_w = dw.kmeans_labels(), dw.kmeans_distances()
        ir, _, counts_r, cent_r = dr.kmeans_step(C0)
        iu, changed_u, _, _ = du.kmeans_step(C0)
        # counts and centroids: those of the unweighted step on the replicated block
        assert np.array_equal(counts_w, counts_r)
        assert np.array_equal(cent_w, cent_r)
        # labels, distances and n_changed (a count of rows): those of the unweighted step on X itself
        assert changed_w == changed_u == n
        assert np.array_equal(labels_w, du.kmeans_labels())
        assert np.array_equal(dist_w, du.kmeans_distances())
        # weighted inertia: every distance is a multiple of 2^-20; the sums are exact while the total stays below 2^33
        exact = math.fsum(w * dist_w)
        assert exact < 2.0 ** 33 and np.all(dist_w * 2.0 ** 20 == np.floor(dist_w * 2.0 ** 20))
        ia, changed_a = dw.kmeans_assign(C0, weighted=True)
        ira, _ = dr.kmeans_assign(C0)
        assert ia == ira == ir == iw == exact
        assert changed_a == 0
        assert np.array_equal(dw.kmeans_labels(), labels_w) and np.array_equal(dw.kmeans_distances(), dist_w)
    finally:
        dw.close(); dr.close(); du.close()


N_SHAPES = [(n, 3, 2) for n in (63, 64, 65, 1025, 2049)]


@pytest.mark.parametrize("switch", [None, "valu", "mfma"])
@pytest.mark.parametrize("n,d,K", N_SHAPES)
def test_replicated_rows_exact_by_rows(ctx, monkeypatch, n, d, K, switch):
    if switch:
        monkeypatch.setenv("MLHIP_KMEANS", switch)
    check_replicated_step(ctx, n, d, K)


@pytest.mark.parametrize("d", [1, 5, 8, 12, 33, 65, 130])
def test_replicated_rows_exact_by_dimension(ctx, d):
    check_replicated_step(ctx, 300, d, 3)


@pytest.mark.parametrize("K,route", [(1, None), (16, None), (17, None), (256, {"kernel": "matrix"})])
def test_replicated_rows_exact_by_clusters(ctx, K, route):
    check_replicated_step(ctx, 600, 8, K, route)


def test_replicated_rows_exact_on_the_padded_copy(ctx):
    check_replicated_step(ctx, 400, 6, 130, {"pad": True})


def test_replicated_rows_exact_chunked_by_dimension(ctx):
    check_replicated_step(ctx, 600, 64, 700)       # 700 clusters x (3 * 64 + 3) words do not fit LDS: 2 dimensions per pass


def test_replicated_rows_exact_chunked_by_clusters(ctx):
    check_replicated_step(ctx, 9000, 2, 8000)      # not even one dimension of 8000 clusters fits: the clusters are chunked too


# ---- real weights ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,d,K", [(3001, 8, 5), (3001, 32, 64)])
def test_real_weights_against_fsum(ctx, n, d, K):
    """Per coordinate |c_gpu - c_ref| <= 2^-49 sum w|x| / sum w over the cluster: at most two roundings converting each of the sum and
    the count (2 * 2^-53 each, relative to sum w|x| resp. sum w), one division (2^-53), and a truncation of at most N units of
    2^-94 * 4 max w max|x_j| -- together below 6 * 2^-53 < 2^-49. Counts to 2^-51 relative."""
    rng = np.random.default_rng(n + d + K)
    X = rng.standard_normal((n, d)) + 3.0 * rng.integers(0, 3, size=(n, 1))
    w = np.exp(3.0 * rng.standard_normal(n))
    C0 = X[rng.choice(n, size=K, replace=False)].copy()
    dw = _block(ctx, X, w)
    try:
        inertia, _, counts, cent = dw.kmeans_step(C0, weighted=True)
        labels, dist = dw.kmeans_labels(), dw.kmeans_distances()
    finally:
        dw.close()
    ref_inertia = math.fsum(w * dist)
    assert abs(inertia - ref_inertia) <= 2.0 ** -40 * ref_inertia      # (a tree sum of n rounded products: n * 2^-53 at the most)
    for k in range(K):
        rows = np.nonzero(labels == k)[0]
        total = math.fsum(w[rows])
        assert abs(counts[k] - total) <= 2.0 ** -51 * total, (k, counts[k], total)
        if total == 0:
            assert not cent[k].any()
            continue
        for j in range(d):
            ref = math.fsum(w[rows] * X[rows, j]) / total
            bound = 2.0 ** -49 * math.fsum(w[rows] * np.abs(X[rows, j])) / total
            assert abs(cent[k, j] - ref) <= bound, (k, j, cent[k, j], ref, bound)


# ---- edge weights ---------------------------------------------------------------------------------------------------------------

def test_a_cluster_of_weight_zero_rows_goes_to_the_origin(ctx):
    rng = np.random.default_rng(5)
    A = rng.integers(8 * 1024, 12 * 1024, size=(40, 3)) / 1024.0
    B = -rng.integers(8 * 1024, 12 * 1024, size=(30, 3)) / 1024.0
    X = np.ascontiguousarray(np.vstack([A, B]))
    w = np.concatenate([rng.integers(1, 8, size=40), np.zeros(30)]).astype(np.float64)
    C0 = np.array([[10.0, 10.0, 10.0], [-10.0, -10.0, -10.0]])
    dw, du = _block(ctx, X, w), _block(ctx, X)
    try:
        _, changed, counts, cent = dw.kmeans_step(C0, weighted=True)
        du.kmeans_step(C0)
        assert counts[1] == 0.0 and not cent[1].any()
        assert counts[0] == w.sum() and np.array_equal(cent[0], (w[:40, None] * A).sum(axis=0) / w.sum())
        labels = dw.kmeans_labels()
        assert changed == 70 and np.array_equal(labels, np.repeat([0, 1], [40, 30]).astype(np.uint32))
        assert np.array_equal(dw.kmeans_distances(), du.kmeans_distances()) and dw.kmeans_distances()[40:].min() > 0
    finally:
        dw.close(); du.close()


def test_a_tiny_weight_leaves_the_sums_unchanged(ctx):
    X, w, C0 = grid_case(200, 4, 3, seed=2, low=1)
    w[:] = 1.0
    tiny, zero = w.copy(), w.copy()
    tiny[1], zero[1] = 2.0 ** -100, 0.0
    dt, dz = _block(ctx, X, tiny), _block(ctx, X, zero)
    try:
        it, _, counts_t, cent_t = dt.kmeans_step(C0, weighted=True)
        iz, _, counts_z, cent_z = dz.kmeans_step(C0, weighted=True)
        assert np.isfinite(it) and np.all(np.isfinite(counts_t)) and np.all(np.isfinite(cent_t))
        assert np.array_equal(counts_t, counts_z) and np.array_equal(cent_t, cent_z)
    finally:
        dt.close(); dz.close()


def test_an_overflowing_product_fails_loudly_and_the_handle_stays_usable(ctx):
    X, w, C0 = grid_case(100, 2, 2, seed=3, low=1)
    X[5, 1] = 1e150
    big = w.copy()
    big[9] = 1e160                                       # 1e310 overflows; every squared distance stays finite
    dt = _block(ctx, X, big)
    try:
        with pytest.raises(ValueError, match="overflow"):
            dt.kmeans_step(C0, weighted=True)
        with pytest.raises(ValueError, match="overflow"):
            dt.kmeans_assign(C0, weighted=True)
        dt.set_weights(w)
        _, changed, counts, cent = dt.kmeans_step(C0, weighted=True)
        assert changed == 100 and counts.sum() == w.sum() and np.all(np.isfinite(cent))
    finally:
        dt.close()


def test_a_weighted_call_on_an_unweighted_handle_is_refused(ctx):
    X, w, C0 = grid_case(100, 2, 2, seed=4)
    dt = _block(ctx, X)
    try:
        for call in (lambda: dt.kmeans_step(C0, weighted=True), lambda: dt.kmeans_assign(C0, weighted=True),
                     lambda: dt.kmeans_iterate(C0, 5, weighted=True)):
            with pytest.raises(ValueError, match="no weights"):
                call()
        dt.set_weights(w)
        dt.kmeans_step(C0, weighted=True)
        dt.set_weights(None)
        with pytest.raises(ValueError, match="no weights"):
            dt.kmeans_step(C0, weighted=True)
    finally:
        dt.close()


@pytest.mark.parametrize("n,d,K", [(700, 5, 4), (600, 8, 256)])
def test_the_unweighted_step_keeps_its_bits(ctx, n, d, K):
    rng = np.random.default_rng(n)
    X = rng.standard_normal((n, d))
    w = np.exp(rng.standard_normal(n))
    C0 = X[:K].copy()
    dt = _block(ctx, X)

    def step():
        inertia, _, counts, cent = dt.kmeans_step(C0)
        return np.concatenate([[inertia], counts, cent.ravel(), dt.kmeans_labels().astype(np.float64), dt.kmeans_distances()])

    try:
        before = step()
        dt.set_weights(w)
        attached = step()
        dt.kmeans_step(C0, weighted=True)
        after_weighted_call = step()
        dt.set_weights(None)
        removed = step()
        assert np.array_equal(before, attached) and np.array_equal(before, after_weighted_call) and np.array_equal(before, removed)
        st = dt.kmeans_iterate(C0, 6)
        dt.set_weights(w)
        st_w = dt.kmeans_iterate(C0, 6)
        assert st[:3] == st_w[:3] and all(np.array_equal(a, b) for a, b in zip(st[3:], st_w[3:]))
    finally:
        dt.close()


# ---- iterate --------------------------------------------------------------------------------------------------------------------

def loop_of_weighted_steps(dt, C0, max_steps):
    """mlhip_kmeans_iterate's loop with absolute tolerance 0, restated over kmeans_step(weighted=True)."""
    cur, old = C0.copy(), np.zeros_like(C0)
    steps, converged = 0, False
    for step in range(max_steps):
        inertia, changed, counts, upd = dt.kmeans_step(cur, weighted=True)
        steps += 1
        if step > 0 and changed == 0:
            converged = True
            break
        old, cur = cur, upd
    return steps, converged, inertia, counts, cur, old


@pytest.mark.parametrize("n,d,K", [(500, 2, 3), (900, 8, 20)])
def test_iterate_equals_the_loop_of_weighted_steps(ctx, n, d, K):
    X, w, C0 = grid_case(n, d, K, seed=6)
    da, db = _block(ctx, X, w), _block(ctx, X, w)
    try:
        if (n, d, K) == (500, 2, 3):
            assert da.kmeans_route(K)["resident"]          # the unweighted call would take the one-launch loop; the weighted must not
        got = da.kmeans_iterate(C0, 200, weighted=True)
        want = loop_of_weighted_steps(db, C0, 200)
        assert got[:3] == want[:3], (got[:3], want[:3])
        assert got[1] and got[0] > 2
        for a, b in zip(got[3:], want[3:]):
            assert np.array_equal(a, b)
        assert np.array_equal(da.kmeans_labels(), db.kmeans_labels()) and np.array_equal(da.kmeans_distances(), db.kmeans_distances())
    finally:
        da.close(); db.close()


@pytest.mark.parametrize("n,d,K", [(500, 2, 3), (900, 8, 20)])
def test_iterate_equals_the_unweighted_iterate_on_replicated_rows(ctx, n, d, K):
    """Weights 1...7 here: n_changed counts ROWS, so a row of weight 0 that changes its label keeps the weighted loop going one trip
    longer than the loop on the replicated block, which does not hold that row."""
    X, w, C0 = grid_case(n, d, K, seed=7, low=1)
    R = replicate(X, w)
    dw, dr = _block(ctx, X, w), _block(ctx, R)
    try:
        steps_w, conv_w, inertia_w, counts_w, cent_w, old_w = dw.kmeans_iterate(C0, 200, weighted=True)
        steps_r, conv_r, inertia_r, counts_r, cent_r, old_r = dr.kmeans_iterate(C0, 200)
        assert (steps_w, conv_w) == (steps_r, conv_r) and conv_w and steps_w > 2
        assert np.array_equal(cent_w, cent_r) and np.array_equal(old_w, old_r) and np.array_equal(counts_w, counts_r)
        assert abs(inertia_w - inertia_r) <= 1e-13 * inertia_r
        first = np.concatenate([[0], np.cumsum(w.astype(np.int64))[:-1]])
        assert np.array_equal(dw.kmeans_labels(), dr.kmeans_labels()[first])
    finally:
        dw.close(); dr.close()


# ---- device group ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("empty_shard", [False, True])
def test_device_group_equals_the_single_context(ctx, empty_shard):
    from ml_amd import _lib
    n, d, K = 1000, 8, 5
    X, w, C0 = grid_case(n, d, K, seed=8)
    group = _lib.Context.group(3, device_ids=[0, 0, 0])
    try:
        dg = _lib.Data(group, X)
        if empty_shard:
            lo, cnt = dg.shard_rows(1)
            w[lo:lo + cnt] = 0.0                           # shard 1 holds rows of weight 0 only
        dg.set_weights(w)
        ds = _block(ctx, X, w)
        step_g, step_s = dg.kmeans_step(C0, weighted=True), ds.kmeans_step(C0, weighted=True)
        assert step_g[:2] == step_s[:2] and np.array_equal(step_g[2], step_s[2]) and np.array_equal(step_g[3], step_s[3])
        assert np.array_equal(dg.kmeans_labels(), ds.kmeans_labels())
        it_g, it_s = dg.kmeans_iterate(C0, 200, weighted=True), ds.kmeans_iterate(C0, 200, weighted=True)
        assert it_g[:2] == it_s[:2] and it_s[1]
        assert abs(it_g[2] - it_s[2]) <= 1e-13 * it_s[2]
        for a, b in zip(it_g[3:], it_s[3:]):
            assert np.array_equal(a, b)
        assert np.array_equal(dg.kmeans_labels(), ds.kmeans_labels())
        assign_g, assign_s = dg.kmeans_assign(it_s[4], weighted=True), ds.kmeans_assign(it_s[4], weighted=True)
        assert assign_g[1] == assign_s[1] and abs(assign_g[0] - assign_s[0]) <= 1e-13 * assign_s[0]
        ds.close()
        dg.close()
    finally:
        group.close()


# ---- Python facade --------------------------------------------------------------------------------------------------------------

def blobs_on_grid(n, seed):
    rng = np.random.default_rng(seed)
    centres = np.array([[-8.0, -8.0, 0.0, 4.0], [8.0, -4.0, 2.0, -6.0], [0.0, 9.0, -7.0, 1.0]])
    X = centres[rng.integers(0, 3, size=n)] + rng.integers(-2048, 2049, size=(n, 4)) / 1024.0
    w = rng.integers(0, 8, size=n).astype(np.float64)
    return np.ascontiguousarray(X), w, centres + 0.5


@pytest.mark.parametrize("inits", [1, 3])
def test_python_facade_against_replicated_rows(inits):
    """FixedCentroids on both sides (Forgy would draw different rows from the two samples); with three initialisations and a fixed
    seed the winner goes through the weighted assignment and the '<' on the sequential weighted inertia."""
    from ml_amd.cppyml import clustering
    X, w, start = blobs_on_grid(900, 11)
    R = replicate(X, w)

    def model():
        km = clustering.KMeans(3)
        km.set_centroids_initialiser(clustering.FixedCentroids(start))
        km.set_seed(5)
        if inits > 1:
            km.set_number_initialisations(inits)
        return km

    kw, kr = model(), model()
    assert kw.fit(X, sample_weight=w) and kr.fit(R)
    assert np.array_equal(kw.centroids, kr.centroids)
    assert abs(kw.inertia - kr.inertia) <= 1e-13 * kr.inertia
    sequential = 0.0
    labels, dist = kw.predict(X, return_distances=True)
    for wi, di in zip(w.tolist(), dist.tolist()):
        sequential += wi * di
    assert kw.inertia == sequential
    assert len(kw.labels) == len(X) and np.array_equal(kw.labels_array, labels)
    assert np.array_equal(labels, kr.predict(X))
    # the same object, unweighted again: the fit of a fresh object
    fresh = model()
    assert kw.fit(X) and fresh.fit(X)
    assert np.array_equal(kw.centroids, fresh.centroids) and kw.inertia == fresh.inertia and kw.labels == fresh.labels


def test_python_facade_forgy_initialisations_keep_the_lowest_weighted_inertia():
    """Forgy draws rows, so its fits of X and of the replicated block start differently and cannot be compared; what holds on the
    weighted side alone is the reference's own property (same seed: the first of three initialisations is the single fit, and the
    winner is chosen by '<' on the sequential weighted inertia)."""
    from ml_amd.cppyml import clustering
    X, w, _ = blobs_on_grid(900, 13)
    one, three = clustering.KMeans(3), clustering.KMeans(3)
    one.set_seed(7)
    three.set_seed(7)
    three.set_number_initialisations(3)
    assert one.fit(X, sample_weight=w) and three.fit(X, sample_weight=w)
    assert three.inertia <= one.inertia
    labels, dist = three.predict(X, return_distances=True)
    sequential = 0.0
    for wi, di in zip(w.tolist(), dist.tolist()):
        sequential += wi * di
    assert three.inertia == sequential and np.array_equal(three.labels_array, labels)


def test_python_facade_verbose_loop_takes_the_weighted_step(capfd):
    from ml_amd.cppyml import clustering
    X, w, start = blobs_on_grid(400, 12)
    quiet, loud = clustering.KMeans(3), clustering.KMeans(3)
    for km in (quiet, loud):
        km.set_centroids_initialiser(clustering.FixedCentroids(start))
    loud.set_verbose(True)
    assert quiet.fit(X, sample_weight=w) and loud.fit(X, sample_weight=w)
    capfd.readouterr()
    assert np.array_equal(quiet.centroids, loud.centroids) and quiet.inertia == loud.inertia and quiet.steps_done == loud.steps_done


def test_python_facade_exact_fit_is_unchanged():
    from ml_amd.cppyml import clustering
    X = np.array([[0.0, 1.0], [2.0, 3.0], [4.0, 5.0]])
    a, b = clustering.KMeans(3), clustering.KMeans(3)
    assert a.fit(X, sample_weight=np.array([1.0, 0.0, 5.0])) and b.fit(X)
    assert np.array_equal(a.centroids, b.centroids) and a.labels == b.labels and a.inertia == b.inertia == 0.0
