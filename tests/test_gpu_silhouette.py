"""mlhip_silhouette, _lib.silhouette and clustering.silhouette_samples / silhouette_score on the device against the long-double
restatement of the definition (tests/silhouette_reference.py).

Accuracy: every case asserts the limit of DESIGN.md 4.1 with no further tolerance -- |s^ - s| <= 3 E + 3 u, a and b within E + 2 u
relative, E = ((d + 2) / 2 + 2 + L) u, L the chunk length plus the chunks of the largest cluster (plus the shards of a group) -- and
prints the worst error as a fraction of that limit.

Bitwise: the register tier against the plain tier, the two column feeds, two grids, two row-block sizes, rows=None against the same
rows listed, a weighted handle against the unweighted one. Then device groups (within the limit: their bits depend on the shard
layout), the score, and labels of KMeans and EM going straight in."""
import numpy as np
import pytest

import silhouette_reference as ref

pytestmark = pytest.mark.gpu

SWITCHES = ("MLHIP_SILHOUETTE", "MLHIP_SILHOUETTE_FEED", "MLHIP_SILHOUETTE_ROWS", "MLHIP_SILHOUETTE_GRID")


@pytest.fixture(scope="module")
def ctx():
    from ml_amd import _lib
    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def blobs(n, d, K, seed, shift=0.0):
    """n rows around K centres, every label in [0, K) drawn at random (a label may stay unused)."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(K, d)) * 4
    labels = rng.integers(0, K, size=n)
    if n >= 2 and len(np.unique(labels)) < 2:
        labels[0], labels[1] = 0, 1 % K
    X = np.ascontiguousarray(centres[labels] + rng.normal(size=(n, d)) + shift)
    return X, labels


def evaluate(context, X, labels, rows=None, K=None, weights=None):
    from ml_amd import _lib
    data = _lib.Data(context, X)
    try:
        if weights is not None:
            data.set_weights(weights)
        return _lib.silhouette(data, labels, K=K, rows=rows, parts=True)
    finally:
        data.close()


def check(name, got, X, labels, rows=None, shards=1):
    want = ref.silhouette_parts(X, labels, rows)
    ratios = ref.worst_ratios(*got, want, X.shape[1], ref.chain_length(labels, shards))
    print(f"silhouette {name}: worst error / limit  a {ratios[0]:.3f}  b {ratios[1]:.3f}  s {ratios[2]:.3f}")
    assert max(ratios) <= 1.0, (name, ratios)
    return max(ratios)


@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 257, 1000])
def test_sizes(ctx, n):
    X, labels = blobs(n, 5, min(3, n), seed=n)
    check(f"N={n}", evaluate(ctx, X, labels), X, labels)


def test_cluster_spans_three_chunks_and_a_remainder(ctx):
    n0 = 3 * ref.CHUNK + 5
    X, _ = blobs(n0 + 40, 3, 2, seed=7)
    labels = np.array([0] * n0 + [1] * 40)
    np.random.default_rng(1).shuffle(labels)
    assert ref.chain_length(labels) == ref.CHUNK + 4
    check("3 chunks + 5", evaluate(ctx, X, labels), X, labels)


def test_chunk_boundary_on_a_cluster_boundary(ctx):
    X, _ = blobs(ref.CHUNK + 300, 4, 2, seed=8)
    labels = np.array([0] * ref.CHUNK + [1] * 300)
    np.random.default_rng(2).shuffle(labels)
    check("boundary", evaluate(ctx, X, labels), X, labels)


@pytest.mark.parametrize("d", [1, 2, 5, 16, 17, 31, 32, 33, 100])
def test_dimensions(ctx, d):
    from ml_amd import _lib
    X, labels = blobs(257, d, 3, seed=100 + d)
    data = _lib.Data(ctx, X)
    assert _lib.silhouette_route(data) == ("registers" if d <= 32 else "plain")
    got = _lib.silhouette(data, labels, parts=True)
    data.close()
    check(f"d={d}", got, X, labels)


@pytest.mark.parametrize("K", [2, 3, 17, 64, 65, 300])
def test_cluster_counts(ctx, K):
    X, labels = blobs(1000, 5, K, seed=200 + K)
    check(f"K={K}", evaluate(ctx, X, labels, K=K), X, labels)


def test_unused_labels_singletons_and_a_duplicate(ctx):
    X, labels = blobs(300, 6, 4, seed=31)
    labels = labels * 3 + 2                      # labels 2, 5, 8, 11 of K = 20: the others stay unused
    labels[7], labels[150] = 0, 19               # two rows alone in their clusters
    X[11] = X[10]                                # a duplicated row
    labels[11] = labels[10]
    a, b, s = evaluate(ctx, X, labels, K=20)
    check("unused / singleton / duplicate", (a, b, s), X, labels)
    assert s[7] == 0 and s[150] == 0 and a[7] == 0 and a[150] == 0
    assert bits(s[10]) == bits(s[11])


def test_every_row_its_own_cluster(ctx):
    X, _ = blobs(65, 3, 2, seed=32)
    a, b, s = evaluate(ctx, X, np.arange(65))
    assert not s.any() and not a.any() and (b > 0).all()


def test_identical_rows_give_zero(ctx):
    X = np.ones((10, 3))
    a, b, s = evaluate(ctx, X, np.arange(10) % 2)
    assert not a.any() and not b.any() and not s.any()


def test_shifted_by_1e8(ctx):
    X, labels = blobs(400, 5, 3, seed=33, shift=1e8)
    check("shift 1e8", evaluate(ctx, X, labels), X, labels)


def test_rows_subset_repeats_descending(ctx):
    X, labels = blobs(500, 7, 4, seed=34)
    everything = evaluate(ctx, X, labels)
    rows = np.array([499, 300, 300, 17, 5, 5, 0])
    got = evaluate(ctx, X, labels, rows=rows)
    check("rows", got, X, labels, rows=rows)
    for whole, part in zip(everything, got):
        assert np.array_equal(bits(whole[rows]), bits(part))
    listed = evaluate(ctx, X, labels, rows=np.arange(500))
    for whole, part in zip(everything, listed):
        assert np.array_equal(bits(whole), bits(part))


@pytest.mark.parametrize("d", [2, 5, 16, 32])
def test_tiers_and_feeds_give_the_same_bits(ctx, monkeypatch, d):
    X, labels = blobs(700, d, 3, seed=40 + d)
    base = evaluate(ctx, X, labels)
    monkeypatch.setenv("MLHIP_SILHOUETTE_FEED", "lds")
    lds = evaluate(ctx, X, labels)
    monkeypatch.delenv("MLHIP_SILHOUETTE_FEED")
    monkeypatch.setenv("MLHIP_SILHOUETTE", "plain")
    plain = evaluate(ctx, X, labels)
    for x, y, z in zip(base, lds, plain):
        assert np.array_equal(bits(x), bits(y)) and np.array_equal(bits(x), bits(z))


def test_grid_and_row_blocks_change_no_bit(ctx, monkeypatch):
    X, labels = blobs(1000, 5, 3, seed=45)
    base = evaluate(ctx, X, labels)
    for name, values in (("MLHIP_SILHOUETTE_GRID", ("1", "7")), ("MLHIP_SILHOUETTE_ROWS", ("256", "512"))):
        for v in values:
            monkeypatch.setenv(name, v)
            got = evaluate(ctx, X, labels)
            monkeypatch.delenv(name)
            for x, y in zip(base, got):
                assert np.array_equal(bits(x), bits(y)), (name, v)


def test_weights_play_no_part(ctx):
    X, labels = blobs(300, 5, 3, seed=46)
    w = np.random.default_rng(0).uniform(0.5, 2.0, size=300)
    for x, y in zip(evaluate(ctx, X, labels), evaluate(ctx, X, labels, weights=w)):
        assert np.array_equal(bits(x), bits(y))


@pytest.mark.parametrize("shards,n", [(3, 1000), (8, 5)])
def test_device_group(shards, n):
    from ml_amd import _lib
    X, labels = blobs(n, 5, 3 if n > 5 else 2, seed=50 + n)
    group = _lib.Context.group(shards, device_ids=[0] * shards)
    try:
        data = _lib.Data(group, X)
        if n == 1000:
            assert [data.shard_rows(s)[1] for s in range(3)] == [334, 333, 333]
        rows = None if n == 1000 else np.array([4, 0, 2, 2])
        got = _lib.silhouette(data, labels, rows=rows, parts=True)
        data.close()
    finally:
        group.close()
    check(f"group of {shards}", got, X, labels, rows=rows, shards=shards)


def test_argument_errors_before_any_launch(ctx):
    from ml_amd import _lib
    import ctypes as C
    X, labels = blobs(50, 3, 3, seed=60)
    data = _lib.Data(ctx, X)
    lab = np.ascontiguousarray(labels, dtype=np.uint32)
    s = np.empty(50)
    call = lambda K, lab, rows, m: _lib.lib.mlhip_silhouette(ctx.handle, data.handle, C.c_uint32(K), _lib.u32ptr(lab), rows, C.c_uint64(m), None, None, _lib.dptr(s))
    assert call(2, lab, None, 0) == _lib.E_INVALID_ARGUMENT                       # a label >= K
    bad = np.array([50], dtype=np.uint64)
    assert call(3, lab, bad.ctypes.data_as(C.POINTER(C.c_uint64)), 1) == _lib.E_INVALID_ARGUMENT
    assert call(3, np.zeros(50, dtype=np.uint32), None, 0) == _lib.E_INVALID_ARGUMENT   # one non-empty cluster
    assert call(3, lab, None, 0) == _lib.OK
    data.close()


def test_score_and_model_labels():
    from ml_amd.cppyml import clustering
    X, labels = blobs(600, 4, 3, seed=70)
    s = clustering.silhouette_samples(X, labels)
    want = ref.silhouette_samples(X, labels)
    assert np.max(np.abs(s.astype(np.longdouble) - want)) <= ref.silhouette_limit(4, ref.chain_length(labels))[1]
    total = 0.0
    for v in s.tolist():
        total += v
    assert clustering.silhouette_score(X, labels) == total / len(s)
    rows = np.sort(np.random.default_rng(3).choice(600, 50, replace=False))
    sub = clustering.silhouette_samples(X, labels, rows=rows)
    assert np.array_equal(bits(sub), bits(s[rows]))
    total = 0.0
    for v in sub.tolist():
        total += v
    assert clustering.silhouette_score(X, labels, sample_size=50, seed=3) == total / 50

    km = clustering.KMeans(3)
    km.set_seed(1)
    km.fit(X)
    assert isinstance(km.labels, list)
    s_km = clustering.silhouette_samples(X, km.labels)
    assert np.max(np.abs(s_km.astype(np.longdouble) - ref.silhouette_samples(X, km.labels))) <= ref.silhouette_limit(4, ref.chain_length(np.asarray(km.labels)))[1]
    em = clustering.EM(3)
    em.set_seed(1)
    em.fit(X)
    s_em = clustering.silhouette_samples(X, em.labels)
    assert np.max(np.abs(s_em.astype(np.longdouble) - ref.silhouette_samples(X, em.labels))) <= ref.silhouette_limit(4, ref.chain_length(np.asarray(em.labels)))[1]
