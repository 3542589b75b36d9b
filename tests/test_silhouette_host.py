"""The silhouette without a GPU: the long-double restatement (tests/silhouette_reference.py) against scikit-learn's values
(tests/golden/silhouette_*.npz, written by tests/golden/make_silhouette_golden.py), the library's closing arithmetic
(mlhip_silhouette_finish: device/silhouette_finish.hpp compiled for the host) against the restatement on the cases the definition
singles out, the new symbols and their argument checks, and the Python argument checks that come before any device work. CPU only."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import silhouette_reference as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# Largest |restatement - scikit-learn 1.7.2| over the five centred fixtures, measured when they were written: 1.89e-15 (the
# singletons case; the others 3.9e-16 .. 7.9e-16). The test allows ten times that plus the limit of the library's own arithmetic.
MEASURED_SKLEARN_DIFFERENCE = 1.89e-15


def fixtures():
    return sorted(glob.glob(os.path.join(GOLDEN, "silhouette_*.npz")))


def test_fixtures_exist():
    assert len(fixtures()) == 5


@pytest.mark.parametrize("path", fixtures(), ids=os.path.basename)
def test_restatement_matches_scikit_learn(path):
    g = np.load(path)
    X, labels = g["X"], g["labels"]
    assert np.max(np.abs(X.mean(axis=0))) < 1e-12            # centred: the expansion's cancellation is not what is measured
    s = ref.silhouette_samples(X, labels)
    limit = ref.silhouette_limit(X.shape[1], ref.chain_length(labels))[1]
    worst = float(np.max(np.abs(s - g["s"])))
    print(f"{os.path.basename(path)}: |restatement - sklearn| {worst:.3g}")
    assert worst <= 10 * MEASURED_SKLEARN_DIFFERENCE + limit
    counts = np.bincount(labels)
    assert np.all(g["s"][counts[labels] == 1] == 0) and np.all(s[counts[labels] == 1] == 0)


def sums_of(X, labels, i, K):
    """Row i's K sums of distances in long double, rounded to double: what the finishing function is given."""
    dist = np.sqrt(((X[i].astype(np.longdouble) - X.astype(np.longdouble)) ** 2).sum(axis=1))
    return np.array([float(dist[labels == c].sum()) for c in range(K)])


def test_finish_against_the_restatement():
    from ml_amd import _lib
    rng = np.random.default_rng(5)
    X = rng.normal(size=(40, 3))
    labels = rng.integers(0, 4, size=40) * 2 + 1              # labels 1, 3, 5, 7 of K = 10: the others unused
    labels[9] = 0                                            # a row alone in its cluster
    K = 10
    counts = np.bincount(labels, minlength=K)
    a_ref, b_ref, s_ref = ref.silhouette_parts(X, labels)
    for i in range(40):
        a, b, s = _lib.silhouette_finish(counts, labels[i], sums_of(X, labels, i, K))
        assert abs(a - a_ref[i]) <= 4 * ref.U * abs(a_ref[i]) and abs(b - b_ref[i]) <= 4 * ref.U * abs(b_ref[i])
        assert abs(s - s_ref[i]) <= 16 * ref.U
    assert _lib.silhouette_finish(counts, 0, sums_of(X, labels, 9, K))[::2] == (0.0, 0.0)     # singleton: a = 0, s = 0


def test_finish_conventions():
    from ml_amd import _lib
    # a = b = 0 gives 0 (not 0 / 0)
    assert _lib.silhouette_finish([3, 2], 0, [0.0, 0.0]) == (0.0, 0.0, 0.0)
    # unused labels are passed over, whatever stands in their sums
    assert _lib.silhouette_finish([2, 0, 4], 0, [3.0, -1.0, 8.0]) == (3.0, 2.0, (2.0 - 3.0) / 3.0)
    # the first minimum wins: b is the mean of cluster 1, equal to cluster 2's
    a, b, s = _lib.silhouette_finish([3, 2, 4], 0, [2.0, 6.0, 12.0])
    assert (a, b, s) == (1.0, 3.0, 2.0 / 3.0)
    # a NaN among the sums that enter reaches the result
    assert np.isnan(_lib.silhouette_finish([3, 2], 0, [np.nan, 1.0])[2]) and np.isnan(_lib.silhouette_finish([3, 2], 0, [1.0, np.nan])[2])
    for counts, own in (([3, 0], 0), ([0, 3], 0), ([3, 2], 2)):
        with pytest.raises(ValueError):
            _lib.silhouette_finish(counts, own, [1.0] * len(counts))


def test_symbols_and_null_arguments():
    from ml_amd import _lib
    lib = _lib.lib
    for name in ("mlhip_silhouette", "mlhip_silhouette_route", "mlhip_silhouette_finish", "mlpp_silhouette_samples",
                 "mlpp_em_number_parameters", "mlpp_em_bic", "mlpp_em_aic"):
        assert hasattr(lib, name), name
    tier = C.c_int()
    one = (C.c_double * 1)()
    assert lib.mlhip_silhouette(None, None, C.c_uint32(2), None, None, C.c_uint64(0), None, None, None) == _lib.E_INVALID_ARGUMENT
    assert lib.mlhip_silhouette_route(None, C.byref(tier)) == _lib.E_INVALID_ARGUMENT
    assert lib.mlhip_silhouette_finish(C.c_uint32(2), None, C.c_uint32(0), None, None, None, None) == _lib.E_INVALID_ARGUMENT
    assert lib.mlpp_silhouette_samples(None, C.c_uint64(0), C.c_uint32(1), None, C.c_uint32(2), None, C.c_uint64(0), one) == _lib.E_INVALID_ARGUMENT
    assert lib.mlpp_em_number_parameters(None, None) == _lib.E_INVALID_ARGUMENT


def test_python_argument_checks_come_before_device_work():
    from ml_amd.cppyml import clustering
    X = np.random.default_rng(0).normal(size=(6, 2))
    good = [0, 1, 0, 1, 0, 1]
    for call in (clustering.silhouette_samples, clustering.silhouette_score):
        with pytest.raises(TypeError):
            call(X, [0, 1, 1.5, 0, 1, 0])                      # labels that are not integers
        with pytest.raises(TypeError):
            call(X, np.array(good, dtype=np.float64))
        with pytest.raises(TypeError):
            call(X.astype(np.float32), good)
        with pytest.raises(ValueError):
            call(X, [0, 1, 0])                                 # a wrong number of labels
        with pytest.raises(ValueError):
            call(X, [0, -1, 0, 0, 0, 1])                       # a negative label
        with pytest.raises(ValueError):
            call(X, [2] * 6)                                   # one non-empty cluster
    for rows in ([6], [-1], [0, 7]):
        with pytest.raises(ValueError):
            clustering.silhouette_samples(X, good, rows=rows)
    for m in (0, 7, -1):
        with pytest.raises(ValueError):
            clustering.silhouette_score(X, good, sample_size=m)


def test_no_cpu_fallback():
    from ml_amd import _lib
    from ml_amd.cppyml import clustering
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    X = np.random.default_rng(0).normal(size=(6, 2))
    for call in (clustering.silhouette_samples, clustering.silhouette_score):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(X, [0, 1, 0, 1, 0, 1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        clustering.silhouette_score(X, [0, 1, 0, 1, 0, 1], sample_size=3)
