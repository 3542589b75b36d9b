"""FixedPointKPP on the GPU (mlhip_kpp_draw_fixed_point): the device route picks the rows of the host rule bit for bit -- any d, N up
to 10^8, K up to 256, one GPU or a device group of any number of shards -- fits seeded with it are the fits seeded with its centroids,
and its seedings are as good as KPP's."""
import os
import subprocess
import sys
import textwrap
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _data(n, d, seed):
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(8, d)) * 5.0
    return np.ascontiguousarray(centres[rng.integers(0, 8, n)] + rng.normal(size=(n, d)))


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("n,d,K", [(100, 1, 60), (1000, 2, 256), (4097, 7, 64), (20000, 8, 256), (100000, 8, 128), (1000000, 8, 32),
                                   (30000, 32, 48), (8192, 64, 40), (5000, 130, 12)])
def test_device_route_equals_the_host_rule(n, d, K):
    from ml_amd.cppyml import clustering as cl
    X = _data(n, d, n + d)
    for seed in (1, 2024):
        host = cl.FixedPointKPP()._run(X, K, seed=seed)
        dev = cl.FixedPointKPP()._run_on_device(X, K, seed=seed)
        assert _same(host, dev), (n, d, K, seed)


def test_duplicates_zero_total_and_non_finite_weights_on_the_device():
    from ml_amd.cppyml import clustering as cl
    rng = np.random.default_rng(5)
    X = np.ascontiguousarray(rng.normal(size=(3, 4))[rng.integers(0, 3, 50000)])   # three distinct rows: T = 0 from centroid 4 on
    for seed in (3, 4, 5):
        assert _same(cl.FixedPointKPP()._run(X, 8, seed=seed), cl.FixedPointKPP()._run_on_device(X, 8, seed=seed))
    Y = _data(40000, 3, 9)
    Y[31234, 2] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        cl.FixedPointKPP()._run_on_device(Y, 4, seed=1)
    Y[31234, 2] = 1e300
    with pytest.raises(ValueError, match="not finite"):
        cl.FixedPointKPP()._run_on_device(Y, 4, seed=1)


def test_device_groups_of_one_two_and_three_shards_agree():
    from ml_amd import _lib
    from ml_amd.cppyml import clustering as cl
    X = _data(123457, 8, 77)
    want = cl.FixedPointKPP()._run(X, 64, seed=11)
    for shards in (1, 2, 3):
        grp = _lib.Context.group(shards, device_ids=[0] * shards)
        try:
            _lib.check(_lib.lib.mlpp_device_set_context(grp.handle))
            got = cl.FixedPointKPP()._run_on_device(X, 64, seed=11)
        finally:
            _lib.check(_lib.lib.mlpp_device_set_context(None))
            grp.close()
        assert _same(got, want), shards


GROUP_CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
import numpy as np
from ml_amd.cppyml import clustering as cl
X = np.load(sys.argv[1])
np.save(sys.argv[2], cl.FixedPointKPP()._run_on_device(X, 48, seed=19))
"""


def test_default_context_as_a_three_shard_group(tmp_path):
    from ml_amd.cppyml import clustering as cl
    X = _data(90001, 5, 3)
    np.save(tmp_path / "x.npy", X)
    env = dict(os.environ, MLHIP_NUM_GPUS="3")
    env.pop("LOCAL_RANK", None)
    env.pop("MLHIP_DEVICES", None)
    p = subprocess.run([sys.executable, "-c", GROUP_CHILD % {"root": ROOT}, str(tmp_path / "x.npy"), str(tmp_path / "c.npy")], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert _same(np.load(tmp_path / "c.npy"), cl.FixedPointKPP()._run(X, 48, seed=19))


def test_fits_seeded_with_fixed_point_kpp_are_the_fits_from_its_centroids():
    from ml_amd import synth
    from ml_amd.cppyml import clustering as cl
    X, _ = synth.Mixture(6, 5, seed=13).sample(60000)
    K = 5
    start = cl.FixedPointKPP()._run_on_device(X, K, seed=42)

    a, b = cl.KMeans(K), cl.KMeans(K)
    a.set_centroids_initialiser(cl.FixedPointKPP())
    b.set_centroids_initialiser(cl.FixedCentroids(start))
    for km in (a, b):
        km.set_seed(42)
    assert a.fit(X) == b.fit(X)
    assert a.steps_done == b.steps_done and a.inertia == b.inertia
    assert np.array_equal(a.centroids, b.centroids) and np.array_equal(a.labels_array, b.labels_array)

    for closest in (False, True):
        a, b = cl.EM(K), cl.EM(K)
        if closest:                                  # the responsibilities route: ClosestCentroid(...) with maximise-first
            a.set_responsibilities_initialiser(cl.ClosestCentroid(cl.FixedPointKPP()))
            b.set_responsibilities_initialiser(cl.ClosestCentroid(cl.FixedCentroids(start)))
        else:
            a.set_means_initialiser(cl.FixedPointKPP())
            b.set_means_initialiser(cl.FixedCentroids(start))
        for em in (a, b):
            em.set_seed(42)
            em.set_maximise_first(closest)
            em.set_maximum_steps(30)
        assert a.fit(X) == b.fit(X)
        assert a.steps_done == b.steps_done and a.log_likelihood == b.log_likelihood
        assert np.array_equal(a.means, b.means) and np.array_equal(a.labels, b.labels)


def test_seeding_inertia_matches_kpp():
    from ml_amd import synth
    from ml_amd.cppyml import clustering as cl
    X, _ = synth.Mixture(8, 8, seed=3).sample(20000)

    def inertia(C):
        return ((X[:, None, :] - C[None, :, :]) ** 2).sum(-1).min(1).sum()

    fp = np.mean([inertia(cl.FixedPointKPP()._run_on_device(X, 32, seed=s)) for s in range(1, 11)])
    kpp = np.mean([inertia(cl.KPP()._run_on_device(X, 32, seed=s)) for s in range(1, 11)])
    assert abs(fp - kpp) <= 0.1 * kpp, (fp, kpp)


BIG_CHILD = r"""
import sys, time
sys.path.insert(0, %(root)r)
import numpy as np
from ml_amd.cppyml import clustering as cl
n, K = int(sys.argv[1]), int(sys.argv[2])
X = np.random.default_rng(1).random((n, 8))
t = time.perf_counter()
dev = cl.FixedPointKPP()._run_on_device(X, K, seed=7)
print("FixedPointKPP N=%%d d=8 K=%%d: %%.2f s (upload included)" %% (n, K, time.perf_counter() - t), flush=True)
if sys.argv[3] == "check":
    host = cl.FixedPointKPP()._run(X, K, seed=7)
    assert np.array_equal(host.view(np.uint64), dev.view(np.uint64))
    print("equal to the host rule")
"""


@pytest.mark.parametrize("K,check,bound", [(8, "check", None), (256, "time", 60.0)])
def test_hundred_million_rows(K, check, bound):
    t = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-c", BIG_CHILD % {"root": ROOT}, str(10 ** 8), str(K), check],
                       capture_output=True, text=True)
    wall = time.perf_counter() - t
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    if bound is not None:
        seconds = float(p.stdout.split(": ")[1].split(" s")[0])
        assert seconds < bound, (seconds, wall)
