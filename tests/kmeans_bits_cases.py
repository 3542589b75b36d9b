"""The K-means family against its own recorded bits: the cases and the runner shared by tests/test_gpu_kmeans_bits.py and
tests/golden/make_kmeans_bits_golden.py. Only the public ml_amd._lib API is used.

Every route keeps the same exact arithmetic -- order-free integer limb sums, one rounding at the end, a fixed-order inertia tree --
so a call's results are a function of its inputs alone, and every n here is at most 9000: every grid is set by n, not by the number
of compute units. The fixture holds, per case, what each call returned and the CRC-32 of the labels and distances it left behind.
Arrays of more than 1024 elements (counts and centroids of the many-cluster cases) are recorded as the CRC-32 of their bytes."""
import contextlib
import os
import zlib

import numpy as np

# (name, d, K, n, environment switches, expected route) -- the smallest shapes at which each path is taken
STEP_CASES = [
    ("direct_8_copies", 3, 2, 2049, {}, {"kernel": "direct", "pad": False}),
    ("direct_2_copies", 8, 100, 2049, {"MLHIP_KMEANS": "valu"}, {"kernel": "direct", "pad": False}),
    ("direct_512_threads", 33, 3, 1025, {"MLHIP_KMEANS": "valu"}, {"kernel": "direct", "pad": False}),
    ("direct_sweep_2_dim_chunks", 8, 400, 3001, {"MLHIP_KMEANS": "valu"}, {"kernel": "direct", "pad": False}),
    ("matrix_lds_accumulators", 8, 32, 2049, {}, {"kernel": "matrix", "pad": False}),
    ("matrix_separate_sweep", 8, 300, 3001, {}, {"kernel": "matrix", "pad": False}),
    ("matrix_chunked_table", 64, 700, 600, {}, {"kernel": "matrix", "pad": False}),
    ("padded_copy", 6, 130, 400, {}, {"kernel": "matrix", "pad": True}),
    ("sweep_chunked_by_clusters", 2, 8000, 9000, {}, {"kernel": "matrix", "pad": True}),
    ("big_dim", 130, 3, 300, {}, {"kernel": "big_dim", "pad": False}),
    ("plain", 130, 3, 300, {"MLHIP_BIG_DIM": "0"}, {"kernel": "plain", "pad": False}),
]

# kmeans_iterate(c0, 60, 1e-12) at d = 2, K = 3, n = 4000: (name, switches, weighted, expected route)
ITERATE_SHAPE = (2, 3, 4000)
ITERATE_CASES = [
    ("iterate_resident", {}, False, {"kernel": "direct", "pad": False, "resident": True}),
    ("iterate_launches", {"MLHIP_RESIDENT": "0"}, False, {"kernel": "direct", "pad": False, "resident": False}),
    ("iterate_weighted", {}, True, {"kernel": "direct", "pad": False}),
]

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kmeans_bits.npz")


def make_inputs(d, K, n):
    """A seeded normal mixture (not on a grid), weights exp(N(0, 1)), K rows of X as the start (repeated where K > n)."""
    rng = np.random.default_rng(100003 * d + 101 * K + n)
    centres = 4.0 * rng.standard_normal((min(K, 8), d))
    X = np.ascontiguousarray(centres[rng.integers(0, len(centres), size=n)] + rng.standard_normal((n, d)))
    w = np.exp(rng.standard_normal(n))
    C0 = X[np.resize(rng.permutation(n), K)].copy()
    return X, w, C0


@contextlib.contextmanager
def switches(env):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _pin(a):
    a = np.ascontiguousarray(a)
    return a if a.size <= 1024 else np.uint32(zlib.crc32(a.tobytes()))


def _left_behind(dt, out, tag):
    out[tag + "/labels_crc"] = np.uint32(zlib.crc32(dt.kmeans_labels().tobytes()))
    out[tag + "/distances_crc"] = np.uint32(zlib.crc32(dt.kmeans_distances().tobytes()))


def _step(dt, C, out, tag, weighted):
    inertia, changed, counts, cent = dt.kmeans_step(C, weighted=weighted)
    out[tag + "/inertia"], out[tag + "/n_changed"] = np.float64(inertia), np.uint64(changed)
    out[tag + "/counts"], out[tag + "/centroids"] = _pin(counts), _pin(cent)
    _left_behind(dt, out, tag)
    return cent


def _assign(dt, C, out, tag, weighted):
    inertia, changed = dt.kmeans_assign(C, weighted=weighted)
    out[tag + "/inertia"], out[tag + "/n_changed"] = np.float64(inertia), np.uint64(changed)
    _left_behind(dt, out, tag)


def route_mismatch(dt, K, expected):
    route = dt.kmeans_route(K)
    return {k: (route[k], v) for k, v in expected.items() if route[k] != v}


def run_step_case(ctx, case):
    """{field: value} of one step case, and the route's differences from the expected one ({} when it is the expected route)."""
    from ml_amd import _lib
    name, d, K, n, env, expected = case
    X, w, C0 = make_inputs(d, K, n)
    out = {}
    with switches(env):
        dt = _lib.Data(ctx, X)
        try:
            wrong = route_mismatch(dt, K, expected)
            for weighted in (False, True):
                pre = name + ("/weighted_" if weighted else "/")
                if weighted:
                    dt.set_weights(w)
                C1 = _step(dt, C0, out, pre + "step1", weighted)
                C2 = _step(dt, C1, out, pre + "step2", weighted)      # (labels of step 1 on the device: the have_old path)
                _assign(dt, C2, out, pre + "assign", weighted)
        finally:
            dt.close()
    return out, wrong


def run_iterate_case(ctx, case):
    from ml_amd import _lib
    name, env, weighted, expected = case
    d, K, n = ITERATE_SHAPE
    X, w, C0 = make_inputs(d, K, n)
    out = {}
    with switches(env):
        dt = _lib.Data(ctx, X)
        try:
            if weighted:
                dt.set_weights(w)
            wrong = route_mismatch(dt, K, expected)
            steps, converged, inertia, counts, cent, old = dt.kmeans_iterate(C0, 60, 1e-12, weighted=weighted)
            out[name + "/steps"], out[name + "/converged"] = np.uint32(steps), np.bool_(converged)
            out[name + "/inertia"], out[name + "/counts"] = np.float64(inertia), _pin(counts)
            out[name + "/centroids"], out[name + "/old_centroids"] = _pin(cent), _pin(old)
            _left_behind(dt, out, name)
        finally:
            dt.close()
    return out, wrong


def all_cases():
    return [(c[0], run_step_case, c) for c in STEP_CASES] + [(c[0], run_iterate_case, c) for c in ITERATE_CASES]
