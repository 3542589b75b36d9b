"""FixedPointKPP (include/ML/Clustering.hpp) on the host: a pure-Python restatement of its rule -- the engine's canonical draws, an
exact fma and Python integers -- against the library's host init bit for bit, its sampling distribution, and the Python surfaces.
CPU only."""
import math
from fractions import Fraction

import numpy as np
import pytest

from ml_amd import _lib
from ml_amd.cppyml import clustering

_M = 2147483647          # std::minstd_rand0 (libstdc++'s std::default_random_engine): x <- 16807 x mod (2^31 - 1)


class Engine:
    """std::default_random_engine and std::generate_canonical<double, 53> as libstdc++ computes them (two engine calls per draw)."""

    def __init__(self, seed=None):
        self.x = 1 if seed is None or seed % _M == 0 else seed % _M

    def canonical(self):
        r = float(_M - 1)                       # max() - min() + 1
        total, scale = 0.0, 1.0
        for _ in range(2):
            self.x = self.x * 16807 % _M
            total += float(self.x - 1) * scale
            scale *= r
        u = total / scale
        return u if u < 1.0 else math.nextafter(1.0, 0.0)


def fma(a, b, c):
    """a * b + c rounded once (Python's int / int is correctly rounded)."""
    na, da = a.as_integer_ratio()
    nb, db = b.as_integer_ratio()
    nc, dc = c.as_integer_ratio()
    return (na * nb * dc + nc * da * db) / (da * db * dc)


def restated(X, K, seed=None):
    """The rule of FixedPointKPP, statement by statement."""
    n, d = X.shape
    rows = X.tolist()
    engine = Engine(seed)
    weights = [0.0] * n
    out = []
    for chosen in range(K):
        pick = 0
        if n >= 2:
            u = engine.canonical()
            total, q = 0, None
            if chosen > 0:
                c = out[chosen - 1]
                for i, x in enumerate(rows):
                    s = 0.0
                    for j in range(d):
                        t = x[j] - c[j]
                        s = fma(t, t, s)
                    w = s if chosen == 1 else min(weights[i], s)
                    if not math.isfinite(w):
                        raise ValueError("not finite")
                    weights[i] = w
                largest = max(weights)
                if largest > 0:
                    E = math.frexp(largest)[1]
                    q = [math.floor(Fraction(w) * Fraction(2) ** (52 - E)) for w in weights]
                    assert max(q) < 2 ** 52
                    total = sum(q)
            if total == 0:
                pick = math.floor(Fraction(u) * n)
            else:
                target = math.floor(Fraction(u) * total)
                cumulative = 0
                for i, qi in enumerate(q):
                    cumulative += qi
                    if cumulative > target:
                        pick = i
                        break
        out.append(rows[pick])
    return np.array(out, dtype=np.float64).reshape(K, d)


def test_engine_restatement_matches_the_library():
    # the first centroid is row floor(u N): with N = 2^16 the row index carries 16 bits of u
    n = 1 << 16
    X = np.arange(n, dtype=np.float64).reshape(n, 1)
    for seed in (None, 1, 5, 123456789):
        u = Engine(seed).canonical()
        got = clustering.FixedPointKPP()._run(X, 1, seed=seed)
        assert got[0, 0] == math.floor(Fraction(u) * n)


def _cases():
    rng = np.random.default_rng(2026)
    for case in range(60):
        n = int(rng.integers(1, 301)) if case >= 4 else (1, 2, 3, 300)[case]
        d = int(rng.integers(1, 6))
        K = int(rng.integers(1, min(n, 12) + 1)) if case % 5 else int(rng.integers(1, n + 1))
        X = rng.normal(size=(n, d)) * 10.0 ** rng.integers(-3, 4)
        if case % 3 == 0 and n > 4:                      # duplicate rows
            X[rng.integers(0, n, n // 2)] = X[rng.integers(0, n, n // 2)]
        if case % 7 == 0:                                # few distinct rows: T = 0 once they are all chosen
            X = X[rng.integers(0, min(n, 3), n)]
        if case % 11 == 0:                               # integer grid
            X = np.round(X)
        yield case, np.ascontiguousarray(X), K, int(rng.integers(0, 2 ** 31 - 1))


@pytest.mark.parametrize("case,X,K,seed", list(_cases()), ids=lambda v: None)
def test_host_init_equals_the_restated_rule(case, X, K, seed):
    got = clustering.FixedPointKPP()._run(X, K, seed=seed)
    want = restated(X, K, seed)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), case


def test_total_zero_picks_a_uniform_row():
    X = np.zeros((7, 3))
    X[:, 0] = [5.0] * 7                                  # all rows equal: every weight is 0 after the first centroid
    for seed in range(20):
        assert np.array_equal(clustering.FixedPointKPP()._run(X, 4, seed=seed), restated(X, 4, seed))
    # two distinct rows, K = 4: after both are chosen T = 0 and the draws fall back to floor(u N)
    Y = np.array([[0.0], [0.0], [1.0], [1.0], [1.0]])
    for seed in range(50):
        assert np.array_equal(clustering.FixedPointKPP()._run(Y, 4, seed=seed), restated(Y, 4, seed))


def test_single_row_and_no_draw():
    X = np.array([[1.5, -2.0]])
    assert np.array_equal(clustering.FixedPointKPP()._run(X, 3, seed=4), np.repeat(X, 3, axis=0))


def test_non_finite_weights_raise():
    X = np.arange(20, dtype=np.float64).reshape(10, 2)
    X[6, 1] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        clustering.FixedPointKPP()._run(X, 2, seed=3)
    assert clustering.FixedPointKPP()._run(X, 1, seed=3).shape == (1, 2)   # no weights, no check
    X[6, 1] = 1e300                                      # the squared distance overflows
    with pytest.raises(ValueError, match="not finite"):
        clustering.FixedPointKPP()._run(X, 2, seed=3)


# chi-square quantiles at 0.999 (4 and 15 degrees of freedom)
_CHI2_999 = {4: 18.467, 15: 37.697}


def test_draws_follow_the_d2_distribution():
    X = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 3.0], [2.0, 2.0], [-1.5, 0.5]])
    n = len(X)
    seeds = np.random.default_rng(7).integers(1, _M, 4000)
    first = np.zeros(n)
    second = np.zeros((n, n))
    init = clustering.FixedPointKPP()
    for s in seeds:
        c = init._run(X, 2, seed=int(s))
        a = int(np.flatnonzero((X == c[0]).all(axis=1))[0])
        b = int(np.flatnonzero((X == c[1]).all(axis=1))[0])
        first[a] += 1
        second[a, b] += 1
    expected = len(seeds) / n
    assert ((first - expected) ** 2 / expected).sum() < _CHI2_999[4]
    chi2 = 0.0
    for a in range(n):
        w = ((X - X[a]) ** 2).sum(axis=1)
        assert w[a] == 0 and second[a, a] == 0           # a row with q = 0 is never picked
        p = np.delete(w, a) / w.sum()
        obs = np.delete(second[a], a)
        exp = p * first[a]
        chi2 += ((obs - exp) ** 2 / exp).sum()
    assert chi2 < _CHI2_999[15]


def test_surfaces():
    from cppyml import clustering as alias
    from ml_amd.cppyml import clustering as direct
    assert alias.FixedPointKPP is direct.FixedPointKPP
    assert issubclass(direct.FixedPointKPP, direct.CentroidsInitialiser)
    assert direct.ClosestCentroid(direct.FixedPointKPP()) is not None
    for name in ("mlpp_fixed_point_kpp_create", "mlhip_kpp_draw_fixed_point"):
        assert hasattr(_lib.lib, name), name
