"""The sparse self-normalising statistics kernel (device/em_mstats_sparse.hip) against the dense one it stands in for
(em_mstats_wide.hip, EXP = 2): the same terms summed in another order. MLHIP_MSTATS_SPARSE=1 / 0 forces either kernel; without
it the runtime chooses from the nonzero count of the pass two passes back."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def relerr(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, np.max(np.abs(b)))


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


def _problem(d, K, n, seed, spread=6.0):
    rng = np.random.default_rng(seed)
    means = spread * rng.standard_normal((K, d))
    comp = rng.integers(0, K, n)
    X = np.ascontiguousarray(means[comp] + rng.standard_normal((n, d)))
    mu0 = means + 0.2 * rng.standard_normal((K, d))
    S0 = np.stack([np.eye(d)] * K)
    pi0 = np.full(K, 1.0 / K)
    return X, pi0, mu0, S0


def _step(ctx, X, pi, mu, S, m, mode, calls=1):
    from ml_amd import _lib
    mode(m)
    dt = _lib.Data(ctx, X)
    for _ in range(calls):
        out = dt.em_step(pi, mu, S)
    dt.close()
    return out


def _check_close(a, b):
    ll_a, pi_a, mu_a, S_a = a
    ll_b, pi_b, mu_b, S_b = b
    assert ll_a == ll_b                     # (max, sum of exponentials) come from the same staging code: bit-identical
    assert relerr(pi_a, pi_b) <= 1e-13
    assert relerr(mu_a, mu_b) <= 1e-13
    assert relerr(S_a, S_b) <= 1e-12


@pytest.mark.parametrize("d,K", [(16, 16), (16, 64), (32, 16), (32, 64), (64, 16), (64, 64)])
def test_one_step_sparse_vs_dense(ctx, mode, d, K):
    X, pi0, mu0, S0 = _problem(d, K, 200_000, seed=d * 100 + K)
    _check_close(_step(ctx, X, pi0, mu0, S0, "1", mode), _step(ctx, X, pi0, mu0, S0, "0", mode))


def test_sparse_reproducible(ctx, mode):
    X, pi0, mu0, S0 = _problem(32, 64, 200_000, seed=5)
    a = _step(ctx, X, pi0, mu0, S0, "1", mode)
    b = _step(ctx, X, pi0, mu0, S0, "1", mode)
    for u, v in zip(a, b):
        assert np.array_equal(np.asarray(u), np.asarray(v))


def test_ragged_n_and_empty_component(ctx, mode):
    # N not a multiple of the 64-sample tile; component 0's start is far from every sample: no responsibility of it survives
    X, pi0, mu0, S0 = _problem(24, 40, 200_003, seed=9)
    mu0 = mu0.copy()
    mu0[0] = 1e3
    a = _step(ctx, X, pi0, mu0, S0, "1", mode)
    b = _step(ctx, X, pi0, mu0, S0, "0", mode)
    assert a[0] == b[0]
    assert a[1][0] == 0.0 and b[1][0] == 0.0
    assert relerr(a[1], b[1]) <= 1e-13
    assert relerr(a[2][1:], b[2][1:]) <= 1e-13
    assert relerr(a[3][1:], b[3][1:]) <= 1e-12


def test_auto_choice(ctx, mode):
    from ml_amd import _lib
    # overlapping mixture: every responsibility nonzero, the runtime keeps the dense kernel -> the dense bits on every call
    X, pi0, mu0, S0 = _problem(32, 64, 100_000, seed=3, spread=0.05)
    for u, v in zip(_step(ctx, X, pi0, mu0, S0, None, mode, calls=4), _step(ctx, X, pi0, mu0, S0, "0", mode, calls=4)):
        assert np.array_equal(np.asarray(u), np.asarray(v))
    # separated mixture: dense for the first two passes of a handle, sparse from the third on
    X, pi0, mu0, S0 = _problem(32, 64, 100_000, seed=4)
    mode(None)
    dt = _lib.Data(ctx, X)
    auto = [dt.em_step(pi0, mu0, S0) for _ in range(3)]
    dt.close()
    dense = _step(ctx, X, pi0, mu0, S0, "0", mode)
    sparse = _step(ctx, X, pi0, mu0, S0, "1", mode)
    for u, v in zip(auto[0], dense):
        assert np.array_equal(np.asarray(u), np.asarray(v))
    for u, v in zip(auto[2], sparse):
        assert np.array_equal(np.asarray(u), np.asarray(v))


def test_iterate_sparse_vs_dense(ctx, mode):
    from ml_amd import _lib
    X, pi0, mu0, S0 = _problem(32, 64, 200_000, seed=12)
    res = {}
    for m in ("1", "0"):
        mode(m)
        dt = _lib.Data(ctx, X)
        res[m] = dt.em_iterate(pi0, mu0, S0, 10)
        dt.close()
    s, dn = res["1"], res["0"]
    assert s[0] == dn[0] == 10
    assert abs(s[2] - dn[2]) <= 1e-13 * abs(dn[2])
    for u, v in zip(s[3:6], dn[3:6]):
        assert relerr(u, v) <= 1e-12
