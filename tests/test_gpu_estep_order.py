"""The matrix-core E-step's row-quad-major block order (device/em_estep_mfma4.hip, the FOLD lw-only form at D = 24 and 32, 128 samples
per wave) against the column-quad-major order it replaces there (MLHIP_ESTEP_ORDER=column): every accumulator receives the same
products in the same order and q the same squares through the same fma chain, so everything an EM step returns and the
responsibilities it leaves behind are equal BIT FOR BIT -- np.array_equal, no tolerance. The switch is read per call: both orders run
in one process, each on a block of its own (the statistics route of a block depends on its call history). Which instantiation a
launch took is not visible through the C ABI; profiles/estep_rowmajor_kernel_stats.txt names the kernels of both settings."""
import numpy as np
import pytest

from ml_amd import _lib, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _problem(d, K, n, seed=3):
    mix = synth.Mixture(d, K, seed=seed)
    X, _ = mix.sample(n)
    cov = np.cov(X.T) if n > d + 1 else np.eye(d)
    return X, np.full(K, 1.0 / K), mix.initial_means(), np.stack([cov] * K)


def _step(ctx, X, pi0, mu0, S0):
    dt = _lib.Data(ctx, X)
    route = dt.em_route(len(pi0))
    out = dt.em_step(pi0, mu0, S0)
    resp = dt.em_responsibilities(len(pi0))
    dt.close()
    return route, out, resp


def _both_orders(ctx, monkeypatch, X, pi0, mu0, S0, env=None):
    """(route, em_step's outputs, responsibilities) under the default order after the two have been found equal to the column order's."""
    for name, value in (env or {}).items():
        monkeypatch.setenv(name, value)
    monkeypatch.delenv("MLHIP_ESTEP_ORDER", raising=False)
    route, got, resp = _step(ctx, X, pi0, mu0, S0)
    monkeypatch.setenv("MLHIP_ESTEP_ORDER", "column")
    route_c, want, resp_c = _step(ctx, X, pi0, mu0, S0)
    monkeypatch.delenv("MLHIP_ESTEP_ORDER")
    assert route == route_c
    assert route["estep"] == "matrix4"
    assert np.isfinite(want[0]) and all(np.all(np.isfinite(a)) for a in want[1:]) and np.all(np.isfinite(resp_c))
    assert got[0] == want[0]
    for a, b in zip(got[1:], want[1:]):
        assert np.array_equal(a, b)
    assert np.array_equal(resp, resp_c)
    return route, got, resp


def _assert_fold_lw_only(route):
    """The route on which the row-major form exists: FOLD allowed, the statistics kernel normalises (the E-step writes lw only)."""
    assert route["fold_allowed"] and route["self_norm"] and not route["fused"], route


# N = 1: a single row; 130: the second 64-sample half of the first wave partly padding; 300: two padded tiles
@pytest.mark.parametrize("n", [1, 130, 300])
def test_padded_tiles(ctx, monkeypatch, n):
    X, pi0, mu0, S0 = _problem(32, 5, max(n, 64))
    route, _, _ = _both_orders(ctx, monkeypatch, np.ascontiguousarray(X[:n]), pi0, mu0, S0)
    _assert_fold_lw_only(route)


# K >= 16 cuts the last, partial round of tiles into 8 component ranges; K = 17 makes them uneven
@pytest.mark.parametrize("K", [1, 3, 16, 17, 64])
def test_component_counts(ctx, monkeypatch, K):
    route, _, _ = _both_orders(ctx, monkeypatch, *_problem(32, K, 3000))
    _assert_fold_lw_only(route)


# more tiles (1 172) than resident workgroups: whole-tile rounds, then (K = 16) the split tail
@pytest.mark.parametrize("K", [4, 16])
def test_more_tiles_than_workgroups(ctx, monkeypatch, K):
    route, _, _ = _both_orders(ctx, monkeypatch, *_problem(32, K, 300_000))
    _assert_fold_lw_only(route)


# d = 30 and 29 pad to D = 32; D = 24 has the form as well (d = 21 pads to it)
@pytest.mark.parametrize("d", [30, 29, 24, 21])
def test_dimensions(ctx, monkeypatch, d):
    route, _, _ = _both_orders(ctx, monkeypatch, *_problem(d, 6, 1500))
    _assert_fold_lw_only(route)


def test_fold_rejected_runs_the_exact_form(ctx, monkeypatch):
    """Tight covariances: W = 10 I against means whose distance from the data's centre is 6 per coordinate in the root mean square, so
    entries of W (mu - s) are above 64, the host rejects FOLD, and under either order the exact (column-major) kernel runs -- the
    bits of MLHIP_ESTEP_FOLD=0. (Every component keeps the rows around its mean: the step's outputs are finite.)"""
    X, pi0, mu0, _ = _problem(32, 6, 1500)
    S0 = np.stack([0.01 * np.eye(32)] * 6)
    assert np.max(np.abs(10.0 * (mu0 - X.mean(axis=0)))) > 2 * 64
    route, got, resp = _both_orders(ctx, monkeypatch, X, pi0, mu0, S0)
    _assert_fold_lw_only(route)
    _, exact, resp_exact = _both_orders(ctx, monkeypatch, X, pi0, mu0, S0, {"MLHIP_ESTEP_FOLD": "0"})
    assert got[0] == exact[0] and all(np.array_equal(a, b) for a, b in zip(got[1:], exact[1:])) and np.array_equal(resp, resp_exact)


def test_sparse_statistics_behind_it(ctx, monkeypatch):
    """A well-separated K = 64 mixture from its own covariances (nine responsibilities in ten are exactly 0) with the sparse statistics
    kernel behind the E-step."""
    X, pi0, mu0, _ = _problem(32, 64, 20_000)
    route, _, resp = _both_orders(ctx, monkeypatch, X, pi0, mu0, synth.Mixture(32, 64, seed=3).covs, {"MLHIP_MSTATS_SPARSE": "1"})
    _assert_fold_lw_only(route)
    assert route["sparse"] is True
    assert np.mean(resp == 0.0) > 0.5
