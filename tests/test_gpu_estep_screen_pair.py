"""The screened E-step after its candidate loop and its bucket loop became one (device/em_estep_screen.hip: the 256-sample, eight-wave
form stayed -- the 128-sample pair form was measured slower). A wave now ballots inside the loop that decides the
candidates, collects the 32 counts of its half and segment in one register -- lane kk holds component 32 * half + kk's -- and stores
them with one LDS write of the lanes below min(32, K - 32 * half). The cases put that write at its edges: one lane, 31, 32, the upper
half's first lane, all 64 components; counts of 0 and of 64 in both halves. Method and helpers: tests/estep_screen_cases.py -- every
case runs the same three passes with MLHIP_ESTEP_SCREEN=1 and =0 on fresh handles, compares everything em_step returns, the
responsibilities and the labels bit for bit, and asserts the route counts."""
import os

import numpy as np
import pytest

from estep_screen_cases import THREE, axis_means, both, mixture, placed, routes, set_screen, three_passes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from ml_amd import _lib
    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture(autouse=True)
def restore_switch():
    old = os.environ.get("MLHIP_ESTEP_SCREEN")
    yield
    set_screen(old)


@pytest.mark.parametrize("d", [12, 32])
@pytest.mark.parametrize("K", [1, 31, 32, 33, 64])
def test_counts_of_a_wave_in_one_write(ctx, d, K):
    # the lanes that store a count: lane 0 alone (K = 1), 31 lanes, the whole lower half with the upper half's waves storing nothing
    # (32), the upper half's lane 0 alone (33), every lane of both halves (64); 700 rows: two whole tiles and a partly filled one
    n = 700
    X, p = mixture(d, K, n, seed=2000 * d + K)
    trail = both(ctx, X, three_passes(p))
    assert routes(trail) == THREE
    assert n <= trail[-1]["candidates"] <= K * n


def test_empty_and_full_buckets_in_both_halves(ctx):
    """K = 64, a row's only candidate is its own component. Per-segment counts inside a 256-sample tile: component 40 (upper half)
    (64, 64, 64, 64), a full bucket, in the first tile; in the second, component 0 (64, 0, 0, 0), component 63 (0, 1, 0, 0),
    components 31 and 32 -- the last lane of the lower half's count register and the first of the upper's -- (0, 0, 32, 0) each, and
    component 33 (0, 0, 0, 64), component 7 the rest of the second segment; every other component's count is 0 everywhere."""
    d, K = 32, 64
    tile0 = [[40] * 64] * 4
    tile1 = [[0] * 64, [63] + [7] * 63, [31] * 32 + [32] * 32, [33] * 64]
    rng = np.random.default_rng(31)
    comp = np.concatenate([rng.permutation(np.array(seg)) for tile in (tile0, tile1) for seg in tile])
    assert comp.shape == (512,)
    X, p = placed(axis_means(K, d), comp, seed=32)
    trail = both(ctx, X, three_passes(p))
    assert routes(trail) == THREE
    assert trail[1]["candidates"] == 512 and trail[2]["candidates"] == 512


def test_every_count_is_64(ctx):
    # 64 coincident components: every lane of every wave's count register holds 64 in the first tile, 44 rows remain for the second
    d, n, K = 12, 300, 64
    rng = np.random.default_rng(33)
    mu = 8.0 * rng.standard_normal((1, d))
    X = np.ascontiguousarray(mu + rng.standard_normal((n, d)))
    p = (np.full(K, 1.0 / K), np.repeat(mu, K, axis=0), np.stack([np.eye(d)] * K))
    trail = both(ctx, X, three_passes(p))
    assert routes(trail) == THREE
    assert trail[1]["candidates"] == K * n and trail[2]["candidates"] == K * n
