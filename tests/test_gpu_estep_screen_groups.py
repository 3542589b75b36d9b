"""The screened E-step's evaluation two 16-entry groups at a time (device/em_estep_screen.hip: a step serves the bucket entries
first .. first + 31 of a component with one read of the record and two accumulator chains; a step with at most 16 entries left takes
the single-group path; an entry's segment is found without a branch; the cross-lane adds are lane swaps). The cases are the smallest
shapes at which that can go wrong: bucket sizes around the step's edges, steps whose groups lie in different 64-sample segments of the
bucket, and -- for the staging of D = 28 and 32, whose coordinates a tile ahead were built, measured slower and left out
-- workgroups that stage one, two or no further tile. Method and helpers: tests/estep_screen_cases.py -- every
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


def tile_of(buckets, fill, rng):
    """256 component indices in a random order: `count` rows of each (component, count), the rest the filler's."""
    rows = [c for c, count in buckets for _ in range(count)]
    assert len(rows) <= 256
    return rng.permutation(np.array(rows + [fill] * (256 - len(rows)), dtype=np.int64))


def test_bucket_sizes_around_the_step_edges(ctx):
    """A row's only candidate is its own component, so a component's bucket in a tile holds exactly its rows there. Buckets of 1 entry
    (one single-group step), 15, 16; 17, 31, 32 (one two-group step, the second group holding 1, 15, 16 entries); 33, 47, 48 (a
    two-group step, then a single group of 1, 15, 16); 49, 64 (two two-group steps); 65 (a single group after two steps); 128; 256,
    the whole tile; component 14 empty everywhere; component 15 fills the tiles. Component j < 14 has the j-th size. The fourteen
    buckets hold 802 rows, so they take four tiles, the full one among them; rows are in random order inside a tile, so buckets
    straddle the 64-sample segments as it falls."""
    d, K, fill = 12, 16, 15
    sizes = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 65, 128, 256]
    comp_of = {b: j for j, b in enumerate(sizes)}
    layout = [[256], [128, 65, 49], [64, 48, 47, 33, 32, 31, 1], [17, 16, 15]]
    assert sorted(b for t in layout for b in t) == sizes
    rng = np.random.default_rng(41)
    comp = np.concatenate([tile_of([(comp_of[b], b) for b in t], fill, rng) for t in layout])
    assert comp.shape == (1024,) and not np.any(comp == 14)
    for j, b in enumerate(sizes):
        assert np.sum(comp == j) == b
    X, p = placed(axis_means(K, d), comp, seed=42)
    trail = both(ctx, X, three_passes(p))
    assert routes(trail) == THREE
    assert trail[1]["candidates"] == 1024 and trail[2]["candidates"] == 1024


def test_steps_that_straddle_segments(ctx):
    """Per-segment counts of a bucket inside one tile. Component 0 (10, 10, 10, 10): both groups of its first step cross a segment
    boundary (entries 10 and 20, 30), its second step has 8 entries. Component 1 (16, 0, 17, 0) and component 2 (0, 0, 0, 33): the
    second group starts in a later segment than the first, and a single group follows. Component 3 fills the tile."""
    d, K, fill = 12, 4, 3
    segs = [[0] * 10 + [1] * 16 + [fill] * 38, [0] * 10 + [fill] * 54, [0] * 10 + [1] * 17 + [fill] * 37, [0] * 10 + [2] * 33 + [fill] * 21]
    rng = np.random.default_rng(43)
    comp = np.concatenate([rng.permutation(np.array(sg)) for sg in segs])
    assert comp.shape == (256,)
    X, p = placed(axis_means(K, d), comp, seed=44)
    trail = both(ctx, X, three_passes(p))
    assert routes(trail) == THREE
    assert trail[1]["candidates"] == 256 and trail[2]["candidates"] == 256


@pytest.mark.parametrize("n,d", [(70_000, 28), (70_000, 32), (257, 32), (513, 32)])
def test_staging_over_one_two_or_no_further_tile(ctx, n, d):
    # 70 000 rows are 274 tiles: on a 256-CU part some workgroups stage a second tile (its stored values loaded under the first), most
    # take one tile and load nothing ahead; 257 and 513 rows: the last tile holds one row, and no load goes past it
    K = 5
    X, p = mixture(d, K, n, seed=n + d)
    trail = both(ctx, X, three_passes(p))
    assert routes(trail) == THREE
    assert n <= trail[-1]["candidates"] <= K * n


def test_many_candidates_per_sample(ctx):
    # the plain mixture at the headline's d and K: buckets of every small size, samples that sit in several buckets
    d, K, n = 32, 64, 3000
    X, p = mixture(d, K, n, seed=45)
    trail = both(ctx, X, three_passes(p))
    assert routes(trail) == THREE
    assert n <= trail[-1]["candidates"] <= K * n
