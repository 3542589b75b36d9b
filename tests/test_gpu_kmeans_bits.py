"""The K-means family against its own past: every route's step, second step (have_old), assignment, their weighted forms and the
step loop give the bits recorded in tests/golden/kmeans_bits.npz (tests/golden/make_kmeans_bits_golden.py, tests/kmeans_bits_cases.py).
Equality, no tolerance: the update sums are exact integer limb sums and the inertia is summed in a fixed order, so nothing here may
depend on the build. If a value differs, the library changed what it computes -- the fixture is not recorded again.
Needs a GPU: `timeout -k 10 600 pytest tests/test_gpu_kmeans_bits.py -m gpu -x`."""
import numpy as np
import pytest

import kmeans_bits_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from ml_amd import _lib
    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    with np.load(cases.FIXTURE) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize("name,run,case", cases.all_cases(), ids=[c[0] for c in cases.all_cases()])
def test_recorded_bits(ctx, golden, name, run, case):
    got, wrong_route = run(ctx, case)
    assert not wrong_route, wrong_route
    assert sorted(got) == sorted(k for k in golden if k.split("/")[0] == name)
    for key, value in got.items():
        want = golden[key]
        assert np.asarray(value).dtype == want.dtype and np.array_equal(value, want), (key, value, want)


def test_the_fixture_holds_no_other_case(golden):
    assert {k.split("/")[0] for k in golden} == {c[0] for c in cases.all_cases()}
