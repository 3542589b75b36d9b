"""EM in its three covariance modes against its own past: the per-step, loop, restarts and scoring entry points and the facade's
fit give the bits recorded in tests/golden/em_mode_bits.npz (tests/golden/make_em_mode_bits_golden.py, tests/em_mode_bits_cases.py)
before the covariance mode became one type from the C ABI to EM::fit. Equality, no tolerance: every n is small enough for the grids
to be set by n, and every host summation has one fixed order. If a value differs, the library changed what it computes -- the
fixture is not recorded again.
Needs a GPU: `timeout -k 10 600 pytest tests/test_gpu_em_mode_bits.py -m gpu -x`."""
import numpy as np
import pytest

import em_mode_bits_cases as cases

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
    assert {k.split("/")[0] for k in golden} == {c[0] for c in cases.all_cases()} | {"device"}
    assert golden["device/compute_units"].dtype == np.uint32 and golden["device/compute_units"] > 0
