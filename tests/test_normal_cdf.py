"""mlhip_normal_cdf and mlhip_normal_quantile (ml_amd/csrc/device/normal_cdf.hpp compiled for the host; no GPU) against mpmath at 40
digits.

normal_cdf: the grid covers a in [-38, 9] -- 47 001 evenly spaced points, 4 001 more across [-0.01, 0.01], 2 001 each across the
places where the one-range form changes behaviour: 0 (the reflection), [-37.6, -37.4] (the result leaves the normal numbers) and
[8.2, 8.4] (1 - Phi(-a) becomes 1); the form has no other joints --, and a handful of tiny arguments either side of 0. The
relative error is asserted at TWICE the maximum measured on this grid when the header's figure was taken (MEASURED below, the number in
normal_cdf.hpp and DESIGN.md 4.1) wherever the exact result is a normal number; below 2^-1022 the format has no relative accuracy
left and the error is held to twice the measured number of subnormal spacings. Monotone over the sorted grid; the special values.

normal_quantile: Phi(Phi^-1(p)) against p for p from 1e-300 to 1 - 2^-53 within what one rounding of z allows on top of the CDF's
bound; odd about 0.5; +0.0 at 0.5."""
import mpmath as mp
import numpy as np
import pytest

from ml_amd import _lib

MEASURED = 6.01e-16          # max relative error of normal_cdf on the grid, normal results
MEASURED_SUBNORMAL = 1.84    # max error below 2^-1022, in spacings of 2^-1074
TINY = 2.0 ** -1022


def grid():
    parts = [np.linspace(-38.0, 9.0, 47001), np.linspace(-0.01, 0.01, 4001), np.linspace(-37.6, -37.4, 2001), np.linspace(8.2, 8.4, 2001),
             np.array([0.0, -0.0, 1e-300, -1e-300, 1e-17, -1e-17, 1e-9, -1e-9, 2.0 ** -1074, -2.0 ** -1074])]
    return np.sort(np.concatenate(parts))


@pytest.fixture(scope="module")
def measured():
    mp.mp.dps = 40
    a = grid()
    F = _lib.normal_cdf(a)
    exact = [mp.ncdf(mp.mpf(float(x))) for x in a]
    return a, F, exact


def test_normal_cdf_against_forty_digits(measured):
    a, F, exact = measured
    worst, at, worst_sub = 0.0, None, 0.0
    for x, f, e in zip(a, F, exact):
        err = abs(mp.mpf(float(f)) - e)
        if e >= TINY:
            rel = float(err / e)
            if rel > worst:
                worst, at = rel, x
        else:
            worst_sub = max(worst_sub, float(err / mp.mpf(2) ** -1074))
    print("normal_cdf: max relative error %.3e (%.2f ulp) at a = %r; below 2^-1022: %.2f spacings" % (worst, worst / 2.0 ** -53, at, worst_sub))
    assert worst <= 2 * MEASURED
    assert worst_sub <= 2 * MEASURED_SUBNORMAL


def test_normal_cdf_does_not_step_down(measured):
    a, F, _ = measured
    assert (np.diff(F) >= 0).all()
    assert (F >= 0).all() and (F <= 1).all()


def test_normal_cdf_special_values():
    F = _lib.normal_cdf([-np.inf, np.inf, np.nan, 0.0, -0.0, -40.0, 40.0, -1e308, 1e308])
    assert F[0] == 0.0 and F[1] == 1.0 and np.isnan(F[2]) and F[3] == 0.5 and F[4] == 0.5
    assert F[5] == 0.0 and F[6] == 1.0 and F[7] == 0.0 and F[8] == 1.0
    assert _lib.normal_cdf(np.empty(0)).shape == (0,)
    a = np.linspace(-3, 3, 12).reshape(3, 4)
    assert _lib.normal_cdf(a).shape == (3, 4)


def test_normal_quantile_round_trip():
    """z = Phi^-1(p) is a double: rounding it moves Phi by phi(z) ulp(z) / 2 <= Phi |z| (|z| + 1 / |z|) 2^-53 in the lower tail (Mills: phi / Phi <= |z| +
    1 / |z|), phi(z) |z| 2^-53 elsewhere; the CDF's own error 2 MEASURED beside it, and as much for the Halley steps' last evaluation."""
    p = np.unique(np.concatenate([10.0 ** -np.arange(300.0, 0.0, -1.0), np.linspace(0.001, 0.999, 999), 1 - 2.0 ** -np.arange(11.0, 54.0)]))
    z = _lib.normal_quantile(p)
    assert np.isfinite(z).all() and (np.diff(z) > 0).all()
    back = _lib.normal_cdf(z)
    lower = np.minimum(p, 1 - p)
    allowed = 4 * MEASURED * p + (z * z + 1) * 2.0 ** -53 * lower * 2
    worst = np.max(np.abs(back - p) / allowed)
    print("normal_quantile round trip: worst %.3f of the allowance" % worst)
    assert (np.abs(back - p) <= allowed).all()
    mp.mp.dps = 40
    # and through the 40-digit Phi instead of the library's own: the quantile is not merely the inverse of the CDF's errors
    for q, zq in zip(p[::37], z[::37]):
        tail = mp.mpf(float(min(q, 1 - q)))
        exact = mp.ncdf(mp.mpf(float(zq))) if q < 0.5 else mp.ncdf(-mp.mpf(float(zq)))
        assert abs(exact - (mp.mpf(float(q)) if q < 0.5 else 1 - mp.mpf(float(q)))) <= tail * (4 * MEASURED + (float(zq) ** 2 + 1) * 2.0 ** -52), q


def test_normal_quantile_is_odd_about_a_half():
    assert _lib.normal_quantile([0.5])[0] == 0.0 and not np.signbit(_lib.normal_quantile([0.5])[0])
    p = np.concatenate([np.arange(1, 512) / 1024.0, 2.0 ** -np.arange(2.0, 53.0)])      # 1 - p is exact: equal bits
    assert np.array_equal(_lib.normal_quantile(p), -_lib.normal_quantile(1 - p))
    # 1 - p rounds: Phi^-1(1 - p) is taken at a probability up to 2^-54 off -- a shift of 2^-54 / phi(z) in z
    p = 10.0 ** -np.arange(1.0, 16.0)
    z, mirrored = _lib.normal_quantile(p), -_lib.normal_quantile(1 - p)
    phi = np.exp(-z * z / 2) / np.sqrt(2 * np.pi)
    assert (np.abs(z - mirrored) <= 2.0 ** -53 / phi + 4 * np.spacing(np.abs(z))).all()


def test_normal_quantile_rejects_what_is_not_a_probability():
    for bad in (0.0, 1.0, -0.5, 1.5, np.nan, np.inf):
        with pytest.raises(ValueError):
            _lib.normal_quantile([0.25, bad])
