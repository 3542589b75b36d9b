"""The covariance ridge on the GPU (mlhip_data_set_covariance_ridge): every M-step on a handle adds the
handle's ridge r to the diagonal of each covariance it forms, on every route alike.
Needs a GPU: `timeout -k 10 1200 pytest tests/test_gpu_ridge.py -m gpu -x -s`.

A. Exact identity, one step per route, r = 0 against r = 1e-3: the log-likelihood, the mixing weights, the means and every
   off-diagonal entry bit for bit, every diagonal entry (variance) == fp64(entry at r = 0) + r bit for bit.
B. The device closings of mlhip_em_iterate (register, LDS, panelled, diagonal, the one-launch resident loop) against the host
   closing at r = 1e-3, bit for bit -- the equality tests/test_gpu_close_big.py, test_gpu_resident.py and test_gpu_iterate.py hold
   at the default ridge.
C. Distance from the truth at r = 1e-3: the limits of tests/hp_limits.py unchanged, the extended-precision step (which carries no
   ridge) as the reference, the oracle's step (1e-15, taken off) as the yardstick; the library's covariances are compared with r
   taken off again in long double (_ridge_taken_off; hp_limits._ridge_off is fixed at 1e-15 and stays).
D. The scikit-learn reg_covar = 1e-3 fixtures through Data.em_step / em_step_diag / em_step_tied, at the tolerances
   tests/test_gpu_abi_parity.py, test_gpu_diag.py and test_gpu_tied.py apply to their fixtures of the same mode.
E. The Python facade: EM.set_covariance_regularisation == the handle-level loop bit for bit; a sample with two collinear columns.

Both calls of a comparison take the same route: a fresh Data handle per call, the same switches, MLHIP_MSTATS_SPARSE pinned where
the statistics kernel runs (its automatic choice depends on the handle's call history). Each case asserts its route first."""
import contextlib
import os

import numpy as np
import pytest

from conftest import load_golden
from oracle import hp_cases
from oracle import hp_reference as hp
from oracle.hp_cases import problem, refinement_problem
from hp_limits import FOLD_BOUND, _errors, _report_and_check

pytestmark = pytest.mark.gpu

LD = np.longdouble
R = 1e-3


@pytest.fixture(scope="module")
def ctx():
    from ml_amd import _lib
    c = _lib.Context()
    yield c
    c.close()


@contextlib.contextmanager
def _switches(env):
    keep = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _data(ctx, X, ridge=None, w=None):
    from ml_amd import _lib
    dt = _lib.Data(ctx, np.ascontiguousarray(X, dtype=np.float64))
    if w is not None:
        dt.set_weights(w)
    if ridge is not None:
        dt.set_covariance_ridge(ridge)
        assert dt.covariance_ridge == ridge
    return dt


def _launches(ctx, name):
    return ctx.timing_get(name)[1]


def _ridge_taken_off(S, ridge, diagonal):
    """The library's covariances (variances) with the handle's ridge taken off again, in long double."""
    S = np.asarray(S, dtype=LD)
    return S - LD(ridge) if diagonal else S - LD(ridge) * np.eye(S.shape[-1], dtype=LD)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _assert_relation(name, base, got, variances):
    """got (ridge R) against base (ridge 0), both (ll, mixing, means, covariances | variances | the one covariance)."""
    assert _same_bits(base[0], got[0]), (name, "log-likelihood", base[0], got[0])
    assert _same_bits(base[1], got[1]), (name, "mixing")
    assert _same_bits(base[2], got[2]), (name, "means")
    S0, S1 = np.asarray(base[3]), np.asarray(got[3])
    assert S0.shape == S1.shape and np.isfinite(S0).all(), name
    if variances:
        assert _same_bits(S1, S0 + np.float64(R)), (name, "variances")
        return
    d = S0.shape[-1]
    off = ~np.eye(d, dtype=bool)
    assert _same_bits(S0[..., off], S1[..., off]), (name, "off-diagonal entries")
    eye = np.eye(d, dtype=bool)
    assert _same_bits(S1[..., eye], S0[..., eye] + np.float64(R)), (name, "diagonal entries")
    assert (S1[..., eye] != S0[..., eye]).all(), name


def _assert_pooled_relation(name, base, got):
    """The composed tied route pools Sigma = sum_k pi_k (S_k + r I) as it always did -- nothing is subtracted or re-added --, so its
    diagonal is S_jj + r to the rounding of two K-term fp64 sums of positive terms and of sum_k pi_k = 1, not bit for bit: each sum is
    within (K + 1) 2^-53 of its exact value, sum_k pi_k within K 2^-53 of 1 -- together below 4 (K + 2) 2^-53 (S_jj + r). Everything
    the ridge does not enter stays bit for bit."""
    assert _same_bits(base[0], got[0]) and _same_bits(base[1], got[1]) and _same_bits(base[2], got[2]), name
    S0, S1, K = np.asarray(base[3]), np.asarray(got[3]), len(base[1])
    off = ~np.eye(S0.shape[0], dtype=bool)
    assert _same_bits(S0[off], S1[off]), (name, "off-diagonal entries")
    want = np.diag(S0).astype(LD) + LD(R)
    err = np.abs(np.diag(S1).astype(LD) - want) / want
    assert float(err.max()) <= 4 * (K + 2) * hp.EPS64, (name, float(err.max()))


def _subset(route, want):
    got = {k: route[k] for k in want}
    assert got == want, (got, want)


# ---- the cases of A and C: one step per route ---------------------------------------------------------------------------------

SPARSE0 = {"MLHIP_MSTATS_SPARSE": "0"}
# name, kind, (d, K, N, offset), switches, route
STEP_CASES = [
    ("fused vector-unit, d=2 K=3", "full", (2, 3, 3001, 0.0), {}, {"fused": True, "fused_form": "valu"}),
    ("fused scalar-feed, d=8 K=5", "full", (8, 5, 3001, 3.0), {}, {"fused": True, "fused_form": "scalar_feed"}),
    ("scalar-fed + split statistics, d=8 K=5", "full", (8, 5, 3001, 3.0), {"MLHIP_FUSED": "0"},
     {"estep": "scalar_fed", "fused": False, "self_norm": False}),
    ("matrix-core, self-normalising, d=16 K=8", "full", (16, 8, 4001, 2.0), SPARSE0, {"estep": "matrix4", "self_norm": True, "sparse": False}),
    ("matrix-core, split statistics, d=16 K=24", "full", (16, 24, 5001, 1.0), {"MLHIP_SELF_NORM": "0"}, {"estep": "matrix4", "self_norm": False}),
    ("matrix-core, d=128 K=3", "full", (128, 3, 2001, 0.0), SPARSE0, {"estep": "matrix4", "fold_allowed": False}),
    ("big-dim, d=192 K=2", "full", (192, 2, 1501, 0.0), {}, {"estep": "big_dim", "fused": False, "self_norm": False}),
    ("diagonal kernel, d=16 K=8", "diag", (16, 8, 4001, 0.5), {}, {"diag_kernel": True, "diag_exact": False}),
    ("diagonal kernel, d=7 K=40", "diag", (7, 40, 4001, 0.0), {}, {"diag_kernel": True, "diag_exact": False}),
    ("diagonal beyond the kernel, d=40 K=3", "diag", (40, 3, 2001, 0.0), SPARSE0, {"diag_kernel": False}),
    ("weighted, d=16 K=8", "weighted", (16, 8, 4001, 2.0), SPARSE0, {"estep": "matrix4", "self_norm": True, "fused": False, "sparse": False}),
    ("tied kernel, d=16 K=16", "tied", (16, 16, hp_cases.TIED_N), {"MLHIP_TIED": "kernel"}, "kernel"),
    ("tied composed, d=16 K=16", "tied", (16, 16, hp_cases.TIED_N), dict(SPARSE0, MLHIP_TIED="composed"), "composed"),
    ("weighted tied (composed), d=16 K=16", "weighted_tied", (16, 16, hp_cases.TIED_N), SPARSE0, "composed"),
]
STEP_IDS = [c[0] for c in STEP_CASES]


def _inputs(kind, shape):
    """(X, weights or None, pi0, mu0, S0)."""
    from test_weights_cases import case, weights
    if kind == "weighted":
        X, w, pi0, mu0, S0, _ = case(*shape)
        return X, w, pi0, mu0, S0
    if kind in ("tied", "weighted_tied"):
        X, pi0, mu0, S0 = hp_cases.tied_problem(*shape)
        return X, (weights(len(X)) if kind == "weighted_tied" else None), pi0, mu0, S0
    X, pi0, mu0, S0 = problem(*shape, diagonal=kind == "diag")
    return X, None, pi0, mu0, S0


_STEPS = {}


def _step(ctx, name, ridge):
    """One step of case `name` on a fresh handle with `ridge` -> ((ll, mixing, means, covariances), the route taken, launches of
    em_refine); run once per (case, ridge) and shared by A and C."""
    if (name, ridge) in _STEPS:
        return _STEPS[(name, ridge)]
    _, kind, shape, env, route = STEP_CASES[STEP_IDS.index(name)]
    X, w, pi0, mu0, S0 = _inputs(kind, shape)
    K = len(pi0)
    with _switches(env):
        dt = _data(ctx, X, ridge, w)
        if kind in ("tied", "weighted_tied"):
            taken = dt.em_tied_route(K)
            assert taken == route, (taken, route)
        else:
            taken = dt.em_route(K, "diag" if kind == "diag" else "full")
            _subset(taken, route)
        ctx.timing_enable(True)
        ctx.timing_reset()
        fn = {"diag": dt.em_step_diag, "tied": dt.em_step_tied, "weighted_tied": dt.em_step_tied}.get(kind, dt.em_step)
        out = fn(pi0, mu0, S0)
        refined = _launches(ctx, "em_refine")
        ctx.timing_enable(False)
        dt.close()
    _STEPS[(name, ridge)] = (out, taken, refined)
    return _STEPS[(name, ridge)]


# ---- A. exact identity ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", STEP_IDS)
def test_step_adds_the_ridge_to_the_diagonal_and_nothing_else(ctx, name):
    kind = STEP_CASES[STEP_IDS.index(name)][1]
    base, _, refined0 = _step(ctx, name, 0.0)
    got, _, refined = _step(ctx, name, R)
    assert refined0 == refined == 0
    if kind in ("tied", "weighted_tied"):
        assert np.array_equal(got[3], got[3].T)
    if _step(ctx, name, R)[1] == "composed":
        _assert_pooled_relation(name, base, got)
    else:
        _assert_relation(name, base, got, kind == "diag")


@pytest.mark.parametrize("d", [8, 32])
def test_a_refined_component_carries_the_ridge_alike(ctx, d):
    X, pi0, mu0, S0 = refinement_problem(d, 2e4)
    outs = []
    for ridge in (0.0, R):
        with _switches(SPARSE0):
            dt = _data(ctx, X, ridge)
            ctx.timing_enable(True)
            ctx.timing_reset()
            outs.append(dt.em_step(pi0, mu0, S0))
            assert _launches(ctx, "em_refine") == 1
            ctx.timing_enable(False)
            dt.close()
    _assert_relation(f"refinement d={d}", outs[0], outs[1], False)


def test_device_group_of_two_shards(ctx):
    from ml_amd import _lib
    X, pi0, mu0, S0 = problem(16, 8, 4001, 2.0)
    group = _lib.Context.group(2, device_ids=[0, 0])
    outs = []
    with _switches(SPARSE0):
        for ridge in (0.0, R):
            gd = _lib.Data(group, X)
            assert gd.covariance_ridge == 1e-15
            gd.set_covariance_ridge(ridge)
            assert gd.covariance_ridge == ridge                         # the group's handle mirrors its parts
            _subset(gd.em_route(len(pi0)), {"estep": "matrix4", "self_norm": True, "sparse": False})
            outs.append(gd.em_step(pi0, mu0, S0))
            for bad in (float("nan"), float("inf"), -1e-3):
                with pytest.raises(ValueError):
                    gd.set_covariance_ridge(bad)
                assert gd.covariance_ridge == ridge
            gd.close()
    group.close()
    _assert_relation("group of two shards", outs[0], outs[1], False)
    # ... and the group's sums are the single context's to rounding: the ridge arrives in every shard
    one = _step(ctx, "matrix-core, self-normalising, d=16 K=8", R)[0]
    assert np.max(np.abs(outs[1][3] - one[3])) <= 1e-11 * np.max(np.abs(one[3]))


def test_setting_the_ridge_drops_nothing_and_touches_no_given_parameter(ctx):
    """E-step results stay valid across mlhip_data_set_covariance_ridge; the M-step entry points read it; the E-step, the score and
    the sample covariance do not; a refused value leaves the handle as it was."""
    X, pi0, mu0, S0 = problem(8, 5, 3001, 3.0)
    K = len(pi0)
    with _switches({"MLHIP_FUSED": "0"}):
        dt = _data(ctx, X)
        assert dt.covariance_ridge == 1e-15
        _, cov = dt.sample_covariance()
        dens = dt.em_score(pi0, mu0, S0)[0]
        ll = dt.em_expectation(pi0, mu0, S0)
        dt.set_covariance_ridge(0.0)
        base = (ll,) + tuple(dt.em_maximisation(K))
        resp, labels = dt.em_responsibilities(K), dt.em_labels(K)
        dt.set_covariance_ridge(R)                                      # the E-step's results are still there
        got = (ll,) + tuple(dt.em_maximisation(K))
        _assert_relation("maximisation", base, got, False)
        for bad in (float("nan"), float("inf"), -float("inf"), -1e-3):
            with pytest.raises(ValueError):
                dt.set_covariance_ridge(bad)
            assert dt.covariance_ridge == R
        assert _same_bits(dt.em_expectation(pi0, mu0, S0), ll)
        assert _same_bits(dt.em_score(pi0, mu0, S0)[0], dens)
        assert _same_bits(dt.sample_covariance()[1], cov)
        from_resp, from_labels = dt.em_maximisation_from(resp), dt.em_maximisation_from_labels(labels, K)
        dt.set_covariance_ridge(-0.0)                                   # counts as 0
        assert dt.covariance_ridge == 0.0 and not np.signbit(dt.covariance_ridge)
        _assert_relation("maximisation_from", (ll,) + tuple(dt.em_maximisation_from(resp)), (ll,) + tuple(from_resp), False)
        _assert_relation("maximisation_from_labels", (ll,) + tuple(dt.em_maximisation_from_labels(labels, K)), (ll,) + tuple(from_labels), False)
        dt.close()


# ---- B. the device closings against the host closing ---------------------------------------------------------------------------

# name, (d, K, N, offset), diagonal, switches of both calls, route of the device call
CLOSE_CASES = [
    ("register closing, d=16", (16, 8, 4001, 2.0), False, dict(SPARSE0, MLHIP_RESIDENT="0"), {"device_close": True}),
    ("LDS closing, d=64", (64, 4, 3001, 3.0), False, SPARSE0, {"device_close": True, "records_on_device": False}),
    # (the first records on the host in both calls, as tests/test_gpu_close_big.py compares: the first log-likelihood sees them)
    ("panelled closing, d=72", (72, 2, 2501, 0.0), False, dict(SPARSE0, MLHIP_DEVICE_RECORDS="0"), {"device_close": True}),
    ("diagonal closing kernel, d=16", (16, 8, 4001, 0.5), True, {}, {"device_close": True, "diag_kernel": True}),
]
CLOSE_IDS = [c[0] for c in CLOSE_CASES]
_CLOSED = {}


def _closed_on_the_device(ctx, name):
    """One em_iterate step of case `name` at ridge R with the closing on the device (run once, shared by B and C)."""
    if name in _CLOSED:
        return _CLOSED[name]
    _, shape, diagonal, env, route = CLOSE_CASES[CLOSE_IDS.index(name)]
    X, pi0, mu0, S0 = problem(*shape, diagonal=diagonal)
    with _switches(env):
        dt = _data(ctx, X, R)
        _subset(dt.em_route(len(pi0), "diag" if diagonal else "full"), route)
        ctx.timing_enable(True)
        ctx.timing_reset()
        out = dt.em_iterate(pi0, mu0, S0, 1, 0.0, 0.0, diagonal)
        closes = _launches(ctx, "em_close")
        ctx.timing_enable(False)
        dt.close()
    assert out[0] == 1 and closes >= 1, (out[0], closes)
    _CLOSED[name] = out
    return out


@pytest.mark.parametrize("name", CLOSE_IDS)
def test_device_closing_equals_host_closing_at_the_ridge(ctx, name):
    _, shape, diagonal, env, _ = CLOSE_CASES[CLOSE_IDS.index(name)]
    X, pi0, mu0, S0 = problem(*shape, diagonal=diagonal)
    dev = _closed_on_the_device(ctx, name)
    with _switches(dict(env, MLHIP_DEVICE_CLOSE="0")):
        dt = _data(ctx, X, R)
        _subset(dt.em_route(len(pi0), "diag" if diagonal else "full"), {"device_close": False})
        ctx.timing_enable(True)
        ctx.timing_reset()
        host = dt.em_iterate(pi0, mu0, S0, 1, 0.0, 0.0, diagonal)
        assert _launches(ctx, "em_close") == 0
        ctx.timing_enable(False)
        dt.close()
    assert host[0] == 1 and _same_bits(dev[2], host[2])
    assert _same_bits(dev[3], host[3]) and _same_bits(dev[4], host[4]) and _same_bits(dev[5], host[5])
    # ... and the ridge is in them: against the same closing at ridge 0
    with _switches(env):
        dt = _data(ctx, X, 0.0)
        base = dt.em_iterate(pi0, mu0, S0, 1, 0.0, 0.0, diagonal)
        dt.close()
    _assert_relation(name, (base[2], base[3], base[4], base[5]), (dev[2], dev[3], dev[4], dev[5]), diagonal)


RESIDENT = (2, 3, 3001, 0.0)
_RESIDENT = {}


def _resident_run(ctx):
    if "out" not in _RESIDENT:
        X, pi0, mu0, S0 = problem(*RESIDENT)
        dt = _data(ctx, X, R)
        _subset(dt.em_route(3), {"fused": True, "fused_form": "valu", "resident": True, "device_close": True})
        ctx.timing_enable(True)
        ctx.timing_reset()
        out = dt.em_iterate(pi0, mu0, S0, 4)
        assert _launches(ctx, "em_resident") == 1 and _launches(ctx, "em_fused") == 0 and out[0] == 4
        ctx.timing_enable(False)
        dt.close()
        _RESIDENT["out"] = out
    return _RESIDENT["out"]


def test_resident_loop_equals_the_three_launch_loop_at_the_ridge(ctx):
    X, pi0, mu0, S0 = problem(*RESIDENT)
    got = _resident_run(ctx)
    with _switches({"MLHIP_RESIDENT": "0"}):
        dt = _data(ctx, X, R)
        _subset(dt.em_route(3), {"fused": True, "resident": False, "device_close": True})
        ctx.timing_enable(True)
        ctx.timing_reset()
        ref = dt.em_iterate(pi0, mu0, S0, 4)
        assert _launches(ctx, "em_resident") == 0 and _launches(ctx, "em_close") >= 4
        ctx.timing_enable(False)
        dt.close()
    assert got[0] == ref[0] == 4 and got[1] == ref[1] and _same_bits(got[2], ref[2]) and _same_bits(got[6], ref[6])
    for a, b in zip(got[3:6], ref[3:6]):
        assert _same_bits(a, b)
    # the ridge took part in every iteration: the trajectory is not the default's
    dt = _data(ctx, X)
    default = dt.em_iterate(pi0, mu0, S0, 4)
    dt.close()
    assert _same_bits(default[6][0], got[6][0]) and (default[6][1:] != got[6][1:]).all()


# ---- C. distance from the truth -----------------------------------------------------------------------------------------------------

def _full_refs(shape, diagonal):
    from test_gpu_hp_error import _diag_case, _full_case
    return (_diag_case if diagonal else _full_case)(*shape)


@pytest.mark.parametrize("name", STEP_IDS)
def test_step_error_at_the_ridge(ctx, name):
    _, kind, shape, _, _ = STEP_CASES[STEP_IDS.index(name)]
    (ll, pi1, mu1, S1), taken, refined = _step(ctx, name, R)
    if kind in ("tied", "weighted_tied"):
        from test_gpu_tied_hp import _as_stack, _check, _composed_ratio, _references
        X, w, pi0, mu0, S0 = _inputs(kind, shape)
        got = (ll, None, pi1, mu1, _ridge_taken_off(S1, R, False)[None])
        if w is None:
            refs = _references(X, pi0, mu0, S0)
        else:
            # as test_weighted_composed_step: the weighted reference, the oracle's step on the replicated sample as the yardstick
            from oracle import oracle_ctypes as orc
            counts = w.astype(np.int64)
            Xr = np.ascontiguousarray(np.repeat(X, counts, axis=0))
            ref = _as_stack(hp.em_step_tied(X, pi0, mu0, S0, w))
            no_resp = lambda s: (s[0], None) + tuple(s[2:])   # noqa: E731
            e_cpu = _errors(no_resp(_as_stack(hp_cases.oracle_tied_step(orc, Xr, pi0, mu0, S0))), no_resp(ref))
            shift = Xr.astype(LD).mean(axis=0)
            resp_r = np.repeat(ref[1], counts, axis=0)
            refs = (ref, e_cpu, hp.tied_conditioning(Xr, shift, mu0, S0, ref[4][0], resp=resp_r), _composed_ratio(Xr, shift, resp_r))
        _check(f"ridge 1e-3: {name}", taken, got, refined, refs, resp=False)
        return
    if kind == "weighted":
        from test_weights_cases import case, references
        X = case(*shape)[0]
        ref, cpu = references(*shape)
        ratio = hp.conditioning(X.astype(LD).mean(axis=0), ref[3], covs=ref[4])["ratio"]
        _report_and_check(f"ridge 1e-3: {name}", _errors((ll, None, pi1, mu1, _ridge_taken_off(S1, R, False)), ref),
                          dict(_errors(cpu, ref), resp=None), ratio)
        return
    diagonal = kind == "diag"
    X, pi0, mu0, S0, ref, e_cpu, ratio, old = _full_refs(shape, diagonal)
    model, model_name = None, ""
    if diagonal and taken["diag_kernel"] and not taken["diag_exact"]:
        from test_gpu_hp_error import _diag_model
        assert old["b2"].max() <= 64.0 ** 2
        model, model_name = _diag_model(X, mu0, S0), "2^-53 sum abs b"
    elif not diagonal and taken["estep"] == "matrix4" and taken["fold_allowed"] and old["fold"].max() <= 64:
        model, model_name = FOLD_BOUND, "FOLD"
    _report_and_check(f"ridge 1e-3: {name}", _errors((ll, None, pi1, mu1, _ridge_taken_off(S1, R, diagonal)), ref), dict(e_cpu, resp=None),
                      ratio, model, model_name, abs(float(ref[0])))


@pytest.mark.parametrize("name", CLOSE_IDS)
def test_closing_error_at_the_ridge(ctx, name):
    _, shape, diagonal, _, _ = CLOSE_CASES[CLOSE_IDS.index(name)]
    X, pi0, mu0, S0, ref, e_cpu, ratio, old = _full_refs(shape, diagonal)
    _, _, ll, pi1, mu1, S1, _ = _closed_on_the_device(ctx, name)
    model, model_name = None, ""
    if diagonal:
        from test_gpu_hp_error import _diag_model
        assert old["b2"].max() <= 64.0 ** 2
        model, model_name = _diag_model(X, mu0, S0), "2^-53 sum abs b"
    _report_and_check(f"ridge 1e-3, one iteration: {name}", _errors((ll, None, pi1, mu1, _ridge_taken_off(S1, R, diagonal)), ref),
                      dict(e_cpu, resp=None), ratio, model, model_name, abs(float(ref[0])))


def test_resident_loop_error_at_the_ridge(ctx):
    """The one-launch loop at r = 1e-3: the end of 4 iterations against 4 reference steps, each fed the previous one's
    extended-precision parameters + r I as the library adds it -- the pattern of test_resident_em_loop_error, whose oracle yardstick
    carries the oracle's hard-wired 1e-15 and is therefore not available here: the run is held to the limit rule's own floors, FLOOR
    and 3e-15 max(1, ratio) (an oracle error of 0 in hp_limits._report_and_check)."""
    d, K = RESIDENT[0], RESIDENT[1]
    X, pi0, mu0, S0 = problem(*RESIDENT)
    _, _, ll, pi1, mu1, S1, _ = _resident_run(ctx)
    pi, mu, S = pi0, mu0, S0
    for _ in range(4):
        ref = hp.em_step(X, pi, mu, S)
        pi, mu, S = ref[2], ref[3], ref[4] + LD(R) * np.eye(d, dtype=LD)
    ratio = hp.conditioning(X.astype(LD).mean(axis=0), ref[3], covs=ref[4])["ratio"]
    none = {"ll": 0.0, "resp": None, "mixing": 0.0, "means": 0.0, "covs": np.zeros(K)}
    _report_and_check("ridge 1e-3: resident EM loop, 4 iterations, d=2 K=3", _errors((ll, None, pi1, mu1, _ridge_taken_off(S1, R, False)), ref),
                      none, ratio)


@pytest.mark.parametrize("d", [8, 32])
def test_refinement_pass_error_at_the_ridge(ctx, d):
    """refinement_problem(d, 2e4): the guard sees the covariances WITH the ridge, so the ratios come from the reference covariances
    + r I; the one component above MLHIP_REFINE_RATIO is refined (em_refine launched once) and held at ratio 1."""
    from oracle import oracle_ctypes as orc
    from test_gpu_hp_error import _with_references
    X, pi0, mu0, S0 = refinement_problem(d, 2e4)
    _, _, _, _, ref, e_cpu, _, _ = _with_references(orc, X, pi0, mu0, S0, False)
    ratio = hp.conditioning(X.astype(LD).mean(axis=0), ref[3], covs=ref[4] + LD(R) * np.eye(d, dtype=LD))["ratio"]
    with _switches(SPARSE0):
        dt = _data(ctx, X, R)
        ctx.timing_enable(True)
        ctx.timing_reset()
        ll, pi1, mu1, S1 = dt.em_step(pi0, mu0, S0)
        refined = _launches(ctx, "em_refine")
        ctx.timing_enable(False)
        dt.close()
    assert refined == int((ratio > 1e4).sum()) == 1, (refined, ratio)
    _report_and_check(f"ridge 1e-3: refinement pass d={d} ratio {ratio.max():.4g}", _errors((ll, None, pi1, mu1, _ridge_taken_off(S1, R, False)), ref),
                      dict(e_cpu, resp=None), ratio, refined=ratio > 1e4)


# ---- D. the scikit-learn fixtures ------------------------------------------------------------------------------------------------

def relerr(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, np.max(np.abs(b)))


def test_full_step_matches_sklearn_reg_covar(ctx):
    g = load_golden("em_ridge_onestep_full_d4_K3.npz")
    dt = _data(ctx, g["X"], float(g["ridge"]))
    ll, pi1, mu1, S1 = dt.em_step(g["pi0"], g["mu0"], g["Sigma0"])
    assert abs(ll - float(g["ll0"])) <= 1e-12 * abs(float(g["ll0"]))
    assert relerr(pi1, g["pi1"]) < 1e-11 and relerr(mu1, g["mu1"]) < 1e-11 and relerr(S1, g["Sigma1"]) < 1e-10
    pi3, mu3, S3 = dt.em_maximisation_from(g["R0"])
    assert relerr(pi3, g["pi1"]) < 1e-11 and relerr(mu3, g["mu1"]) < 1e-11 and relerr(S3, g["Sigma1"]) < 1e-10
    dt.close()


def test_diag_step_matches_sklearn_reg_covar(ctx):
    g = load_golden("em_ridge_onestep_diag_d7_K5.npz")
    dt = _data(ctx, g["X"], float(g["ridge"]))
    _subset(dt.em_route(5, "diag"), {"diag_kernel": True})
    ll, pi1, mu1, var1 = dt.em_step_diag(g["pi0"], g["mu0"], g["var0"])
    dt.close()
    assert abs(ll - float(g["ll0"])) <= 1e-12 * abs(float(g["ll0"]))
    assert relerr(pi1, g["pi1"]) < 1e-11 and relerr(mu1, g["mu1"]) < 1e-11 and relerr(var1, g["var1"]) < 1e-10


@pytest.mark.parametrize("route", ["kernel", "composed"])
def test_tied_step_matches_sklearn_reg_covar(ctx, route):
    g = load_golden("em_ridge_onestep_tied_d13_K5.npz")
    with _switches({"MLHIP_TIED": route}):
        dt = _data(ctx, g["X"], float(g["ridge"]))
        assert dt.em_tied_route(5) == route
        ll, pi1, mu1, S1 = dt.em_step_tied(g["pi0"], g["mu0"], g["Sigma0"])
        dt.close()
    assert abs(ll - float(g["ll0"])) <= 1e-12 * abs(float(g["ll0"]))
    assert relerr(pi1, g["pi1"]) < 1e-11 and relerr(mu1, g["mu1"]) < 1e-11 and relerr(S1, g["Sigma1"]) < 1e-10


# ---- E. the facade -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("covariance_type", ["full", "diag", "tied"])
def test_facade_equals_the_handle_level_loop(ctx, covariance_type):
    from ml_amd.cppyml import clustering as cl
    X, _, mu0, _ = problem(4, 3, 3001, 0.0)
    K, d, steps = 3, 4, 5
    em = cl.EM(K)
    em.set_covariance_type(covariance_type)
    em.set_means_initialiser(cl.FixedCentroids(mu0))
    em.set_maximum_steps(steps)
    em.set_absolute_tolerance(0)
    em.set_relative_tolerance(0)
    em.set_covariance_regularisation(R)
    em.fit(X)
    assert em.steps_done == steps and em.covariance_regularisation == R
    # the facade's start: those means, the sample covariance (no ridge on it), pi = 1 / K
    dt = _data(ctx, X, R)
    _, cov = dt.sample_covariance()
    pi0 = np.full(K, 1.0 / K)
    if covariance_type == "diag":
        S0 = np.stack([np.diag(cov).copy()] * K)
    elif covariance_type == "tied":
        S0 = np.zeros((d, d))
        for k in range(K):                                              # the pooled start, ascending k
            S0 += pi0[k] * cov
    else:
        S0 = np.stack([cov] * K)
    out = dt.em_iterate(pi0, mu0, S0, steps, 0.0, 0.0, covariance_type == "diag", covariance_type == "tied")
    dt.close()
    assert out[0] == steps
    assert _same_bits(em.log_likelihood, out[2])
    assert _same_bits(em.mixing_probabilities, out[3]) and _same_bits(np.ascontiguousarray(em.means.T), out[4])
    for k in range(K):
        want = np.diag(out[5][k]) if covariance_type == "diag" else out[5] if covariance_type == "tied" else out[5][k]
        assert _same_bits(em.covariance(k), want), k
    # the ridge reached the fit: every diagonal entry lies at least r above ... nothing smaller than r
    assert min(np.diag(em.covariance(k)).min() for k in range(K)) >= R


@pytest.mark.parametrize("covariance_type", ["full", "diag", "tied"])
def test_a_collinear_sample_is_fitted_with_the_ridge(covariance_type):
    """Column 15 repeats column 0: every M-step's covariance S_k is singular up to rounding (lambda_min ~ 1e-15 against lambda_max
    40 ... 85), and Sigma_k = S_k + r I has lambda_min >= r (1 - 1e-6): S_k is positive semidefinite up to rounding of order
    2^-53 |S_k| ~ 1e-14 (the extended-precision M-step alone gives 0.00099999999999885 on this input's first M-step). The same fit
    at the default ridge is not asserted on."""
    from ml_amd.cppyml import clustering as cl
    X = problem(16, 8, 4001, 2.0)[0].copy()
    X[:, 15] = X[:, 0]
    K = 8
    em = cl.EM(K)
    em.set_covariance_type(covariance_type)
    em.set_maximise_first(True)
    em.set_responsibilities_initialiser(cl.ClosestCentroid(cl.FixedCentroids(np.ascontiguousarray(X[:K]))))
    em.set_maximum_steps(10)
    em.set_covariance_regularisation(R)
    em.fit(X)
    assert np.isfinite(em.log_likelihood) and np.isfinite(em.means).all() and np.isfinite(em.mixing_probabilities).all()
    for k in range(K):
        S = em.covariance(k)
        assert np.isfinite(S).all()
        assert np.linalg.eigvalsh(S).min() >= R * (1 - 1e-6), (k, np.linalg.eigvalsh(S).min())
