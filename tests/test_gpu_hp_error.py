"""How far each kernel route is from the TRUE value: kernel, CPU oracle and the extended-precision reference
(oracle/hp_reference.py) on the same inputs, err_gpu = |gpu - hp| and err_cpu = |oracle - hp| in DESIGN.md section 4's norms
(log-likelihood relative, responsibilities absolute, mixing / means max-norm relative, covariances max-norm relative PER
COMPONENT). Needs a GPU: `timeout -k 10 1800 pytest tests/test_gpu_hp_error.py -m gpu -x -s`.

Every case first asserts the route it is written for (Data.em_route / Data.kmeans_route; decisions taken at launch by a launch
counter or a pinned switch). Limits -- from section 4's own models or the oracle's error on the same case, never from what a
kernel was seen to give:

* covariances / variances:  err_gpu <= 4 max(err_cpu, 3e-15 max(1, ratio_k))  per component, ratio_k from hp.conditioning();
* what a fast density form (FOLD, the diagonal two-operation form) feeds directly -- responsibilities, log-likelihood, mixing
  weights:  4 x the section 4 absolute bound (1e-13; 2^-53 sum_j |b_j|), and never below the next line's limit (no form can be
  asked to beat the rounding of its own output); a component the library refined: the covariance model at ratio 1;
* everything else:  err_gpu <= 4 max(err_cpu, 8 * 2^-53).

The 4 allows for another, equally valid summation order. Each case prints one `HPERR` line; DESIGN.md section 4 holds the table
of one run on one MI355X. All shapes have a ragged last tile (N not a multiple of 64) and most data sit off-centre."""
import functools
import math

import numpy as np
import pytest

from oracle import hp_reference as hp
from oracle.hp_cases import KMEANS_SHAPES, edge_problem, oracle_step, problem, refinement_problem
from hp_limits import FLOOR, FOLD_BOUND, _check_kmeans, _errors, _fsum_centroids, _report_and_check, _ridge_off

pytestmark = pytest.mark.gpu

LD = np.longdouble


@pytest.fixture(scope="module")
def ctx():
    from ml_amd import _lib
    c = _lib.Context()
    yield c
    c.close()


def _data(ctx, X):
    from ml_amd import _lib
    return _lib.Data(ctx, np.ascontiguousarray(X, dtype=np.float64))


def _launches(ctx, name):
    return ctx.timing_get(name)[1]


def _setenv(monkeypatch, env):
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def _assert_route(route, want):
    got = {k: route[k] for k in want}
    assert got == want, (got, want)


@functools.lru_cache(maxsize=None)
def _full_case(d, K, n, offset):
    """Inputs, the reference step, the oracle step and its errors, the new parameters' refinement ratios (cached: the switch
    variants of one shape share them)."""
    from oracle import oracle_ctypes as orc
    X, pi0, mu0, S0 = problem(d, K, n, offset)
    return _with_references(orc, X, pi0, mu0, S0, False)


def _with_references(orc, X, pi0, mu0, S0, diagonal):
    ref = (hp.em_step_diag if diagonal else hp.em_step)(X, pi0, mu0, S0)
    e_cpu = _errors(oracle_step(orc, X, pi0, mu0, S0, diagonal), ref)
    shift = X.astype(LD).mean(axis=0)
    new = hp.conditioning(shift, ref[3], **({"variances": ref[4]} if diagonal else {"covs": ref[4]}))
    old = hp.conditioning(shift, mu0, **({"variances": S0} if diagonal else {"covs": S0}))
    return X, pi0, mu0, S0, ref, e_cpu, new["ratio"], old


# ---- one E + M step, full covariances: every E-step and statistics route --------------------------------------------------

# name, (d, K, N, offset), switches, the route the case is written for
STEP_CASES = [
    ("estep scalar-fed + split statistics, d=8", (8, 5, 3001, 3.0), {"MLHIP_FUSED": "0"}, {"estep": "scalar_fed", "fused": False, "self_norm": False}),
    ("estep scalar-fed, d=3", (3, 4, 3001, 5.0), {"MLHIP_FUSED": "0"}, {"estep": "scalar_fed", "fused": False}),
    ("estep scalar-fed (valu), d=16", (16, 8, 4001, 2.0), {"MLHIP_ESTEP": "valu"}, {"estep": "scalar_fed", "fused": False, "self_norm": False}),
    ("matrix-core FOLD + self-norm dense, d=16", (16, 8, 4001, 2.0), {"MLHIP_MSTATS_SPARSE": "0"},
     {"estep": "matrix4", "fold_allowed": True, "self_norm": True, "sparse": False}),
    ("matrix-core FOLD + self-norm sparse, d=16", (16, 8, 4001, 2.0), {"MLHIP_MSTATS_SPARSE": "1"},
     {"estep": "matrix4", "fold_allowed": True, "self_norm": True, "sparse": True}),
    ("matrix-core exact form, d=16", (16, 8, 4001, 2.0), {"MLHIP_ESTEP_FOLD": "0", "MLHIP_MSTATS_SPARSE": "0"},
     {"estep": "matrix4", "fold_allowed": False, "self_norm": True}),
    ("matrix-core + MLHIP_SELF_NORM=0, d=16", (16, 8, 4001, 2.0), {"MLHIP_SELF_NORM": "0"}, {"estep": "matrix4", "self_norm": False}),
    ("matrix-core FOLD, d=32 K=16 sparse", (32, 16, 6001, 0.0), {"MLHIP_MSTATS_SPARSE": "1"},
     {"estep": "matrix4", "fold_allowed": True, "self_norm": True, "sparse": True}),
    ("matrix-core exact form, d=32 K=16 dense", (32, 16, 6001, 0.0), {"MLHIP_ESTEP_FOLD": "0", "MLHIP_MSTATS_SPARSE": "0"},
     {"estep": "matrix4", "fold_allowed": False, "self_norm": True, "sparse": False}),
    ("split statistics (MLHIP_SELF_NORM=0), d=16 K=24", (16, 24, 5001, 1.0), {"MLHIP_SELF_NORM": "0"}, {"estep": "matrix4", "self_norm": False}),
    ("split statistics (MLHIP_SELF_NORM=0), d=16 K=40", (16, 40, 6001, 1.0), {"MLHIP_SELF_NORM": "0"}, {"estep": "matrix4", "self_norm": False}),
    ("statistics d=12", (12, 5, 3001, 4.0), {"MLHIP_MSTATS_SPARSE": "0"}, {"estep": "matrix4", "self_norm": True, "sparse": False}),
    ("matrix-core d=33 (above the FOLD range)", (33, 4, 3001, 0.0), {}, {"estep": "matrix4", "fold_allowed": False}),
    ("matrix-core d=128", (128, 3, 2001, 0.0), {}, {"estep": "matrix4", "fold_allowed": False}),
    ("fused vector-unit, d=2 K=3", (2, 3, 3001, 0.0), {}, {"fused": True, "fused_form": "valu"}),
    ("fused scalar-feed, d=8 K=5", (8, 5, 3001, 3.0), {}, {"fused": True, "fused_form": "scalar_feed"}),
    ("fused LDS-feed, d=6 K=8", (6, 8, 3001, 2.0), {}, {"fused": True, "fused_form": "lds_feed"}),
    ("big-dim d=192 K=2 N=1501", (192, 2, 1501, 0.0), {}, {"estep": "big_dim", "fused": False, "self_norm": False}),
    ("big-dim d=192 K=4 N=3001", (192, 4, 3001, 1.0), {}, {"estep": "big_dim", "fused": False, "self_norm": False}),
    ("plain tier d=192 K=2", (192, 2, 1501, 0.0), {"MLHIP_BIG_DIM": "0"}, {"estep": "plain", "fused": False, "self_norm": False}),
]


@pytest.mark.parametrize("name,shape,env,route", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_em_step_error(ctx, monkeypatch, name, shape, env, route):
    X, pi0, mu0, S0, ref, e_cpu, ratio, old = _full_case(*shape)
    _setenv(monkeypatch, env)
    dt = _data(ctx, X)
    taken = dt.em_route(len(pi0))
    _assert_route(taken, route)
    ctx.timing_enable(True)
    ctx.timing_reset()
    ll, pi1, mu1, S1 = dt.em_step(pi0, mu0, S0)
    launched = {name: _launches(ctx, name) for name in ("em_fused", "em_estep", "em_mstats")}
    ctx.timing_enable(False)
    # the kernel families the step launched: the fused kernel alone, or an E-step and a statistics kernel
    assert launched == ({"em_fused": 1, "em_estep": 0, "em_mstats": 0} if taken["fused"] else {"em_fused": 0, "em_estep": 1, "em_mstats": 1}), launched
    resp = dt.em_responsibilities(len(pi0))
    dt.close()
    e_gpu = _errors((ll, resp, pi1, mu1, _ridge_off(S1, False)), ref)
    # (the form is chosen at launch from the parameters: FOLD wherever the route allows it and every |W (mu - s)| entry is <= 64)
    fold = taken["estep"] == "matrix4" and taken["fold_allowed"] and old["fold"].max() <= 64
    _report_and_check(name + (f" [max abs W(mu-s) {old['fold'].max():.3g}]" if route.get("estep") == "matrix4" else ""), e_gpu, e_cpu, ratio,
                      FOLD_BOUND if fold else None, "FOLD", abs(float(ref[0])))


# ---- closing: one iteration of mlhip_em_iterate ----------------------------------------------------------------------------

CLOSE_CASES = [
    ("closing on the device, d=16", (16, 8, 4001, 2.0), {"MLHIP_RESIDENT": "0"}, True, {"device_close": True}),
    ("closing on the device, d=64", (64, 4, 3001, 3.0), {}, True, {"device_close": True, "records_on_device": False}),
    ("panelled closing, d=72", (72, 2, 2501, 0.0), {}, True, {"device_close": True, "records_on_device": True}),
    ("panelled closing, d=256", (256, 2, 1501, 0.0), {}, True, {"device_close": True, "records_on_device": True, "estep": "big_dim"}),
    ("closing on the host, d=16", (16, 8, 4001, 2.0), {"MLHIP_DEVICE_CLOSE": "0"}, False, {"device_close": False}),
    ("closing on the host, d=72", (72, 2, 2501, 0.0), {"MLHIP_DEVICE_CLOSE": "0"}, False, {"device_close": False, "records_on_device": False}),
]


@pytest.mark.parametrize("name,shape,env,on_device,route", CLOSE_CASES, ids=[c[0] for c in CLOSE_CASES])
def test_em_closing_error(ctx, monkeypatch, name, shape, env, on_device, route):
    X, pi0, mu0, S0, ref, e_cpu, ratio, _ = _full_case(*shape)
    _setenv(monkeypatch, env)
    dt = _data(ctx, X)
    _assert_route(dt.em_route(len(pi0)), route)
    ctx.timing_enable(True)
    ctx.timing_reset()
    steps, _, ll, pi1, mu1, S1, hist = dt.em_iterate(pi0, mu0, S0, 1)
    closes = _launches(ctx, "em_close")
    ctx.timing_enable(False)
    dt.close()
    assert steps == 1 and (closes >= 1) == on_device, (steps, closes)
    e_gpu = _errors((ll, None, pi1, mu1, _ridge_off(S1, False)), ref)
    e_cpu = dict(e_cpu, resp=None)
    _report_and_check(name, e_gpu, e_cpu, ratio)


def test_resident_em_loop_error(ctx, oracle, monkeypatch):
    """The one-launch loop (d = 2, K = 3): the end of 4 iterations against 4 reference steps (each fed the previous one's
    extended-precision parameters, + 1e-15 I as the library adds it) and the oracle's 4 steps."""
    d, K, n = 2, 3, 3001
    X, pi0, mu0, S0 = problem(d, K, n, 0.0)
    dt = _data(ctx, X)
    _assert_route(dt.em_route(K), {"fused": True, "fused_form": "valu", "resident": True, "device_close": True})
    ctx.timing_enable(True)
    ctx.timing_reset()
    steps, _, ll, pi1, mu1, S1, _ = dt.em_iterate(pi0, mu0, S0, 4)
    assert _launches(ctx, "em_resident") == 1 and _launches(ctx, "em_fused") == 0 and steps == 4
    ctx.timing_enable(False)
    dt.close()
    pi, mu, S = pi0, mu0, S0
    for _ in range(4):
        ref = hp.em_step(X, pi, mu, S)
        pi, mu, S = ref[2], ref[3], ref[4] + LD(1e-15) * np.eye(d, dtype=LD)
    em = oracle.EM(K)
    em.set_parameters(mu0, S0, pi0)
    for _ in range(4):
        em.expectation_step(X)
        em.maximisation_step(X)
    cpu = (em.log_likelihood, None, em.mixing_probabilities, em.means, _ridge_off(em.covariances, False))
    ratio = hp.conditioning(X.astype(LD).mean(axis=0), ref[3], covs=ref[4])["ratio"]
    _report_and_check("resident EM loop, 4 iterations, d=2 K=3", _errors((ll, None, pi1, mu1, _ridge_off(S1, False)), ref),
                      _errors(cpu, ref), ratio)


# ---- diagonal covariances --------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _diag_case(d, K, n, offset):
    from oracle import oracle_ctypes as orc
    X, pi0, mu0, var0 = problem(d, K, n, offset, diagonal=True)
    return _with_references(orc, X, pi0, mu0, var0, True)


def _diag_model(X, mu0, var0):
    """Section 4: the two-operation form costs ~ eps |b| per term, b_kj = (mu_kj - shift_j) / sigma_kj: 2^-53 max_k sum_j |b_kj|
    in a log-responsibility."""
    b = np.abs((mu0 - X.mean(axis=0)) / np.sqrt(var0))
    return hp.EPS64 * float(b.sum(axis=1).max())


DIAG_CASES = [("diagonal two-operation form, K<=16", (16, 8, 4001, 0.5), {}, False), ("diagonal exact form, K<=16", (16, 8, 4001, 0.5), {"MLHIP_DIAG_AB": "0"}, True),
              ("diagonal two-operation form, K=17..64", (7, 40, 4001, 0.0), {}, False), ("diagonal exact form, K=17..64", (7, 40, 4001, 0.0), {"MLHIP_DIAG_AB": "0"}, True),
              ("diagonal two-operation form, d=32", (32, 8, 3001, 1.0), {}, False)]


@pytest.mark.parametrize("name,shape,env,exact", DIAG_CASES, ids=[c[0] for c in DIAG_CASES])
def test_em_diag_step_error(ctx, monkeypatch, name, shape, env, exact):
    X, pi0, mu0, var0, ref, e_cpu, ratio, old = _diag_case(*shape)
    _setenv(monkeypatch, env)
    dt = _data(ctx, X)
    _assert_route(dt.em_route(len(pi0), "diag"), {"diag_kernel": True, "diag_exact": exact})
    ctx.timing_enable(True)
    ctx.timing_reset()
    ll, pi1, mu1, var1 = dt.em_step_diag(pi0, mu0, var0)
    assert _launches(ctx, "em_diag") >= 1
    ctx.timing_enable(False)
    dt.close()
    assert exact or old["b2"].max() <= 64.0 ** 2                    # (the case is written for the fast form: inside its guard)
    model = None if exact else _diag_model(X, mu0, var0)
    _report_and_check(f"{name} [B2 {old['b2'].max():.3g}]", _errors((ll, None, pi1, mu1, _ridge_off(var1, True)), ref),
                      dict(e_cpu, resp=None), ratio, model, "2^-53 sum abs b", abs(float(ref[0])))


# ---- guard sweeps ----------------------------------------------------------------------------------------------------------

REFINEMENT_ROUTES = {4: {"estep": "scalar_fed", "fused": True}, 8: {"estep": "scalar_fed", "fused": True},
                     32: {"estep": "matrix4", "fused": False}, 80: {"estep": "matrix4", "fused": False}}


@pytest.mark.parametrize("d", [4, 8, 32, 80])
@pytest.mark.parametrize("factor", [0.5, 0.9, 1.1])
def test_refinement_guard_sweep(ctx, oracle, d, factor):
    """Shared-shift covariances just below and just above MLHIP_REFINE_RATIO = 1e4: the model 3e-15 ratio holds up to the guard,
    the refinement pass runs above it and not below, and a refined component is held to the two-pass form's 3e-15 (ratio 1)."""
    X, pi0, mu0, S0 = refinement_problem(d, factor * 1e4)
    _, _, _, _, ref, e_cpu, ratio, _ = _with_references(oracle, X, pi0, mu0, S0, False)
    assert abs(ratio.max() / (factor * 1e4) - 1) < 0.02, ratio           # the achieved value, read back
    dt = _data(ctx, X)
    _assert_route(dt.em_route(2), REFINEMENT_ROUTES[d])
    ctx.timing_enable(True)
    ctx.timing_reset()
    ll, pi1, mu1, S1 = dt.em_step(pi0, mu0, S0)
    refined = _launches(ctx, "em_refine")
    ctx.timing_enable(False)
    dt.close()
    assert refined == int((ratio > 1e4).sum()) == (1 if factor > 1 else 0), (refined, ratio)
    _report_and_check(f"refinement sweep d={d} ratio {ratio.max():.4g} refine launches {refined}",
                      _errors((ll, None, pi1, mu1, _ridge_off(S1, False)), ref), dict(e_cpu, resp=None), ratio, refined=ratio > 1e4)


@pytest.mark.parametrize("d", [16, 32])
@pytest.mark.parametrize("factor", [0.9, 1.1])
def test_fold_guard_sweep(ctx, oracle, monkeypatch, d, factor):
    """max |W (mu - shift)| just below and just above 64 on data whose components OVERLAP at the edge (hp_cases.edge_problem: dense
    covariances, two components one whitened unit apart, hundreds of rows with responsibilities strictly inside (0, 1)). Below, the
    FOLD form must have run -- its bits differ from MLHIP_ESTEP_FOLD=0 -- and keep its 1e-13 in the responsibilities; above, the
    library must have switched to the exact form: the bits of MLHIP_ESTEP_FOLD=0."""
    X, pi0, mu0, S0 = edge_problem(d, factor * 64)
    _, _, _, _, ref, e_cpu, ratio, old = _with_references(oracle, X, pi0, mu0, S0, False)
    assert abs(old["fold"].max() / (factor * 64) - 1) < 1e-6, old["fold"]
    soft = int(((ref[1] > 1e-3) & (ref[1] < 1 - 1e-3)).any(axis=1).sum())
    assert soft >= 500
    dt = _data(ctx, X)
    _assert_route(dt.em_route(3), {"estep": "matrix4", "fold_allowed": True, "fused": False})
    ctx.timing_enable(True)
    ctx.timing_reset()
    ll, pi1, mu1, S1 = dt.em_step(pi0, mu0, S0)
    refined = _launches(ctx, "em_refine")
    ctx.timing_enable(False)
    resp = dt.em_responsibilities(3)
    dt.close()
    monkeypatch.setenv("MLHIP_ESTEP_FOLD", "0")
    dt = _data(ctx, X)
    _assert_route(dt.em_route(3), {"estep": "matrix4", "fold_allowed": False, "fused": False})
    ll_x = dt.em_step(pi0, mu0, S0)[0]
    resp_x = dt.em_responsibilities(3)
    dt.close()
    same = ll == ll_x and np.array_equal(resp, resp_x)
    e_gpu = _errors((ll, resp, pi1, mu1, _ridge_off(S1, False)), ref)
    e_exact = hp.abs_err(resp_x, ref[1])
    name = (f"FOLD sweep d={d} max abs W(mu-s) {old['fold'].max():.4g}, {soft} soft rows, bits of the exact form: {same}, "
            f"exact form's resp {e_exact:.1e}")
    assert same == (factor > 1), name
    _report_and_check(name, e_gpu, e_cpu, ratio, FOLD_BOUND if factor < 1 else None, "FOLD", abs(float(ref[0])), refined=ratio > 1e4,
                      mix_max=float(ref[2].max()))
    assert refined == int((ratio > 1e4).sum())


@pytest.mark.parametrize("factor", [0.9, 1.1])
def test_diag_guard_sweep(ctx, oracle, monkeypatch, factor):
    """B2_k just below and just above 64^2 on data whose components overlap at the edge (hp_cases.edge_problem, diagonal). Below, the
    two-operation form must have run -- its bits differ from MLHIP_DIAG_AB=0 -- and stay within its model 2^-53 sum |b| in what
    depends on the responsibilities (log-likelihood, mixing weights; the diagonal path hands out no responsibilities of its own:
    em_responsibilities rebuilds them with the full-covariance E-step); above, the exact form: the bits of MLHIP_DIAG_AB=0."""
    d = 16
    X, pi0, mu0, var0 = edge_problem(d, 64 * math.sqrt(factor), diagonal=True)
    _, _, _, _, ref, e_cpu, ratio, old = _with_references(oracle, X, pi0, mu0, var0, True)
    assert abs(old["b2"].max() / (factor * 4096) - 1) < 1e-6, old["b2"]
    soft = int(((ref[1] > 1e-3) & (ref[1] < 1 - 1e-3)).any(axis=1).sum())
    assert soft >= 500
    dt = _data(ctx, X)
    _assert_route(dt.em_route(3, "diag"), {"diag_kernel": True, "diag_exact": False})
    got = dt.em_step_diag(pi0, mu0, var0)
    dt.close()
    monkeypatch.setenv("MLHIP_DIAG_AB", "0")
    dt = _data(ctx, X)
    _assert_route(dt.em_route(3, "diag"), {"diag_kernel": True, "diag_exact": True})
    exact = dt.em_step_diag(pi0, mu0, var0)
    dt.close()
    same = all(np.array_equal(a, b) for a, b in zip(got, exact))
    e_exact = _errors((exact[0], None, exact[1], exact[2], _ridge_off(exact[3], True)), ref)
    name = (f"diagonal sweep d={d} B2 {old['b2'].max():.5g}, {soft} soft rows, bits of the exact form: {same}, exact form's ll "
            f"{e_exact['ll']:.1e} mixing {e_exact['mixing']:.1e}")
    assert same == (factor > 1), name
    model = _diag_model(X, mu0, var0) if factor < 1 else None
    _report_and_check(name, _errors((got[0], None, got[1], got[2], _ridge_off(got[3], True)), ref), dict(e_cpu, resp=None), ratio, model,
                      "2^-53 sum abs b", abs(float(ref[0])), mix_max=float(ref[2].max()))


# ---- K-means ---------------------------------------------------------------------------------------------------------------

def _scaled(X):
    """Columns of different scale and offset (as test_kmeans_update_is_bitwise_reproducible_and_exact)."""
    d = X.shape[1]
    scale = np.resize(np.array([1e-3, 1.0, 50.0, 1e4, 3.0]), d)
    offset = np.resize(np.array([0.0, 5.0, -7.0, 1e5, 0.1]), d)
    return np.ascontiguousarray(X * scale + offset)


KM_CASES = [("K-means direct, d=5 K=7", (5, 7, 3001), {}, {"kernel": "direct", "pad": False}),
            ("K-means direct forced, d=16 K=10", (16, 10, 3001), {"MLHIP_KMEANS": "valu"}, {"kernel": "direct", "pad": False}),
            ("K-means matrix-core, d=16 K=10", (16, 10, 3001), {}, {"kernel": "matrix", "pad": False}),
            ("K-means matrix-core, d=72 K=6", (72, 6, 2001), {}, {"kernel": "matrix", "pad": False}),
            ("K-means matrix-core on the padded block, d=5 K=130", (5, 130, 6001), {}, {"kernel": "matrix", "pad": True}),
            ("K-means big-dim, d=192 K=5", (192, 5, 2001), {}, {"kernel": "big_dim", "pad": False}),
            ("K-means plain tier, d=192 K=5", (192, 5, 2001), {"MLHIP_BIG_DIM": "0"}, {"kernel": "plain", "pad": False})]


assert all(c[1] in KMEANS_SHAPES for c in KM_CASES)      # (test_hp_reference.py checks the rows these data leave out, on the CPU)


@functools.lru_cache(maxsize=None)
def _km_case(d, K, n):
    X, _, C0, _ = problem(d, K, n, 2.0)
    return X, C0, hp.kmeans_step(X, C0)


@pytest.mark.parametrize("name,shape,env,route", KM_CASES, ids=[c[0] for c in KM_CASES])
def test_kmeans_step_error(ctx, oracle, monkeypatch, name, shape, env, route):
    d, K, n = shape
    X, C0, ref = _km_case(*shape)
    km = oracle.KMeans(K)
    km.set_centroids(C0, n)
    km.assignment_step(X)
    _setenv(monkeypatch, env)
    dt = _data(ctx, X)
    _assert_route(dt.kmeans_route(K), route)
    ctx.timing_enable(True)
    ctx.timing_reset()
    got = dt.kmeans_step(C0)
    assert _launches(ctx, "kmeans_assign") == 1
    ctx.timing_enable(False)
    labels, dists = dt.kmeans_labels(), dt.kmeans_distances()
    dt.close()
    _check_kmeans(name, X, C0, got, labels, dists, ref, km)


UPDATE_CASES = [("update sums, matrix-core d=8 K=9", (8, 9, 5001), {"kernel": "matrix"}),
                ("update sums, chunked accumulators K=3100 d=4", (4, 3100, 12001), {"kernel": "matrix"}),
                ("update sums, direct K=3100 d=3", (3, 3100, 12001), {"kernel": "direct", "pad": False}),
                ("update sums, the sweep above d=128 (d=136 K=6)", (136, 6, 3001), {"kernel": "big_dim"})]


@pytest.mark.parametrize("name,shape,route", UPDATE_CASES, ids=[c[0] for c in UPDATE_CASES])
def test_kmeans_update_sums_are_exact(ctx, monkeypatch, name, shape, route):
    """The routes test_kmeans_update_is_bitwise_reproducible_and_exact does not reach, columns of different scale and offset: the new
    centroids against math.fsum over the GPU's own labels."""
    d, K, n = shape
    rng = np.random.default_rng(12)
    X = _scaled(rng.standard_normal((n, d)))
    C0 = X[rng.choice(n, K, replace=False)]
    if route["kernel"] == "direct":
        monkeypatch.setenv("MLHIP_KMEANS", "valu")                   # (K >= 128 would run the matrix-core kernel on a padded copy)
    dt = _data(ctx, X)
    _assert_route(dt.kmeans_route(K), route)
    _, _, counts, C1 = dt.kmeans_step(C0)
    labels = dt.kmeans_labels()
    dt.close()
    exact = _fsum_centroids(X, labels, K)
    assert np.array_equal(counts, np.bincount(labels, minlength=K).astype(float))
    err = float(np.max(np.abs(C1 - exact) / np.maximum(np.abs(exact), 1e-300)))
    print(f"HPERR {name} | centroids vs fsum {err:.1e} | empty clusters {int((counts == 0).sum())}", flush=True)
    assert err <= 4e-16                                              # (the existing exactness test's bound)


def test_resident_kmeans_loop_error(ctx, oracle):
    """The one-launch K-means loop (d = 2, K = 5): 3 steps against 3 reference steps (each from the previous one's centroids rounded
    to fp64, as any fp64 route holds them)."""
    d, K, n = KMEANS_SHAPES[0]
    X, _, C0, _ = problem(d, K, n, 2.0)
    dt = _data(ctx, X)
    _assert_route(dt.kmeans_route(K), {"kernel": "direct", "pad": False, "resident": True})
    ctx.timing_enable(True)
    ctx.timing_reset()
    steps, _, inertia, counts, cur, old = dt.kmeans_iterate(C0, 3)
    assert _launches(ctx, "kmeans_resident") == 1 and _launches(ctx, "kmeans_assign") == 0 and steps == 3
    ctx.timing_enable(False)
    labels = dt.kmeans_labels()
    dt.close()
    C, all_safe = C0, True
    for _ in range(3):
        start = C
        dist, label, margin, ref_inertia, ref_counts, new = hp.kmeans_step(X, start)
        all_safe = all_safe and bool((margin > 64 * hp.EPS64 * dist).all())
        C = new.astype(np.float64)
    assert all_safe                                                  # (a condition on the data: no near-tie in any of the steps)
    e_in, e_c = abs(float((LD(inertia) - ref_inertia) / ref_inertia)), hp.rel_err(cur, new)
    print(f"HPERR resident K-means loop, 3 steps, d=2 K=5 | inertia {e_in:.1e} | centroids {e_c:.1e}", flush=True)
    assert np.array_equal(labels, label) and np.array_equal(counts, ref_counts.astype(float))
    assert e_in <= 4 * FLOOR and e_c <= 4 * FLOOR and hp.rel_err(old, start) <= 4 * FLOOR
