"""Every EM route on ILL-CONDITIONED covariances (cond 1e6 and 1e8: kappa = |L|_inf |L^-1|_inf of 1e3 ... 1e5), held to the
whitening model instead of the oracle's error. Needs a GPU: `timeout -k 10 1800 pytest tests/test_gpu_hp_ill.py -m gpu -x -s`.

The oracle evaluates the density with the explicit inverse covariance and loses ~ cond * 2^-53 there; every kernel whitens
(y = W (x - mu), W = L^-1, q = |y|^2) and should lose only ~ kappa * 2^-53, kappa ~ sqrt(cond). On such inputs
tests/test_gpu_hp_error.py's rule err_gpu <= 4 max(err_cpu, floor) would let a kernel be 10 to 100 times worse than its own algorithm
permits. Here the limits are tests/hp_limits.ill_limits():

* log-likelihood, responsibilities, mixing weights:  max(C_ILL[o] sqrt(N) 2^-53 max kappa, 4 * 8 * 2^-53), plus 4 x 1e-13 (scaled as
  in test_gpu_hp_error.py) where the FOLD form ran;
* means, covariances, per component:  max(C_ILL[o] sqrt(N_k) 2^-53 kappa_k, the well conditioned suites' floor);
* a second E-step's log-likelihood (the closing's factor of an ill-conditioned NEW covariance) against the reference on the very
  fp64 parameters the library returned:  max(C_ILL["ll2"] sqrt(N) 2^-53 max kappa(new), 4 * 8 * 2^-53);
* em_score's per-row log-densities:  C_ILL["lse"] sqrt(N) 2^-53 max kappa, absolute; labels on every row the reference decides by
  more than that (at least 99.9 % of the rows).

C_ILL (oracle/hp_cases.py) is 4 x what an fp64 numpy restatement of the whitening form needs on the same inputs, measured on the
CPU (tests/test_hp_reference.py), never on a kernel. Every case first asserts the route it is written for and prints one `HPERR`
line: err_gpu / err_whitened_fp64 / err_oracle per output; DESIGN.md section 4.1 holds the table of one run on one MI355X."""
import functools

import numpy as np
import pytest

from oracle import hp_cases
from oracle import hp_reference as hp
from hp_limits import FOLD_BOUND, _ridge_off, check_ill, check_ill_rows, ill_errors, ill_limits, ill_ll2_limit, ill_references

pytestmark = pytest.mark.gpu

LD = np.longdouble
SHAPE = {s[0]: s for s in hp_cases.ILL_SHAPES}


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
def _case(shape, cond):
    """The input and its CPU references (cached: the switch variants, the closing and the scoring cases of one shape share them)."""
    return ill_references(*shape, cond)


def _fold_ran(taken, conditioning):
    """FOLD runs wherever the route allows it and every |W (mu - shift)| entry is <= 64 (decided at launch from the parameters)."""
    return bool(taken["estep"] == "matrix4" and not taken["fused"] and taken["fold_allowed"] and conditioning["fold"].max() <= 64)


# ---- (a) one E + M step through every E-step and statistics family ------------------------------------------------------------

FOLD_D16 = {"estep": "matrix4", "fold_allowed": True, "self_norm": True}
ABOVE_FOLD = {"estep": "matrix4", "fold_allowed": False, "fused": False}
# name, shape, switches, the route the case is written for
STEP_CASES = [
    ("fused vector-unit, d=2 K=3", SHAPE[2], {}, {"fused": True, "fused_form": "valu"}),
    ("fused scalar-feed, d=8 K=5", SHAPE[8], {}, {"fused": True, "fused_form": "scalar_feed"}),
    ("fused LDS-feed, d=6 K=8", SHAPE[6], {}, {"fused": True, "fused_form": "lds_feed"}),
    ("estep scalar-fed + split statistics, d=3", SHAPE[3], {"MLHIP_FUSED": "0"}, {"estep": "scalar_fed", "fused": False}),
    ("estep scalar-fed + split statistics, d=8", SHAPE[8], {"MLHIP_FUSED": "0"}, {"estep": "scalar_fed", "fused": False, "self_norm": False}),
    ("matrix-core FOLD + self-norm dense, d=16", SHAPE[16], {"MLHIP_MSTATS_SPARSE": "0"}, dict(FOLD_D16, sparse=False)),
    ("matrix-core FOLD + self-norm sparse, d=16", SHAPE[16], {"MLHIP_MSTATS_SPARSE": "1"}, dict(FOLD_D16, sparse=True)),
    ("matrix-core exact form, d=16", SHAPE[16], {"MLHIP_ESTEP_FOLD": "0", "MLHIP_MSTATS_SPARSE": "0"},
     {"estep": "matrix4", "fold_allowed": False, "self_norm": True}),
    ("matrix-core + MLHIP_SELF_NORM=0, d=16", SHAPE[16], {"MLHIP_SELF_NORM": "0"}, {"estep": "matrix4", "self_norm": False}),
    ("estep scalar-fed (valu), d=16", SHAPE[16], {"MLHIP_ESTEP": "valu"}, {"estep": "scalar_fed", "fused": False, "self_norm": False}),
    ("matrix-core row-major FOLD, d=24 K=6", SHAPE[24], {}, {"estep": "matrix4", "fold_allowed": True, "self_norm": True, "fused": False}),
    ("matrix-core row-major FOLD, d=32 K=16 sparse", SHAPE[32], {"MLHIP_MSTATS_SPARSE": "1"},
     {"estep": "matrix4", "fold_allowed": True, "self_norm": True, "fused": False, "sparse": True}),
    ("matrix-core d=33 (above the FOLD range)", SHAPE[33], {}, ABOVE_FOLD),
    ("matrix-core d=64", SHAPE[64], {}, ABOVE_FOLD),
    ("matrix-core d=72", SHAPE[72], {}, ABOVE_FOLD),
    ("matrix-core d=128", SHAPE[128], {}, ABOVE_FOLD),
    ("big-dim d=136", SHAPE[136], {}, {"estep": "big_dim", "fused": False, "self_norm": False}),
    ("plain tier d=136", SHAPE[136], {"MLHIP_BIG_DIM": "0"}, {"estep": "plain", "fused": False, "self_norm": False}),
]


def _step(ctx, c, route):
    """One em_step on a fresh handle, its route asserted first: (route, launch counts, (ll, resp, pi1, mu1, S1 without the ridge))."""
    K = len(c["pi0"])
    dt = _data(ctx, c["X"])
    taken = dt.em_route(K)
    _assert_route(taken, route)
    ctx.timing_enable(True)
    ctx.timing_reset()
    ll, pi1, mu1, S1 = dt.em_step(c["pi0"], c["mu0"], c["S0"])
    launched = {name: _launches(ctx, name) for name in ("em_fused", "em_estep", "em_mstats", "em_refine")}
    ctx.timing_enable(False)
    resp = dt.em_responsibilities(K)
    dt.close()
    return taken, launched, (ll, resp, pi1, mu1, _ridge_off(S1, False))


@pytest.mark.parametrize("cond", hp_cases.ILL_CONDS, ids=[f"cond={c:g}" for c in hp_cases.ILL_CONDS])
@pytest.mark.parametrize("name,shape,env,route", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_em_step_error_ill(ctx, monkeypatch, name, shape, env, route, cond):
    c = _case(shape, cond)
    _setenv(monkeypatch, env)
    taken, launched, got = _step(ctx, c, route)
    # the kernel families the step launched: the fused kernel alone, or an E-step and a statistics kernel; no refinement pass
    assert launched == dict({"em_fused": 1, "em_estep": 0, "em_mstats": 0} if taken["fused"] else {"em_fused": 0, "em_estep": 1, "em_mstats": 1},
                            em_refine=0), launched
    fold_ran = _fold_ran(taken, c["old"])
    label = f"{name}, cond {cond:g}" + (f" [max abs W(mu-s) {c['old']['fold'].max():.3g}]" if taken["estep"] == "matrix4" else "")
    if taken["estep"] == "matrix4" and not taken["fused"] and taken["fold_allowed"]:
        # a FOLD route: below the guard the FOLD form must have run -- its bits differ from MLHIP_ESTEP_FOLD=0 --, above it the
        # library must have switched to the exact form: the bits of MLHIP_ESTEP_FOLD=0
        monkeypatch.setenv("MLHIP_ESTEP_FOLD", "0")
        _, _, exact = _step(ctx, c, {"estep": "matrix4", "fold_allowed": False, "fused": False})
        same = got[0] == exact[0] and np.array_equal(got[1], exact[1])
        label += f" [bits of the exact form: {same}]"
        assert same == (not fold_ran), label
    check_ill(label, ill_errors(got, c["ref"]), c["ref"], c["old"]["kappa"], c["new"]["ratio"], shape[2], fold_ran, c["e_white"], c["e_oracle"])


# ---- (b) closing: the factor of an ill-conditioned NEW covariance, as the next E-step sees it ----------------------------------

# name, shape, switches, the route, the launch counter that must (not) have counted
CLOSE_CASES = [
    ("resident loop, d=2", SHAPE[2], {}, {"fused": True, "fused_form": "valu", "resident": True, "device_close": True}, ("em_resident", True)),
    ("register closing, d=16", SHAPE[16], {"MLHIP_RESIDENT": "0"}, {"device_close": True, "resident": False}, ("em_close", True)),
    ("register closing, d=32 K=16", SHAPE[32], {"MLHIP_RESIDENT": "0"}, {"device_close": True, "resident": False}, ("em_close", True)),
    ("LDS closing, d=64", SHAPE[64], {}, {"device_close": True, "records_on_device": False}, ("em_close", True)),
    ("panelled closing, d=72", SHAPE[72], {}, {"device_close": True, "records_on_device": True}, ("em_close", True)),
    ("panelled closing, d=128", SHAPE[128], {}, {"device_close": True, "records_on_device": True}, ("em_close", True)),
    ("closing on the host, d=16", SHAPE[16], {"MLHIP_DEVICE_CLOSE": "0"}, {"device_close": False}, ("em_close", False)),
    ("closing on the host, d=72", SHAPE[72], {"MLHIP_DEVICE_CLOSE": "0"}, {"device_close": False, "records_on_device": False}, ("em_close", False)),
]


@pytest.mark.parametrize("name,shape,env,route,counter", CLOSE_CASES, ids=[c[0] for c in CLOSE_CASES])
def test_em_closing_error_ill(ctx, monkeypatch, name, shape, env, route, counter):
    """em_iterate(..., 1) hands out (pi1, mu1, S1) as the fp64 numbers the loop goes on with, ridge included; em_iterate(..., 2)'s
    second log-likelihood is compared with the reference's on exactly these parameters -- no intrinsic rounding of S1 enters, only
    the closing's factorization of it (kappa ~ 1e4 ... 1e5) and the density."""
    cond = 1e8
    d, K, n = shape
    c = _case(shape, cond)
    _setenv(monkeypatch, env)
    dt = _data(ctx, c["X"])
    taken = dt.em_route(K)
    _assert_route(taken, route)
    steps1, _, _, pi1, mu1, S1, _ = dt.em_iterate(c["pi0"], c["mu0"], c["S0"], 1)
    dt.close()
    dt = _data(ctx, c["X"])
    ctx.timing_enable(True)
    ctx.timing_reset()
    steps2, _, _, _, _, _, hist = dt.em_iterate(c["pi0"], c["mu0"], c["S0"], 2)
    launched = {key: _launches(ctx, key) for key in ("em_close", "em_resident")}
    ctx.timing_enable(False)
    dt.close()
    assert steps1 == 1 and steps2 == 2 and len(hist) == 2
    if counter[0] == "em_resident":
        assert launched["em_resident"] == 1, launched
    else:
        assert (launched["em_close"] >= 1) == counter[1] and launched["em_resident"] == 0, launched
    ref = c["ref"]
    first = ill_limits(ref, c["old"]["kappa"], c["new"]["ratio"], n, _fold_ran(taken, c["old"]))["ll"]
    e_first = abs(float((LD(hist[0]) - ref[0]) / ref[0]))
    ref2 = hp._normalise(hp.log_weights(c["X"], pi1, mu1, S1))[1].sum() / n
    new = hp.conditioning(c["X"].astype(LD).mean(axis=0), mu1, covs=S1)
    limit = ill_ll2_limit(n, new["kappa"]) + (4 * FOLD_BOUND / abs(float(ref2)) if _fold_ran(taken, new) else 0.0)
    e_second = abs(float((LD(hist[1]) - ref2) / ref2))
    white = abs(float((LD(hp_cases.whitened_log_likelihood_fp64(c["X"], pi1, mu1, S1)[0]) - ref2) / ref2))
    print(f"HPERR {name}, cond {cond:g} | kappa {c['old']['kappa'].max():.3g}, of the new covariances {new['kappa'].max():.3g} | first ll "
          f"{e_first:.1e} (limit {first:.1e}) | second ll {e_second:.1e} / {white:.1e} / - (limit {limit:.1e})", flush=True)
    assert e_first <= first and e_second <= limit, (name, e_first, first, e_second, limit)


# ---- (c) scoring ------------------------------------------------------------------------------------------------------------------

SCORE_CASES = [("score scalar-fed, d=8", SHAPE[8], {}, "scalar_fed"), ("score matrix-core, d=16", SHAPE[16], {}, "matrix4"),
               ("score matrix-core, d=72", SHAPE[72], {}, "matrix4"), ("score composed, d=136", SHAPE[136], {}, "composed")]


@pytest.mark.parametrize("name,shape,env,route", SCORE_CASES, ids=[c[0] for c in SCORE_CASES])
def test_em_score_error_ill(ctx, monkeypatch, name, shape, env, route):
    cond = 1e8
    c = _case(shape, cond)
    _setenv(monkeypatch, env)
    dt = _data(ctx, c["X"])
    assert dt.em_score_route(len(c["pi0"])) == route
    ctx.timing_enable(True)
    ctx.timing_reset()
    dens, labels = dt.em_score(c["pi0"], c["mu0"], c["S0"])
    n_score, n_estep = _launches(ctx, "em_score"), _launches(ctx, "em_estep")
    ctx.timing_enable(False)
    dt.close()
    assert n_score >= 1 and ((n_estep >= 1) if route == "composed" else (n_estep == 0)), (n_score, n_estep)
    assert np.all(np.isfinite(dens))
    check_ill_rows(f"{name}, cond {cond:g}", dens, labels, c["lw"], shape[2], c["old"]["kappa"])
