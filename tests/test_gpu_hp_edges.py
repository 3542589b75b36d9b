"""Every EM route on the inputs a plain sample never holds -- a component without mass, rows far in a tail, a second iteration after
a component died -- against the extended-precision reference (oracle/hp_reference.py), the CPU oracle as the yardstick, in the
norms and under the limit rules of tests/test_gpu_hp_error.py (tests/hp_limits.py). Needs a GPU:
`timeout -k 10 1800 pytest tests/test_gpu_hp_edges.py -m gpu -x -s`.

Inputs (oracle/hp_cases.py; tests/test_hp_reference.py checks on the CPU what each one is built for):

* massless kinds -- `zero_weight_first` / `zero_weight_last` (pi_k = 0), `far` (the mean 1e4 sigma out: exact density forms), `hole`
  (the mean on the shift, Sigma = tiny^2 I: FOLD and the two-operation form stay on, every row >= 400 whitened units away). The
  reference, the oracle and every route give the pattern DESIGN.md section 4.1 documents: column k of the responsibilities exactly
  0, no label k, pi_k = 0, mu_k and Sigma_k / var_k NaN in every entry, everything else finite -- and that is held to the limits
  of hp_limits._report_and_check, the massless component's entries left out on both sides. `em_refine` launches equal the LIVE
  components above MLHIP_REFINE_RATIO. A `hole` case on a FOLD / two-operation route shows that the fast form ran: its bits differ
  from the exact-form switch.
* `tail` -- twenty rows 40 whitened units behind a mean (log-weights near -800; the oracle's linear-domain sum has underflowed: its
  errors count as 0, as in tests/test_gpu_tied_hp.py::test_rows_far_in_every_tail). The log-likelihood is the mean of the per-row
  log-sum-exp, so it is finite exactly when every one of them is; rows sum to 1 within 4 max(FLOOR, 2 * 2^-53 * lse_max), which is
  also the responsibilities' yardstick (the rounding of an fp64 log-weight of that size); moved rows carry their own label.
* the loop after a component died -- mlhip_em_iterate for 2 iterations on a zero-weight input through every closing: the first
  log-likelihood at the step's limit, the second NaN, every returned parameter NaN, as two steps of the oracle give.

No limit comes from what a kernel gave. Every case asserts its route, then its launch counters, and prints one `HPERR` line
(DESIGN.md section 4.1 holds the table of one run)."""
import functools

import numpy as np
import pytest

from oracle import hp_cases
from oracle import hp_reference as hp
from hp_limits import FLOOR, FOLD_BOUND, _ridge_off, check_massless, check_tail, edge_references
from test_weights_cases import replicate, weights

pytestmark = pytest.mark.gpu

LD = np.longdouble
KINDS = hp_cases.MASSLESS_KINDS + ("tail",)


@pytest.fixture(scope="module")
def ctx():
    from ml_amd import _lib
    c = _lib.Context()
    yield c
    c.close()


def _data(ctx, X, w=None):
    from ml_amd import _lib
    dt = _lib.Data(ctx, np.ascontiguousarray(X, dtype=np.float64))
    if w is not None:
        dt.set_weights(w)
    return dt


def _launches(ctx, name):
    return ctx.timing_get(name)[1]


def _setenv(monkeypatch, env):
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def _assert_route(route, want):
    got = {k: route[k] for k in want}
    assert got == want, (got, want)


@functools.lru_cache(maxsize=None)
def _case(kind, d, K, n, offset, diagonal=False):
    """(X, pi0, mu0, S0, references, moved rows, their components) of one kind at one shape -- cached: the switch variants of a shape
    share it and leave it unchanged."""
    if kind == "tail":
        X, pi0, mu0, S0, rows, comps = hp_cases.tail_problem(d, K, n, offset, diagonal, only_clear=K > hp_cases.TAIL_ROWS)
        k = None
    else:
        X, pi0, mu0, S0, k = hp_cases.massless_problem(kind, d, K, n, offset, diagonal)
        rows = comps = None
    return X, pi0, mu0, S0, edge_references(X, pi0, mu0, S0, k, diagonal), rows, comps


# ---- one E + M step, full covariances ---------------------------------------------------------------------------------------

# name, (d, K, N, offset), switches, the route the case is written for
STEP_ROUTES = [
    ("fused vector-unit, d=2 K=3", (2, 3, 3001, 0.0), {}, {"fused": True, "fused_form": "valu"}),
    ("fused scalar-feed, d=8 K=5", (8, 5, 3001, 3.0), {}, {"fused": True, "fused_form": "scalar_feed"}),
    ("fused LDS-feed, d=6 K=8", (6, 8, 3001, 2.0), {}, {"fused": True, "fused_form": "lds_feed"}),
    ("estep scalar-fed + split statistics, d=8", (8, 5, 3001, 3.0), {"MLHIP_FUSED": "0"}, {"estep": "scalar_fed", "fused": False, "self_norm": False}),
    ("matrix-core FOLD + self-norm dense, d=16", (16, 8, 4001, 2.0), {"MLHIP_MSTATS_SPARSE": "0"},
     {"estep": "matrix4", "fused": False, "fold_allowed": True, "self_norm": True, "sparse": False}),
    ("matrix-core FOLD + self-norm sparse, d=16", (16, 8, 4001, 2.0), {"MLHIP_MSTATS_SPARSE": "1"},
     {"estep": "matrix4", "fused": False, "fold_allowed": True, "self_norm": True, "sparse": True}),
    ("matrix-core exact form, d=16", (16, 8, 4001, 2.0), {"MLHIP_ESTEP_FOLD": "0"}, {"estep": "matrix4", "fused": False, "fold_allowed": False}),
    ("split statistics (MLHIP_SELF_NORM=0), d=16 K=24", (16, 24, 5001, 1.0), {"MLHIP_SELF_NORM": "0"},
     {"estep": "matrix4", "fused": False, "self_norm": False}),
    ("sparse K<64 masks, d=32 K=16", (32, 16, 6001, 0.0), {"MLHIP_MSTATS_SPARSE": "1"},
     {"estep": "matrix4", "fused": False, "fold_allowed": True, "self_norm": True, "sparse": True}),
    ("sparse, every slot a component, d=32 K=64", (32, 64, 2001, 0.0), {"MLHIP_MSTATS_SPARSE": "1"},
     {"estep": "matrix4", "fused": False, "fold_allowed": True, "self_norm": True, "sparse": True}),
    ("dense, d=32 K=64", (32, 64, 2001, 0.0), {"MLHIP_MSTATS_SPARSE": "0"},
     {"estep": "matrix4", "fused": False, "fold_allowed": True, "self_norm": True, "sparse": False}),
    ("matrix-core d=33 (above the FOLD range)", (33, 4, 3001, 0.0), {}, {"estep": "matrix4", "fused": False, "fold_allowed": False}),
    ("big-dim d=136 K=2", (136, 2, 1001, 0.0), {}, {"estep": "big_dim", "fused": False, "self_norm": False}),
    ("plain tier d=136 K=2", (136, 2, 1001, 0.0), {"MLHIP_BIG_DIM": "0"}, {"estep": "plain", "fused": False, "self_norm": False}),
]
STEP_SHAPES = sorted({c[1] for c in STEP_ROUTES})
assert set(STEP_SHAPES) <= set(hp_cases.EDGE_SHAPES)     # (tests/test_hp_reference.py checks every kind's conditions at these shapes)


def _full_step(ctx, dt, pi0, mu0, S0):
    """One mlhip_em_step with the launch counters -> ((ll, resp, mixing, means, covariances with the ridge off), labels, launches)."""
    K = len(pi0)
    ctx.timing_enable(True)
    ctx.timing_reset()
    ll, pi1, mu1, S1 = dt.em_step(pi0, mu0, S0)
    launched = {name: _launches(ctx, name) for name in ("em_fused", "em_estep", "em_mstats", "em_refine", "em_weights")}
    ctx.timing_enable(False)
    resp, labels = dt.em_responsibilities(K), dt.em_labels(K)
    return (ll, resp, pi1, mu1, _ridge_off(S1, False)), labels, launched


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,shape,env,route", STEP_ROUTES, ids=[c[0] for c in STEP_ROUTES])
def test_em_step_edges(ctx, monkeypatch, name, shape, env, route, kind):
    X, pi0, mu0, S0, refs, moved, comps = _case(kind, *shape)
    _setenv(monkeypatch, env)
    dt = _data(ctx, X)
    taken = dt.em_route(len(pi0))
    _assert_route(taken, route)
    got, labels, launched = _full_step(ctx, dt, pi0, mu0, S0)
    dt.close()
    families = {key: launched[key] for key in ("em_fused", "em_estep", "em_mstats")}
    assert families == ({"em_fused": 1, "em_estep": 0, "em_mstats": 0} if taken["fused"] else {"em_fused": 0, "em_estep": 1, "em_mstats": 1}), launched
    # (the form is chosen at launch from the parameters: FOLD wherever the route allows it and every |W (mu - s)| entry is <= 64)
    fold = taken["estep"] == "matrix4" and taken["fold_allowed"] and refs["old"]["fold"].max() <= 64
    assert fold == (taken["estep"] == "matrix4" and taken["fold_allowed"] and kind != "far")      # (what the kinds are built for)
    label = f"{kind}: {name}"
    if kind == "hole":
        assert refs["old"]["fold"][refs["k"]] <= 1e-9
        if fold:                                             # the fast form ran: not the bits of the exact-form switch
            monkeypatch.setenv("MLHIP_ESTEP_FOLD", "0")
            dt = _data(ctx, X)
            _assert_route(dt.em_route(len(pi0)), {"estep": "matrix4", "fold_allowed": False})
            exact, _, _ = _full_step(ctx, dt, pi0, mu0, S0)
            dt.close()
            same = got[0] == exact[0] and np.array_equal(got[1], exact[1])
            label += f" [bits of the exact form: {same}, exact form's resp {hp.abs_err(exact[1], refs['ref'][1]):.1e}]"
            assert not same, label
    model = (FOLD_BOUND, "FOLD") if fold else (None, "")
    if kind == "tail":
        check_tail(label, got, labels, refs, moved, comps, launched["em_refine"], *model)
    else:
        check_massless(label, got, labels, refs, launched["em_refine"], *model)


REFINEMENT_ROUTES = {8: {"estep": "scalar_fed", "fused": True}, 32: {"estep": "matrix4", "fused": False}}


@pytest.mark.parametrize("d,first", hp_cases.MASSLESS_REFINEMENT_CASES)
def test_refinement_skips_the_dead_component_only(ctx, d, first):
    """test_gpu_hp_error.py's refinement problem just above MLHIP_REFINE_RATIO with a third component of weight 0 in front of /
    behind the live ones: ONE refinement launch -- the live component above the guard, held to the model at ratio 1 -- and none
    for the dead one, whose NaN mean and covariance must not reach the pass."""
    X, pi0, mu0, S0, k = hp_cases.massless_refinement_problem(d, 1.1e4, first)
    refs = edge_references(X, pi0, mu0, S0, k, False)
    assert (refs["ratio"] > 1e4).tolist() == [False, True], refs["ratio"]
    dt = _data(ctx, X)
    _assert_route(dt.em_route(3), REFINEMENT_ROUTES[d])
    got, labels, launched = _full_step(ctx, dt, pi0, mu0, S0)
    dt.close()
    assert launched["em_refine"] == 1, launched
    check_massless(f"zero weight {'in front of' if first else 'behind'} a refined component, d={d} ratio {refs['ratio'].max():.4g}", got, labels,
                   refs, launched["em_refine"])


# ---- diagonal covariances -----------------------------------------------------------------------------------------------------

def _diag_model(X, mu0, var0):
    """Section 4: 2^-53 max_k sum_j |b_kj| in a log-responsibility, b_kj = (mu_kj - shift_j) / sigma_kj."""
    b = np.abs((mu0 - X.mean(axis=0)) / np.sqrt(var0))
    return hp.EPS64 * float(b.sum(axis=1).max())


DIAG_ROUTES = [("diagonal two-operation form, K<=16", (16, 8, 4001, 0.5), {}, False),
               ("diagonal exact form, K<=16", (16, 8, 4001, 0.5), {"MLHIP_DIAG_AB": "0"}, True),
               ("diagonal two-operation form, K=17..64", (7, 40, 4001, 0.0), {}, False)]
assert {c[1] for c in DIAG_ROUTES} <= set(hp_cases.EDGE_DIAG_SHAPES)


def _diag_step(ctx, dt, pi0, mu0, var0):
    K = len(pi0)
    ctx.timing_enable(True)
    ctx.timing_reset()
    ll, pi1, mu1, var1 = dt.em_step_diag(pi0, mu0, var0)
    launched, refined = _launches(ctx, "em_diag"), _launches(ctx, "em_refine")
    ctx.timing_enable(False)
    assert launched >= 1
    return (ll, None, pi1, mu1, _ridge_off(var1, True)), refined


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,shape,env,exact", DIAG_ROUTES, ids=[c[0] for c in DIAG_ROUTES])
def test_em_diag_step_edges(ctx, monkeypatch, name, shape, env, exact, kind):
    """The diagonal kernel hands out no responsibilities of its own: mlhip_em_responsibilities / mlhip_em_labels rebuild them from
    the same parameters with the full-covariance E-step -- held to the column, label and row-sum conditions, not to an error limit."""
    X, pi0, mu0, var0, refs, moved, comps = _case(kind, *shape, True)
    K = len(pi0)
    _setenv(monkeypatch, env)
    dt = _data(ctx, X)
    _assert_route(dt.em_route(K, "diag"), {"diag_kernel": True, "diag_exact": exact})
    got, refined = _diag_step(ctx, dt, pi0, mu0, var0)
    resp, labels = dt.em_responsibilities(K), dt.em_labels(K)
    dt.close()
    fast = not exact and refs["old"]["b2"].max() <= 64.0 ** 2
    assert fast == (not exact and kind != "far")
    label = f"{kind}: {name} [B2 {refs['old']['b2'].max():.3g}]"
    if kind == "hole":
        assert refs["old"]["b2"][refs["k"]] <= 1e-18
        if fast:
            monkeypatch.setenv("MLHIP_DIAG_AB", "0")
            dt = _data(ctx, X)
            _assert_route(dt.em_route(K, "diag"), {"diag_kernel": True, "diag_exact": True})
            other, _ = _diag_step(ctx, dt, pi0, mu0, var0)
            dt.close()
            same = got[0] == other[0] and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got[2:], other[2:]))
            label += f" [bits of the exact form: {same}]"
            assert not same, label
    model = (_diag_model(X, mu0, var0), "2^-53 sum abs b") if fast else (None, "")
    if kind == "tail":
        assert len(moved) >= 8
        assert np.abs(resp.sum(axis=1) - 1).max() <= 4 * max(FLOOR, 2 * hp.EPS64 * refs["lse_max"]) and np.array_equal(labels[moved], comps)
        check_tail(label, got, None, refs, moved, comps, refined, *model)
    else:
        assert not resp[:, refs["k"]].any() and not (labels == refs["k"]).any()
        check_massless(label, got, None, refs, refined, *model)


# ---- row weights --------------------------------------------------------------------------------------------------------------

WEIGHTED_ROUTE = {"fused": False, "sparse": False, "resident": False, "diag_kernel": False}
# name, shape, E-step tier, whether the statistics kernel normalises (and weights) the log-responsibilities itself
WEIGHTED_ROUTES = [("weighted self-normalising, d=16 K=8", (16, 8, 4001, 2.0), "matrix4", True),
                   ("weighted w r passes, d=8 K=5", (8, 5, 3001, 3.0), "scalar_fed", False)]
assert {c[1] for c in WEIGHTED_ROUTES} <= set(hp_cases.EDGE_WEIGHTED_SHAPES)


@functools.lru_cache(maxsize=None)
def _weighted_case(kind, d, K, n, offset):
    """A kind's block with test_weights_cases.weights attached, the references on the REPLICATED sample (ratios and guard
    quantities about the block's shift, its unweighted column mean)."""
    w = weights(n)
    special = None
    if kind == "zero_weight_rows":
        X, w, pi0, mu0, S0, special = hp_cases.zero_weight_rows_problem(d, K, n, offset, w)
        k, moved, comps = K - 1, None, None
    elif kind == "tail":
        X, pi0, mu0, S0, moved, comps = hp_cases.tail_problem(d, K, n, offset)
        k = None
    else:
        X, pi0, mu0, S0, k = hp_cases.massless_problem(kind, d, K, n, offset)
        moved = comps = None
    return X, w, pi0, mu0, S0, edge_references(replicate(X, w), pi0, mu0, S0, k, False, shift_of=X), moved, comps, special


@pytest.mark.parametrize("kind", KINDS + ("zero_weight_rows",))
@pytest.mark.parametrize("name,shape,tier,self_norm", WEIGHTED_ROUTES, ids=[c[0] for c in WEIGHTED_ROUTES])
def test_weighted_step_edges(ctx, monkeypatch, name, shape, tier, self_norm, kind):
    """The step is weighted, the per-row results are not: responsibilities and labels cover every row of the block, and are held to
    the reference on the rows of positive weight (each repeated w_i times there)."""
    X, w, pi0, mu0, S0, refs, moved, comps, special = _weighted_case(kind, *shape)
    K = len(pi0)
    dt = _data(ctx, X, w)
    taken = dt.em_route(K)
    _assert_route(taken, dict(WEIGHTED_ROUTE, estep=tier, self_norm=self_norm))
    assert dt.weight_sum == float(w.sum())
    got, labels, launched = _full_step(ctx, dt, pi0, mu0, S0)
    dt.close()
    assert launched["em_fused"] == 0 and launched["em_estep"] == 1 and launched["em_mstats"] == 1, launched
    assert launched["em_weights"] == (0 if self_norm else 2), launched
    fold = tier == "matrix4" and taken["fold_allowed"] and refs["old"]["fold"].max() <= 64
    assert fold == (tier == "matrix4" and taken["fold_allowed"] and kind not in ("far", "zero_weight_rows"))
    model = (FOLD_BOUND, "FOLD") if fold else (None, "")
    label = f"{kind}: {name}"
    replicated = np.repeat(np.arange(len(X)), w.astype(np.int64))             # row of the block behind each row of the reference
    if kind == "hole" and fold:                              # the fast form ran: not the bits of the exact-form switch
        monkeypatch.setenv("MLHIP_ESTEP_FOLD", "0")
        dt = _data(ctx, X, w)
        _assert_route(dt.em_route(K), dict(WEIGHTED_ROUTE, estep=tier, self_norm=self_norm, fold_allowed=False))
        exact, _, _ = _full_step(ctx, dt, pi0, mu0, S0)
        dt.close()
        same = got[0] == exact[0] and np.array_equal(got[1], exact[1])
        label += f" [bits of the exact form: {same}, exact form's resp {hp.abs_err(exact[1][replicated], refs['ref'][1]):.1e}]"
        assert not same, label
    if kind == "zero_weight_rows":
        # alive on the block: the 40 rows belong to it wholly -- and carry no weight, so that it is massless on the weighted sample
        assert np.all(got[1][special, K - 1] == 1.0) and np.all(labels[special] == K - 1) and not w[special].any()
        rest = np.setdiff1d(np.arange(len(X)), special)
        held = (got[0], got[1][rest]) + tuple(got[2:])
        check_massless(label, held, labels[rest], refs, launched["em_refine"], *model, rows=np.searchsorted(rest, replicated))
    elif kind == "tail":
        check_tail(label, got, labels, refs, moved, comps, launched["em_refine"], *model, rows=replicated)
    else:
        check_massless(label, got, labels, refs, launched["em_refine"], *model, rows=replicated)


# ---- the loop after a component died ------------------------------------------------------------------------------------------

# name, kind, (d, K, N, offset), diagonal, switches, route, launches of ONE iteration (em_close: the device closing kernels, full and
# diagonal; the E-step / statistics family beside it; the resident kernel closes inside its one launch; host closing: no em_close)
LOOP_CASES = [
    ("closing on the device, d=16", "zero_weight_last", (16, 8, 4001, 2.0), False, {"MLHIP_RESIDENT": "0"}, {"device_close": True, "resident": False},
     {"em_close": 1, "em_estep": 1, "em_mstats": 1, "em_fused": 0, "em_diag": 0, "em_resident": 0}),
    ("panelled closing, d=72", "zero_weight_first", (72, 2, 2501, 0.0), False, {}, {"device_close": True, "records_on_device": True},
     {"em_close": 1, "em_estep": 1, "em_mstats": 1, "em_fused": 0, "em_diag": 0, "em_resident": 0}),
    ("closing on the host, d=16", "zero_weight_first", (16, 8, 4001, 2.0), False, {"MLHIP_DEVICE_CLOSE": "0"}, {"device_close": False},
     {"em_close": 0, "em_estep": 1, "em_mstats": 1, "em_fused": 0, "em_diag": 0, "em_resident": 0}),
    ("closing on the host, d=72", "zero_weight_last", (72, 2, 2501, 0.0), False, {"MLHIP_DEVICE_CLOSE": "0"},
     {"device_close": False, "records_on_device": False}, {"em_close": 0, "em_estep": 1, "em_mstats": 1, "em_fused": 0, "em_diag": 0, "em_resident": 0}),
    ("diagonal closing, d=16", "zero_weight_last", (16, 8, 4001, 0.5), True, {}, {"diag_kernel": True, "device_close": True},
     {"em_close": 1, "em_estep": 0, "em_mstats": 0, "em_fused": 0, "em_diag": 1, "em_resident": 0}),
    ("lagged loop of fused steps, d=8", "zero_weight_first", (8, 5, 3001, 3.0), False, {"MLHIP_RESIDENT": "0"},
     {"fused": True, "device_close": True, "resident": False}, {"em_close": 1, "em_estep": 0, "em_mstats": 0, "em_fused": 1, "em_diag": 0, "em_resident": 0}),
    # (the resident loop keeps the card to itself for the whole fit: last in the module)
    ("resident loop, d=2 K=3", "zero_weight_last", (2, 3, 3001, 0.0), False, {}, {"fused": True, "fused_form": "valu", "resident": True, "device_close": True},
     {"em_close": 0, "em_estep": 0, "em_mstats": 0, "em_fused": 0, "em_diag": 0, "em_resident": 1}),
]
assert {c[2] for c in LOOP_CASES if not c[3]} <= set(hp_cases.EDGE_SHAPES + hp_cases.EDGE_LOOP_SHAPES)


@pytest.mark.parametrize("name,kind,shape,diagonal,env,route,once", LOOP_CASES, ids=[c[0] for c in LOOP_CASES])
def test_loop_after_a_component_died(ctx, monkeypatch, name, kind, shape, diagonal, env, route, once):
    """One iteration of mlhip_em_iterate: the step's massless pattern through the closing. Two iterations: the component's NaN mean
    and covariance enter every row's log-sum-exp of the second E-step (log 0 + NaN = NaN), so the second log-likelihood and every
    parameter are NaN and the loop does not report convergence -- the oracle's two steps give the same (checked on the CPU)."""
    X, pi0, mu0, S0, refs, _, _ = _case(kind, *shape, diagonal)
    K, k = len(pi0), refs["k"]
    _setenv(monkeypatch, env)
    dt = _data(ctx, X)
    _assert_route(dt.em_route(K, "diag" if diagonal else "full"), route)
    ctx.timing_enable(True)
    ctx.timing_reset()
    steps, conv, ll, pi1, mu1, S1, hist = dt.em_iterate(pi0, mu0, S0, 1, diagonal=diagonal)
    launched = {key: _launches(ctx, key) for key in tuple(once) + ("em_refine",)}
    ctx.timing_enable(False)
    assert steps == 1 and ll == hist[0], (steps, ll, hist)
    assert {key: launched[key] for key in once} == once, launched
    check_massless(f"{kind}, one iteration: {name}", (ll, None, pi1, mu1, _ridge_off(S1, diagonal)), None, refs, launched["em_refine"])
    ctx.timing_enable(True)
    ctx.timing_reset()
    steps, conv, ll, pi2, mu2, S2, hist = dt.em_iterate(pi0, mu0, S0, 2, 1e-6, 1e-6, diagonal=diagonal)
    twice = {key: _launches(ctx, key) for key in once}
    ctx.timing_enable(False)
    dt.close()
    # two iterations: every launch of the one-iteration run twice (the lagged loop launches no third), the resident kernel once
    assert twice == {key: n if key == "em_resident" else 2 * n for key, n in once.items()}, twice
    assert steps == 2 and not conv and len(hist) == 2, (steps, conv, hist)
    e_first = abs(float((LD(hist[0]) - refs["ref"][0]) / refs["ref"][0]))
    print(f"HPERR {kind}, two iterations: {name} | first ll {e_first:.1e} / {refs['e_cpu']['ll']:.1e} | second ll {hist[1]} | "
          f"parameters all NaN: {bool(np.isnan(pi2).all() and np.isnan(mu2).all() and np.isnan(S2).all())}", flush=True)
    assert e_first <= 4 * max(refs["e_cpu"]["ll"], FLOOR)
    assert np.isnan(hist[1]) and np.isnan(ll)
    assert np.isnan(pi2).all() and np.isnan(mu2).all() and np.isnan(S2).all(), (pi2, mu2[k])
