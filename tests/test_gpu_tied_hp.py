"""How far the tied-covariance EM routes (the one-kernel route, device/em_tied.hip, and the composed route)
are from the TRUE value: each route, the CPU oracle (its full-covariance step on K copies of the covariance, pooled:
hp_cases.oracle_tied_step) and the extended-precision reference (hp.em_step_tied) on the same inputs, in the norms and under the
limit rules of tests/test_gpu_hp_error.py (tests/hp_limits.py). Needs a GPU:
`timeout -k 10 900 pytest tests/test_gpu_tied_hp.py -m gpu -x -s`.

Every case first asserts em_tied_route(K) and that timer `em_tied` launched once (kernel) or not at all (composed), and prints one
`HPERR` line (DESIGN.md section 4.1 holds the table of one run). Limits, none taken from what a route was seen to give:

* means:  err_gpu <= 4 max(err_cpu, 8 * 2^-53);
* mixing weights, log-likelihood, responsibilities: the same, and on the KERNEL route additionally the whitening model of section
  3.3i, 4 c 2^-53 whiten -- absolute in a log-responsibility, so relative to |log-likelihood| and to the largest mixing weight as
  the FOLD allowance is; whiten from hp.tied_conditioning(), c = hp_cases.C_WHITEN from the CPU restatement of the kernel's whitening
  order (tests/test_hp_reference.py measures it);
* the covariance, kernel route:    err_gpu <= 4 max(err_cpu, 3e-15 max(1, tratio)),  tratio = max_j (T / N)_jj / Sigma_jj;
* the covariance, composed route:  err_gpu <= 4 max(err_cpu, 3e-15 max(1, max_k ratio_k)), the full-covariance model (ratio_k of the
  K per-component covariances the route pools; a component the route refined counts with ratio 1, and the refinement launches are
  counted against the components above MLHIP_REFINE_RATIO as test_refinement_guard_sweep does).

Where the oracle has no finite value (its linear-domain densities underflow on far rows, the divergence section 4 documents) err_cpu
counts as 0: the limit is then the floor or the model alone."""
import functools

import numpy as np
import pytest

from oracle import hp_cases
from oracle import hp_reference as hp
from hp_limits import FLOOR, _errors, _report_and_check, _ridge_off

pytestmark = pytest.mark.gpu

LD = np.longdouble
ROUTES = ("kernel", "composed")


@pytest.fixture(scope="module")
def ctx():
    from ml_amd import _lib
    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def num_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _launches(ctx, name):
    return ctx.timing_get(name)[1]


def _step(ctx, monkeypatch, route, X, pi0, mu0, S0, w=None):
    """One mlhip_em_step_tied on `route` -> ((ll, responsibilities, mixing, means, [covariance, ridge off]), labels, refinement launches)."""
    from ml_amd import _lib
    monkeypatch.setenv("MLHIP_TIED", route)
    K = len(pi0)
    dt = _lib.Data(ctx, np.ascontiguousarray(X, dtype=np.float64))
    if w is not None:
        dt.set_weights(w)
    assert dt.em_tied_route(K) == route
    ctx.timing_enable(True)
    ctx.timing_reset()
    ll, pi1, mu1, S1 = dt.em_step_tied(pi0, mu0, S0)
    launched, refined = _launches(ctx, "em_tied"), _launches(ctx, "em_refine")
    ctx.timing_enable(False)
    assert launched == (1 if route == "kernel" else 0), (route, launched)
    resp, labels = dt.em_responsibilities(K), dt.em_labels(K)
    dt.close()
    assert np.array_equal(S1, S1.T, equal_nan=True)
    return (ll, resp, pi1, mu1, _ridge_off(S1, False)[None]), labels, refined


def _finite(e_cpu):
    """The oracle's errors as a yardstick: an error that is not finite (the oracle has no value there) counts as 0."""
    clean = lambda v: v if v is None else np.where(np.isfinite(v), v, 0.0) if isinstance(v, np.ndarray) else (v if np.isfinite(v) else 0.0)  # noqa: E731
    return {k: clean(v) for k, v in e_cpu.items()}


def _as_stack(step):
    return tuple(step[:4]) + (np.asarray(step[4])[None],)


def _composed_ratio(X, shift, resp):
    """hp.conditioning()'s `ratio` of the per-component M-step of `resp` (a component of fewer than d rows has no Cholesky factor,
    so not through conditioning() itself): max_j (mu_kj - shift_j)^2 / Sigma_k,jj."""
    _, means, covs = hp.m_step(X, resp)
    return np.array([float(((means[k] - shift) ** 2 / np.diag(covs[k])).max()) for k in range(len(means))])


def _references(X, pi0, mu0, S0, composed=True):
    """(reference step with the covariance as a stack of one, the oracle's errors, tied_conditioning of the step, the composed
    route's per-component ratios -- NaN for a component without mass; None unless `composed`: a second M-step in long double)."""
    from oracle import oracle_ctypes as orc
    ref = hp.em_step_tied(X, pi0, mu0, S0)
    with np.errstate(all="ignore"):
        e_cpu = _finite(_errors(_as_stack(hp_cases.oracle_tied_step(orc, X, pi0, mu0, S0)), _as_stack(ref)))
    shift = X.astype(LD).mean(axis=0)
    cond = hp.tied_conditioning(X, shift, mu0, S0, ref[4], resp=ref[1])
    if not composed:
        return _as_stack(ref), e_cpu, cond, None
    live = np.nonzero(np.asarray(ref[2] > 0))[0]
    ratio = np.full(len(pi0), np.nan)
    ratio[live] = _composed_ratio(X, shift, ref[1][:, live])
    return _as_stack(ref), e_cpu, cond, ratio


def _check(name, route, got, refined, refs, resp=True):
    """The module docstring's limits for one step on one route."""
    ref, e_cpu, cond, ratio = refs
    if not resp:
        got, e_cpu = got[:1] + (None,) + got[2:], dict(e_cpu, resp=None)
    e_gpu = _errors(got, ref)
    tag = f"tied {route}: {name} [tratio {cond['tratio']:.3g}, reach {cond['reach']:.3g}, whiten {cond['whiten']:.3g}"
    if route == "kernel":
        assert refined == 0
        _report_and_check(tag + "]", e_gpu, e_cpu, np.array([cond["tratio"]]), hp_cases.C_WHITEN * hp.EPS64 * cond["whiten"],
                          "c 2^-53 whiten", abs(float(ref[0])), mix_max=float(ref[2].max()))
    else:
        above = np.nan_to_num(ratio) > 1e4
        assert refined == int(above.sum()), (refined, ratio)
        model = float(np.nanmax(np.where(above, 1.0, ratio)))
        _report_and_check(tag + f", ratio_k max {np.nanmax(ratio):.3g}, refine launches {refined}, model ratio {model:.3g}]", e_gpu, e_cpu,
                          np.array([model]))


# ---- a. every code object of the kernel ------------------------------------------------------------------------------------

@pytest.mark.parametrize("d,K", hp_cases.TIED_CODE_OBJECT_CASES)
def test_every_code_object(ctx, monkeypatch, d, K):
    """All 12 padded dimensions x 1, 2 and 3 row blocks of components (and K = 16 / 17, 32 / 33, 48 / 49, 64), d just below the
    padded dimension so that the padded coordinates and the zero slot of the second column block are in use; 12 tiles, the last one
    ragged, in 3 workgroups. Responsibilities and labels through em_responsibilities / em_labels."""
    X, pi0, mu0, S0 = hp_cases.tied_problem(d, K, hp_cases.TIED_N, 2.0, 2.5)
    refs = _references(X, pi0, mu0, S0, composed=False)
    got, labels, refined = _step(ctx, monkeypatch, "kernel", X, pi0, mu0, S0)
    top = np.sort(refs[0][1], axis=1)
    clear = (top[:, -1] - top[:, -2]) > 1e-9                 # (>= 99.9 % of the rows: tests/test_hp_reference.py, on the CPU)
    assert clear.mean() >= 0.999
    assert np.array_equal(labels[clear], refs[0][1].argmax(axis=1)[clear])
    _check(f"code object d={d} K={K} N={hp_cases.TIED_N}", "kernel", got, refined, refs)


# ---- b. many tiles per wave -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d,K", [(3, 2), (21, 5), (32, 40)])
def test_many_tiles_per_wave(ctx, num_cus, monkeypatch, d, K):
    """N = 2 whole tiles per wave of the launch + 37 rows: the first waves take a third, ragged tile -- the tile loop's reuse of the
    wave's LDS tiles, the accumulators carried over tiles and the padding of the last tile. d = 3, K = 2: two workgroups per CU;
    d = 21, K = 5: one; d = 32, K = 40: two row-block groups (against the fp64 restatement at tests/test_gpu_tied.py's tolerances:
    the long-double reference would take most of a minute there). The step run twice gives identical bits."""
    cus = num_cus
    n = hp_cases.tied_many_tiles_rows(d, K, cus)
    grid = hp_cases.tied_grid(d, K, n, cus)
    assert (n + 63) // 64 >= 2 * 4 * grid + 1                # wave 0 of workgroup 0: tiles 0, 4 grid and 8 grid
    X, pi0, mu0, S0 = hp_cases.tied_problem(d, K, n, 2.0, 2.5)
    got, labels, refined = _step(ctx, monkeypatch, "kernel", X, pi0, mu0, S0)
    again, labels2, _ = _step(ctx, monkeypatch, "kernel", X, pi0, mu0, S0)
    assert got[0] == again[0] and all(np.array_equal(a, b) for a, b in zip(got[1:], again[1:])) and np.array_equal(labels, labels2)
    if K == 40:
        ll, resp, pi1, mu1, S1 = hp_cases.tied_step_fp64(X, pi0, mu0, S0)
        err = (abs(got[0] - ll) / abs(ll), float(np.abs(got[1] - resp).max()), hp.rel_err(got[2], pi1), hp.rel_err(got[3], mu1),
               hp.rel_err(got[4][0], S1 - 1e-15 * np.eye(d)))
        print(f"HPERR tied kernel: many tiles d={d} K={K} N={n} ({cus} CUs, grid {grid}) against the fp64 restatement | ll {err[0]:.1e} | "
              f"resp {err[1]:.1e} | mixing {err[2]:.1e} | means {err[3]:.1e} | cov {err[4]:.1e}", flush=True)
        assert err[0] <= 1e-12 and err[1] < 1e-12 and err[2] < 1e-11 and err[3] < 1e-11 and err[4] < 1e-10
        return
    _check(f"many tiles d={d} K={K} N={n} ({cus} CUs, grid {grid})", "kernel", got, refined,
           _references(X, pi0, mu0, S0, composed=False))


# ---- c. conditioning sweep, d. whitening reach -----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _sweep_case(offset, sep):
    problem = hp_cases.tied_problem(8, 5, 3001, offset, sep)
    return problem, _references(*problem)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("offset,sep", hp_cases.TIED_SWEEP_CASES)
def test_conditioning_sweep(ctx, monkeypatch, offset, sep, route):
    """Component means 2.5, 30 and 300 per axis apart: Sigma = T / N - sum_k pi_k mu~_k mu~_k^T cancels log10(tratio) digits on the
    kernel route; the composed route pools two-pass-like per-component covariances and refines above the guard."""
    problem, refs = _sweep_case(offset, sep)
    got, _, refined = _step(ctx, monkeypatch, route, *problem)
    _check(f"sweep offset={offset:g} sep={sep:g}", route, got, refined, refs)


@functools.lru_cache(maxsize=None)
def _reach_case(reach):
    problem = hp_cases.tied_reach_problem(reach)
    return problem, _references(*problem)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("reach", hp_cases.TIED_REACHES)
def test_whitening_reach(ctx, monkeypatch, reach, route):
    """Two overlapping components 0.9, 1.1 and 10 x 64 whitened units from the shift (>= 500 rows with responsibilities strictly
    inside (0, 1)): the kernel has no guard on |L^-1 (mu_k - shift)| and no exact form, and is held to its own model at every reach.

    The composed route takes the exact form of the full-covariance E-step at every reach (runtime/route.cpp, em_route for the tied mode): with the
    FOLD form, which the full-covariance mode runs below 64, its responsibilities at reach 0.9 x 64 were 1.10e-14 against a limit of
    9.08e-15 = 4 err_cpu; the exact form gives 1.9e-15."""
    problem, refs = _reach_case(reach)
    soft = int(((refs[0][1] > 1e-3) & (refs[0][1] < 1 - 1e-3)).any(axis=1).sum())
    assert soft >= 500
    got, _, refined = _step(ctx, monkeypatch, route, *problem)
    _check(f"reach {reach:g}, {soft} soft rows", route, got, refined, refs)


# ---- e. edges ---------------------------------------------------------------------------------------------------------------

ROUTE_TOLERANCES = (1e-12, 1e-12, 1e-11, 1e-11, 1e-10)      # tests/test_gpu_tied.py: ll, responsibilities, mixing, means, covariance


def _routes_agree(a, b):
    assert abs(a[0] - b[0]) <= ROUTE_TOLERANCES[0] * abs(b[0]) and np.abs(a[1] - b[1]).max() < ROUTE_TOLERANCES[1]
    for x, y, tol in zip(a[2:], b[2:], ROUTE_TOLERANCES[2:]):
        keep = np.isfinite(np.asarray(y, dtype=np.float64))
        assert not keep.any() or hp.rel_err(np.asarray(x)[keep], np.asarray(y)[keep]) < tol


@pytest.mark.parametrize("kind,empty", [("zero_weight", 2), ("empty", 4)])
def test_component_without_mass(ctx, monkeypatch, kind, empty):
    """A mixing weight of exactly 0 (c_k = -inf on a real record) and a component 1e4 whitened units from all data: every
    responsibility of the component is exactly 0. Both routes (and the oracle) then give pi_k = 0, mu_k = 0 / 0 = NaN and -- the
    empty component's NaN mean enters every entry of the pooled covariance with weight 0 -- a covariance that is NaN throughout
    (section 3.3i); everything else is held to the reference, whose covariance leaves the empty component out."""
    from oracle import oracle_ctypes as orc
    problem = hp_cases.tied_edge_problem(kind)
    ref, _, cond, ratio = _references(*problem)
    live = [k for k in range(len(problem[1])) if k != empty]
    assert ref[2][empty] == 0 and not ref[1][:, empty].any()
    # held to the reference: everything but the empty component's mean and the covariance (compared below as a finite / NaN pattern;
    # the reference's own stands in for it on every side: error 0)
    part = lambda s: (s[0], s[1], s[2], np.asarray(s[3])[live], ref[4])   # noqa: E731
    with np.errstate(all="ignore"):
        e_cpu = _finite(_errors(part(hp_cases.oracle_tied_step(orc, *problem)), part(ref)))
    results = {}
    for route in ROUTES:
        got, _, refined = _step(ctx, monkeypatch, route, *problem)
        assert got[2][empty] == 0 and not got[1][:, empty].any()
        assert np.isnan(got[3][empty]).all() and np.isfinite(got[3][live]).all() and np.isfinite(got[0])
        results[route] = got
        _check(f"{kind} (component {empty}); covariance all NaN: {bool(np.isnan(got[4].astype(np.float64)).all())}", route, part(got), refined,
               (part(ref), e_cpu, cond, ratio))
    a, b = results["kernel"], results["composed"]
    assert np.array_equal(np.isnan(a[3]), np.isnan(b[3]))
    assert np.array_equal(np.isnan(a[4].astype(np.float64)), np.isnan(b[4].astype(np.float64)))
    assert np.isnan(a[4].astype(np.float64)).all()            # the pattern section 3.3i documents
    _routes_agree(a, b)


def test_rows_far_in_every_tail(ctx, monkeypatch):
    """Twenty rows 40 whitened units from the nearest mean (log-densities near -800, where the oracle's linear-domain sum has
    underflowed: no CPU yardstick, the limits are the floor, the models and the rounding of an fp64 log-weight of that size): every
    per-row log-sum-exp finite -- the log-likelihood is their mean --, the responsibilities of every row sum to 1."""
    problem = hp_cases.tied_edge_problem("tail")
    X, pi0, mu0, S0 = problem
    refs = _references(*problem)
    assert FLOOR >= max(refs[1]["ll"], refs[1]["mixing"], refs[1]["means"])      # (the oracle: not finite, counted as 0)
    # r_k = exp(lw_k - lse): in fp64 lw_k and lse each carry a rounding of 2^-53 of their size, which the difference keeps -- on ANY
    # log-domain route, so this stands in for the oracle's error in a responsibility, and a row's responsibilities sum to 1 within
    # it: 2 * 2^-53 * |lse|, |lse| = 800 on the far rows (x 4 as everywhere)
    lse_max = float(np.abs(hp.log_weights(X, pi0, mu0, np.stack([S0] * len(pi0))).max(axis=0)).max())
    assert 790 < lse_max < 830
    refs = (refs[0], dict(refs[1], resp=2 * hp.EPS64 * lse_max)) + refs[2:]
    results = {}
    for route in ROUTES:
        got, _, refined = _step(ctx, monkeypatch, route, *problem)
        assert np.isfinite(got[0]) and np.abs(got[1].sum(axis=1) - 1).max() <= 4 * max(FLOOR, 2 * hp.EPS64 * lse_max)
        _check("twenty rows 40 whitened units out", route, got, refined, refs)
        results[route] = got
    _routes_agree(results["kernel"], results["composed"])


# ---- f. a weighted step, a chain of steps -----------------------------------------------------------------------------------

def test_weighted_composed_step(ctx, monkeypatch):
    """Row weights in {0, 1, 2, 3}: the composed route (the kernel has no weighted form) against the weighted reference, with the
    oracle's step on the replicated sample as the yardstick."""
    from oracle import oracle_ctypes as orc
    X, pi0, mu0, S0 = hp_cases.tied_problem(8, 5, 3001, 2.0, 2.5)
    w = np.random.default_rng(2024).integers(0, 4, len(X)).astype(np.float64)
    Xr = np.ascontiguousarray(np.repeat(X, w.astype(np.int64), axis=0))
    ref = _as_stack(hp.em_step_tied(X, pi0, mu0, S0, w))
    no_resp = lambda s: (s[0], None) + tuple(s[2:])   # noqa: E731   (per row of the replicated sample on the oracle's side)
    e_cpu = _errors(no_resp(_as_stack(hp_cases.oracle_tied_step(orc, Xr, pi0, mu0, S0))), no_resp(ref))
    shift = Xr.astype(LD).mean(axis=0)                                        # (the weighted data mean)
    resp_r = np.repeat(ref[1], w.astype(np.int64), axis=0)
    cond = hp.tied_conditioning(Xr, shift, mu0, S0, ref[4][0], resp=resp_r)
    ratio = _composed_ratio(Xr, shift, resp_r)
    got, _, refined = _step(ctx, monkeypatch, "composed", X, pi0, mu0, S0, w)
    _check("weighted step d=8 K=5 N=3001", "composed", got, refined, (ref, e_cpu, cond, ratio), resp=False)


@pytest.mark.parametrize("route", ROUTES)
def test_four_step_chain(ctx, monkeypatch, route):
    """em_iterate(tied=True), 4 iterations, against 4 reference steps (each fed the previous one's extended-precision parameters,
    + 1e-15 I as the library adds it, as test_resident_em_loop_error does) and the oracle's 4 steps. whiten: the largest of the 4
    steps."""
    from ml_amd import _lib
    from oracle import oracle_ctypes as orc
    d, K = 8, 5
    X, pi0, mu0, S0 = hp_cases.tied_problem(d, K, 3001, 2.0, 2.5)
    shift = X.astype(LD).mean(axis=0)
    pi, mu, S, whiten = pi0, mu0, S0, 0.0
    cp, cm, cS = pi0, mu0, S0
    for _ in range(4):
        ref = hp.em_step_tied(X, pi, mu, S)
        whiten = max(whiten, hp.tied_conditioning(X, shift, mu, S, ref[4], resp=ref[1])["whiten"])
        cond = hp.tied_conditioning(X, shift, mu, S, ref[4])
        pi, mu, S = ref[2], ref[3], ref[4] + LD(1e-15) * np.eye(d, dtype=LD)
        cpu = hp_cases.oracle_tied_step(orc, X, cp, cm, cS)
        cp, cm, cS = cpu[2], cpu[3], (cpu[4] + LD(1e-15) * np.eye(d, dtype=LD)).astype(np.float64)
    ratio = _composed_ratio(X, shift, ref[1])
    monkeypatch.setenv("MLHIP_TIED", route)
    dt = _lib.Data(ctx, X)
    assert dt.em_tied_route(K) == route
    ctx.timing_enable(True)
    ctx.timing_reset()
    steps, _, ll, pi1, mu1, S1, hist = dt.em_iterate(pi0, mu0, S0, 4, tied=True)
    launched, refined = _launches(ctx, "em_tied"), _launches(ctx, "em_refine")
    ctx.timing_enable(False)
    dt.close()
    assert steps == 4 and launched == (4 if route == "kernel" else 0) and ll == hist[-1]
    strip = lambda s: (s[0], None, s[2], s[3], np.asarray(s[4])[None])   # noqa: E731
    _check("chain of 4 iterations d=8 K=5 N=3001", route, (ll, None, pi1, mu1, _ridge_off(S1, False)[None]), refined,
           (strip(ref), _errors(strip(cpu), strip(ref)), dict(cond, whiten=whiten), ratio), resp=False)
