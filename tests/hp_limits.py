"""The error norms and limit rules of the extended-precision error suites (tests/test_gpu_hp_error.py, tests/test_gpu_tied_hp.py,
tests/test_gpu_hp_edges.py) -- a plain module, no fixtures. The rules are stated in test_gpu_hp_error.py's
docstring; the checkers of test_gpu_hp_edges.py's inputs (a component without mass, rows far in a tail) live here too, so that
tests/test_hp_reference.py can show on the CPU that they reject a wrong result."""
import math

import numpy as np

from oracle import hp_cases
from oracle import hp_reference as hp

LD = np.longdouble
FLOOR = 8 * hp.EPS64
FOLD_BOUND = 1e-13                 # section 4: "<= ~1e-13 in a log-responsibility"


def _ridge_off(S, diagonal):
    """The library's covariances carry the reference's + 1e-15 I (ML/EM.cpp:252); the extended-precision ones do not."""
    S = np.asarray(S, dtype=LD)
    return S - LD(1e-15) if diagonal else S - LD(1e-15) * np.eye(S.shape[-1], dtype=LD)


def _errors(got, ref):
    """(ll relative, resp absolute or None, mixing, means max-norm relative, covariances per component) of a 5-tuple (a tied step: a stack of one covariance)."""
    return {"ll": abs(float((LD(got[0]) - ref[0]) / ref[0])),
            "resp": None if got[1] is None else hp.abs_err(got[1], ref[1]),
            "mixing": hp.rel_err(got[2], ref[2]), "means": hp.rel_err(got[3], ref[3]),
            "covs": np.array([hp.rel_err(got[4][k], ref[4][k]) for k in range(len(ref[4]))])}


def _report_and_check(name, e_gpu, e_cpu, ratio, estep_model=None, model_name="", ll_abs=1.0, refined=None, mix_max=1.0):
    """Prints the case's line, then asserts the limits of the module docstring. `estep_model`: the section 4 absolute bound of a
    fast density form in a log-responsibility -- the same absolute error in a responsibility (r <= 1) and in a sample's term of
    the mean log-likelihood, whose error is relative to `ll_abs` = |log-likelihood|, and in a mixing weight (the mean of a column of
    responsibilities), whose error is relative to `mix_max` = the largest weight. `refined`: the components the library recomputed
    about their own mean -- the two-pass form, held to the model at ratio 1."""
    model_ratio = np.where(refined, 1.0, ratio) if refined is not None else ratio
    worst = int(np.argmax(e_gpu["covs"] / np.maximum(e_cpu["covs"], 3e-15 * np.maximum(1.0, model_ratio))))
    fmt = lambda v: "-" if v is None else f"{v:.1e}"   # noqa: E731
    print(f"HPERR {name} | ll {fmt(e_gpu['ll'])} / {fmt(e_cpu['ll'])} | resp {fmt(e_gpu['resp'])} / {fmt(e_cpu['resp'])} | mixing "
          f"{fmt(e_gpu['mixing'])} / {fmt(e_cpu['mixing'])} | means {fmt(e_gpu['means'])} / {fmt(e_cpu['means'])} | covs[{worst}] "
          f"{fmt(e_gpu['covs'][worst])} / {fmt(e_cpu['covs'][worst])} ratio {ratio[worst]:.3g} (max {ratio.max():.3g})"
          + (f" | {model_name} {estep_model:.1e}" if estep_model is not None else "")
          + ("".join(f" | refined covs[{k}] {e_gpu['covs'][k]:.1e} / {e_cpu['covs'][k]:.1e}" for k in np.nonzero(refined)[0]) if refined is not None else ""),
          flush=True)
    failures = []
    for key in ("ll", "resp", "mixing", "means"):
        if e_gpu[key] is None:
            continue
        limit = 4 * max(e_cpu[key], FLOOR)
        if estep_model is not None and key in ("ll", "resp", "mixing"):
            limit = max(limit, 4 * estep_model / {"ll": ll_abs, "resp": 1.0, "mixing": mix_max}[key])
        if not e_gpu[key] <= limit:
            failures.append(f"{key}: {e_gpu[key]:.2e} > {limit:.2e}")
    limit = 4 * np.maximum(e_cpu["covs"], 3e-15 * np.maximum(1.0, model_ratio))
    for k in np.nonzero(~(e_gpu["covs"] <= limit))[0]:
        failures.append(f"covs[{k}]: {e_gpu['covs'][k]:.2e} > {limit[k]:.2e} (ratio {ratio[k]:.3g})")
    assert not failures, (name, failures)


# ---- K-means: tests/test_gpu_hp_error.py, tests/test_gpu_units.py ------------------------------------------------------------

def _fsum_centroids(X, labels, K):
    out = np.zeros((K, X.shape[1]))
    for k in range(K):
        sel = X[labels == k]
        if len(sel):
            out[k] = [math.fsum(sel[:, j]) / len(sel) for j in range(X.shape[1])]
    return out


def _check_kmeans(name, X, C0, got, labels, dists, ref, km):
    """Labels on every row the reference separates by more than 64 * 2^-53 * dist (the oracle is held to the same); distances and
    centroids against the reference at the rounding level, the inertia with the oracle's error as the yardstick; the update sums
    against math.fsum over the GPU's own labels."""
    inertia, _, counts, C1 = got
    dist, label, margin, ref_inertia, ref_counts, ref_new = ref
    safe = margin > 64 * hp.EPS64 * dist
    assert safe.mean() >= 0.999, safe.mean()                         # (a condition on the data, checked on the CPU too)
    assert np.array_equal(labels[safe], label[safe])
    assert np.array_equal(km.labels[safe], label[safe])
    same = np.array_equal(labels, label)
    e_dist = hp.rel_err(dists[safe], dist[safe])
    e_in, c_in = abs(float((LD(inertia) - ref_inertia) / ref_inertia)), abs(float((LD(km.inertia) - ref_inertia) / ref_inertia))
    K = C0.shape[0]
    exact = _fsum_centroids(X, labels, K)
    e_sum = float(np.max(np.abs(C1 - exact) / np.maximum(np.abs(exact), 1e-300)))       # per entry: the sums are exact
    print(f"HPERR {name} | left out {int((~safe).sum())} of {len(safe)} rows | labels == reference on all rows: {same} | "
          f"distances {e_dist:.1e} | inertia {e_in:.1e} / {c_in:.1e} | centroids vs fsum {e_sum:.1e}", flush=True)
    assert np.array_equal(counts, np.bincount(labels, minlength=K).astype(float))
    assert e_dist <= 4 * FLOOR and e_in <= 4 * max(c_in, FLOOR)
    assert e_sum <= 4e-16                                            # (the existing exactness test's bound)
    if same:
        assert np.array_equal(counts, ref_counts.astype(float)) and hp.rel_err(C1, ref_new) <= 4 * FLOOR


# ---- ill-conditioned covariances: tests/test_gpu_hp_ill.py -----------------------------------------------------------------------

def ill_errors(got, ref):
    """_errors with the means per component too (the whitening model's unit sqrt(N_k) 2^-53 kappa_k differs by orders of magnitude
    between a well and an ill conditioned component of one mixture)."""
    e = _errors(got, ref)
    e["means"] = np.array([hp.rel_err(got[3][k], ref[3][k]) for k in range(len(ref[3]))])
    return e


def ill_limits(ref, kappa, ratio, n, fold_ran):
    """The whitening model's limits: y = W (x - mu) loses kappa = |L|_inf |L^-1|_inf roundings, N_k samples
    add up like a random walk -- C_ILL[o] sqrt(N_k) 2^-53 kappa_k per component for means and covariances (never below the limits
    the well conditioned suites hold them to: 4 FLOOR, 4 * 3e-15 max(1, ratio_k)), C_ILL[o] sqrt(N) 2^-53 max kappa for the
    log-likelihood, the responsibilities and the mixing weights (never below 4 FLOOR), to which the FOLD form, where it ran, adds its
    own 4 FOLD_BOUND, scaled as _report_and_check scales it. The constants come from the fp64 restatement
    hp_cases.whitened_step_fp64 on the CPU; the oracle's error is no part of any limit."""
    n_k = n * np.asarray(ref[2], dtype=np.float64)
    whole = float(np.sqrt(n) * hp.EPS64 * np.max(kappa))
    per = np.sqrt(n_k) * hp.EPS64 * np.asarray(kappa)
    scale = {"ll": abs(float(ref[0])), "resp": 1.0, "mixing": float(np.max(ref[2]))}
    limits = {key: max(hp_cases.C_ILL[key] * whole, 4 * FLOOR) + (4 * FOLD_BOUND / scale[key] if fold_ran else 0.0) for key in scale}
    limits["means"] = np.maximum(hp_cases.C_ILL["means"] * per, 4 * FLOOR)
    limits["covs"] = np.maximum(hp_cases.C_ILL["covs"] * per, 4 * 3e-15 * np.maximum(1.0, ratio))
    return limits


def ill_needed(e, ref, kappa, ratio, n):
    """The constant each output of an ill_errors() dict needs under ill_limits() without FOLD: its error in the model's unit, 0 for
    an entry that its limit's floor already covers; means and covariances at their worst component."""
    n_k = n * np.asarray(ref[2], dtype=np.float64)
    whole = float(np.sqrt(n) * hp.EPS64 * np.max(kappa))
    per = np.sqrt(n_k) * hp.EPS64 * np.asarray(kappa)
    out = {key: (e[key] / whole if e[key] > 4 * FLOOR else 0.0) for key in ("ll", "resp", "mixing")}
    out["means"] = float(np.where(e["means"] > 4 * FLOOR, e["means"] / per, 0.0).max())
    out["covs"] = float(np.where(e["covs"] > 4 * 3e-15 * np.maximum(1.0, ratio), e["covs"] / per, 0.0).max())
    return out


def ill_references(d, K, n, cond):
    """Everything a case of tests/test_gpu_hp_ill.py compares with, from the CPU alone -> dict: the input (X, pi0, mu0, S0), lw (the
    reference's K x N log-weights), lse, ref (the reference step), old / new (conditioning of the input / of the reference's new
    parameters about the data mean), white (hp_cases.whitened_step_fp64's 6-tuple), e_white and e_oracle (their ill_errors)."""
    from oracle import oracle_ctypes as orc
    X, pi0, mu0, S0 = hp_cases.ill_problem(d, K, n, cond, seed=hp_cases.ill_seed(d, K, n, cond))
    lw = hp.log_weights(X, pi0, mu0, S0)
    resp, lse = hp._normalise(lw)
    ref = (lse.sum() / n, resp.T) + hp._close(hp._ld(X), resp, False)            # (hp.em_step, the log-weights kept)
    shift = X.astype(LD).mean(axis=0)
    white = hp_cases.whitened_step_fp64(X, pi0, mu0, S0)
    return {"X": X, "pi0": pi0, "mu0": mu0, "S0": S0, "lw": lw, "lse": lse, "ref": ref, "white": white,
            "old": hp.conditioning(shift, mu0, covs=S0), "new": hp.conditioning(shift, ref[3], covs=ref[4]),
            "e_white": ill_errors(white[:5], ref), "e_oracle": ill_errors(hp_cases.oracle_step(orc, X, pi0, mu0, S0), ref)}


def ill_failures(e, limits):
    """The outputs of an ill_errors() dict that lie over ill_limits(), as strings (resp may be None: not compared)."""
    failures = []
    for key in ("ll", "resp", "mixing"):
        if e[key] is not None and not e[key] <= limits[key]:
            failures.append(f"{key}: {e[key]:.2e} > {limits[key]:.2e}")
    for key in ("means", "covs"):
        for k in np.nonzero(~(e[key] <= limits[key]))[0]:
            failures.append(f"{key}[{k}]: {e[key][k]:.2e} > {limits[key][k]:.2e}")
    return failures


def check_ill(name, e_gpu, ref, kappa, ratio, n, fold_ran, e_white=None, e_oracle=None):
    """Prints the case's line -- per output err_gpu / err_whitened_fp64 / err_oracle, means and covariances at the component where
    the kernel is nearest to its limit --, then asserts ill_limits()."""
    limits = ill_limits(ref, kappa, ratio, n, fold_ran)
    fmt = lambda v: "-" if v is None else f"{v:.1e}"   # noqa: E731
    pick = lambda e, key, k: None if e is None or e[key] is None else (e[key] if k is None else e[key][k])   # noqa: E731
    parts = []
    for key in ("ll", "resp", "mixing", "means", "covs"):
        k = None if key in ("ll", "resp", "mixing") else int(np.argmax(e_gpu[key] / limits[key]))
        parts.append(f"{key}{'' if k is None else f'[{k}]'} {fmt(pick(e_gpu, key, k))} / {fmt(pick(e_white, key, k))} / {fmt(pick(e_oracle, key, k))}"
                     f" (limit {fmt(limits[key] if k is None else limits[key][k])})")
    print(f"HPERR {name} | kappa {np.max(kappa):.3g} | " + " | ".join(parts) + (" | FOLD ran" if fold_ran else ""), flush=True)
    failures = ill_failures(e_gpu, limits)
    assert not failures, (name, failures)


def ill_ll2_limit(n, kappa_new):
    """A second E-step's log-likelihood against the reference on the very fp64 parameters the library returned (ridge included):
    only the factorization of the NEW covariances and the density enter."""
    return max(hp_cases.C_ILL["ll2"] * float(np.sqrt(n) * hp.EPS64 * np.max(kappa_new)), 4 * FLOOR)


def ill_row_limit(n, kappa):
    """The per-row constant of a log-density (absolute), in the responsibilities' unit."""
    return max(hp_cases.C_ILL["lse"] * float(np.sqrt(n) * hp.EPS64 * np.max(kappa)), 4 * FLOOR)


def ill_decided_rows(lw, limit):
    """The rows of a K x N block of reference log-weights whose runner-up lies more than `limit` below the winner: an error of
    limit / 2 in each of the two cannot change their label."""
    order = np.sort(lw, axis=0)
    return np.asarray((order[-1] - order[-2]) > limit)


def check_ill_rows(name, dens, labels, lw, n, kappa):
    """em_score's per-row log-densities within ill_row_limit() of the reference's log-sum-exp, its labels the reference's on every
    decided row; at most 0.1 % of the rows may be undecided. Prints the case's line first."""
    limit = ill_row_limit(n, kappa)
    err = hp.abs_err(dens, hp._normalise(lw)[1])
    decided = ill_decided_rows(lw, limit)
    wrong = int((np.asarray(labels)[decided] != lw.argmax(axis=0)[decided]).sum())
    print(f"HPERR {name} | kappa {np.max(kappa):.3g} | per-row log-density {err:.1e} (limit {limit:.1e}) | undecided rows "
          f"{int((~decided).sum())} of {len(decided)} | wrong labels on decided rows {wrong}", flush=True)
    assert decided.mean() >= 0.999, (name, decided.mean())
    assert wrong == 0, (name, wrong)
    assert err <= limit, (name, err, limit)


# ---- the inputs of tests/test_gpu_hp_edges.py ----------------------------------------------------------------------------------

def finite_errors(e):
    """The oracle's errors as a yardstick: an error that is not finite (the oracle has no value there) counts as 0."""
    def clean(v):
        if v is None:
            return None
        if isinstance(v, np.ndarray):
            return np.where(np.isfinite(v), v, 0.0)
        return v if np.isfinite(v) else 0.0
    return {k: clean(v) for k, v in e.items()}


def live_part(step, live):
    """A step with the massless component's mean and covariance left out (compared as a NaN pattern instead)."""
    return (step[0], step[1], step[2], np.asarray(step[3])[live], np.asarray(step[4])[live])


def edge_references(X, pi0, mu0, S0, k, diagonal, shift_of=None):
    """The reference and the oracle on one input -> dict: ref, cpu (the oracle's step), live (the components compared entry by entry),
    e_cpu (the oracle's errors on the live part, non-finite ones 0), ratio (the live components' refinement ratios about the
    block's shift), old (conditioning of the parameters the E-step is called with), lse_max."""
    from oracle import oracle_ctypes as orc
    K = len(pi0)
    live = np.array([j for j in range(K) if j != k])
    ref = (hp.em_step_diag if diagonal else hp.em_step)(X, pi0, mu0, S0)
    with np.errstate(all="ignore"):
        cpu = hp_cases.oracle_step(orc, X, pi0, mu0, S0, diagonal)
        e_cpu = finite_errors(_errors(live_part(cpu, live), live_part(ref, live)))
    shift = (X if shift_of is None else shift_of).astype(LD).mean(axis=0)
    key = "variances" if diagonal else "covs"
    ratio = hp.conditioning(shift, ref[3][live], **{key: ref[4][live]})["ratio"]
    old = hp.conditioning(shift, mu0, **{key: S0})
    lw = (hp.log_weights_diag if diagonal else hp.log_weights)(X, pi0, mu0, S0)
    return {"ref": ref, "cpu": cpu, "live": live, "e_cpu": e_cpu, "ratio": ratio, "old": old,
            "lse_max": float(np.abs(lw.max(axis=0)).max()), "k": k}


def check_massless(name, got, labels, refs, refined, estep_model=None, model_name="", rows=None):
    """The massless pattern, then the live part within the module's limits. `rows`: the rows the reference holds (a weighted block:
    those of positive weight); got[1] None where the route hands out no responsibilities."""
    k, live, ref = refs["k"], refs["live"], refs["ref"]
    if got[1] is not None:
        assert not got[1][:, k].any(), f"{name}: a responsibility of the massless component is not exactly 0"
        assert not (labels == k).any(), f"{name}: a row is labelled with the massless component"
    assert got[2][k] == 0, (name, got[2][k])
    assert hp_cases.massless_pattern(got, k), f"{name}: not the massless pattern (finite ll {np.isfinite(got[0])}, mu_k {got[3][k]})"
    assert hp_cases.massless_pattern(refs["cpu"], k) and hp_cases.massless_pattern(ref, k)
    resp = got[1] if rows is None or got[1] is None else got[1][rows]
    e_gpu = _errors(live_part((got[0], resp) + tuple(got[2:]), live), live_part(ref, live))
    e_cpu = refs["e_cpu"] if resp is not None else dict(refs["e_cpu"], resp=None)
    above = refs["ratio"] > 1e4
    assert refined == int(above.sum()), (name, refined, refs["ratio"])
    _report_and_check(name, e_gpu, e_cpu, refs["ratio"], estep_model, model_name, abs(float(ref[0])), refined=above,
                      mix_max=float(ref[2].max()))


def check_tail(name, got, labels, refs, moved, comps, refined, estep_model=None, model_name="", rows=None):
    """Rows far in a tail: a finite log-likelihood (the mean of the per-row log-sum-exp: finite exactly when each of them is), rows
    summing to 1, the moved rows `moved` labelled with their own components `comps`, then the module's limits with
    2 * 2^-53 * lse_max -- the rounding of an fp64 log-weight of that size -- as the responsibilities' yardstick (the oracle has
    no finite value on such data). `rows` as in check_massless."""
    ref = refs["ref"]
    yard = 2 * hp.EPS64 * refs["lse_max"]
    assert np.isfinite(got[0]), f"{name}: a per-row log-sum-exp is not finite (log-likelihood {got[0]})"
    if got[1] is not None:
        assert np.abs(got[1].sum(axis=1) - 1).max() <= 4 * max(FLOOR, yard), name
        assert np.array_equal(labels[moved], comps), (name, labels[moved], comps)
    resp = got[1] if rows is None or got[1] is None else got[1][rows]
    e_gpu = _errors((got[0], resp) + tuple(got[2:]), ref)
    e_cpu = dict(refs["e_cpu"], resp=yard if resp is not None else None)
    above = refs["ratio"] > 1e4
    assert refined == int(above.sum()), (name, refined, refs["ratio"])
    _report_and_check(f"{name} [lse max {refs['lse_max']:.4g}]", e_gpu, e_cpu, refs["ratio"], estep_model, model_name, abs(float(ref[0])),
                      refined=above, mix_max=float(ref[2].max()))
