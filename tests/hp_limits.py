"""The error norms and limit rules of the extended-precision error suites (tests/test_gpu_hp_error.py, tests/test_gpu_tied_hp.py;
DESIGN.md section 4.1) -- a plain module, no fixtures. The rules are stated in test_gpu_hp_error.py's docstring."""
import numpy as np

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
