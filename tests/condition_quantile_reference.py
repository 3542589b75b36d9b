"""numpy restatement of the conditional CDF's and quantile's definitions (include/mlhip.h, mlhip_em_conditional_cdfs and
mlhip_em_conditional_quantiles): given x_O, missing coordinate j follows the one-dimensional mixture sum_k r_k N(t_kj, s_kj^2),
    F_j(v) = sum_k r_k Phi((v - t_kj) / s_kj),        quantile: the v with F_j(v) = p S,  S = sum_k r_k,
in float64 (Phi: scipy.special.ndtr) and in np.longdouble (Phi: ncdf_ld below, held to mpmath at 40 digits by
tests/test_condition_quantile_host.py), and the limits a device result is held to against the longdouble form. The responsibilities r
and the component predictions t (named `m` there) come from tests/condition_reference.py, the conditioned covariances from
tests/condition_variance_reference.py. A helper, not a test, and it imports nothing from the code under test.

The limits. u = 2^-53, gamma_n = n u / (1 - n u).
  t chain    the kernel's t_kj = mu_M + sum_c A_jc (x_c - mu_O,c), dO fused multiply-adds behind dO subtractions, and the subtraction
             v - t behind it:  |dt_ikj| <= E_ikj = gamma_{dO+2} (|mu_k,M[j]| + sum_c |A_k[j][c]| |x_ic - mu_k,O[c]|)   (Higham, 3.1).
  CDF        err = max |F - F_ld| / max |F_ld|   (max |F_ld| is 1 to within the case's tail)
             err <= 4 max(err_f64, FLOOR) + max_ij sum_k |r^E_ik - r^ld_ik| Phi_ikj + max_ij sum_k r^ld_ik phi(a_ikj) / s_kj E_ikj
             -- the float64 restatement's own error, the existing E-step kernels' error in the responsibilities (theirs, not the new
             kernel's), and what the chain's rounding moves F by: dF = sum_k r_k phi(a) w dt. No term comes from the code under test.
  quantile   a certificate, not a distance:  F_ld(v - h) - lim <= p S_ld <= F_ld(v + h) + lim,  with
             h_ij = max_k E_ikj: shifting every t_kj by at most E is shifting v by at most E;  lim = the CDF limit above, evaluated
             at v. Nothing is granted for the search's stop rule: what it leaves of |F - p S| has to fit the CDF's own limit, and
             the device's CDF at its own quantile is held to that limit of p S as well.

ncdf_ld is this module's own longdouble Phi (a series and a continued fraction), not mpmath's: mpmath on every (row, component,
coordinate) of every case, three times per probability, takes minutes. tests/test_condition_quantile_host.py holds ncdf_ld to mpmath
at 40 digits (7e-18 for |a| <= 20, 2.8e-17 to a = -37), two orders below the limits it carries."""
import functools

import numpy as np

import condition_reference as cref
import condition_variance_reference as vref

LD = cref.LD
U = 2.0 ** -53


def ncdf_ld(a):
    """Phi(a) elementwise in np.longdouble. |a| <= 3: Phi(-t) = 1/2 - phi(t) sum_n t^(2n+1) / (2n+1)!! (all terms of one sign);
    beyond: Phi(-t) = phi(t) / (t + 1 / (t + 2 / (t + 3 / ...))) to depth 300, evaluated from the bottom."""
    a = np.asarray(a, dtype=LD)
    t = np.minimum(np.abs(a), LD(60))
    phi = np.exp(-t * t / LD(2)) / np.sqrt(LD(2) * pi_ld())
    lower = np.full(t.shape, LD(np.nan))
    flat, flat_t, flat_phi = lower.reshape(-1), t.reshape(-1), phi.reshape(-1)
    small = flat_t <= LD(1.5)                                    # (beyond, 1/2 - phi sum cancels too many digits)
    x = flat_t[small]
    term, total = x.copy(), x.copy()
    for n in range(1, 60):
        term = term * x * x / LD(2 * n + 1)
        total = total + term
    flat[small] = LD(0.5) - flat_phi[small] * total
    for region, depth in (((flat_t > LD(1.5)) & (flat_t <= LD(3)), 2500), (flat_t > LD(3), 300)):
        x = flat_t[region]
        cf = x.copy()
        for n in range(depth, 0, -1):
            cf = x + LD(n) / cf
        flat[region] = flat_phi[region] / cf
    out = np.where(a > 0, LD(1) - lower, lower)
    return np.where(np.isnan(a), LD(np.nan), out)


@functools.lru_cache(maxsize=None)
def pi_ld():
    """pi in longdouble (np.pi is a float64): 4 atan(1) evaluated in longdouble."""
    return LD(4) * np.arctan(LD(1))


def npdf(a):
    a = np.asarray(a)
    dtype = a.dtype.type
    return np.exp(-a * a / dtype(2)) / np.sqrt(dtype(2) * (pi_ld() if dtype is LD else dtype(np.pi)))


def ncdf(a):
    """Phi in the array's dtype: ncdf_ld, or scipy.special.ndtr for float64."""
    a = np.asarray(a)
    if a.dtype.type is LD:
        return ncdf_ld(a)
    from scipy.special import ndtr
    return ndtr(a)


def nquantile(p, dtype=np.float64):
    """Phi^-1(p) in `dtype`: float64 through scipy.special.ndtri, refined in longdouble by Newton steps on ncdf_ld."""
    from scipy.special import ndtri
    z = np.asarray(ndtri(np.asarray(p, dtype=np.float64)), dtype=LD)
    if dtype is np.float64:
        return z.astype(np.float64)
    p = np.asarray(p, dtype=LD)
    for _ in range(3):
        z = z - (ncdf_ld(z) - p) / npdf(z)
    return z


def scales(C):
    """s_kj = sqrt(C_k[j][j]) in C's dtype -> K x dM."""
    dM = C.shape[1]
    return np.sqrt(C[:, np.arange(dM), np.arange(dM)])


def cdf(r, m, s, values):
    """F_j(v_ij) = sum_k r_ik Phi((v_ij - t_ikj) / s_kj) in the arrays' dtype -> N x dM. values: N x dM."""
    a = (np.asarray(values, dtype=r.dtype)[:, None, :] - m) / s[None]
    return (r[:, :, None] * ncdf(a)).sum(axis=1)


def density(r, m, s, values):
    """f_j(v_ij) = sum_k r_ik phi(a_ikj) / s_kj."""
    a = (np.asarray(values, dtype=r.dtype)[:, None, :] - m) / s[None]
    return (r[:, :, None] * npdf(a) / s[None]).sum(axis=1)


def component_quantiles(m, s, p, dtype):
    """q_ikj = t_ikj + s_kj z(p) -> N x K x dM."""
    z = nquantile(p, dtype)
    return m + s[None] * z


def quantile(r, m, s, p):
    """The v with F_j(v) = p S for one probability p, by bisection inside [min_k q_k, max_k q_k] over the components with a share until the
    bracket has collapsed, in the arrays' dtype -> N x dM."""
    dtype = r.dtype.type
    q = component_quantiles(m, s, p, dtype)
    share = (r != 0)[:, :, None]
    lo = np.where(share, q, dtype(np.inf)).min(axis=1)
    hi = np.where(share, q, dtype(-np.inf)).max(axis=1)
    T = (dtype(p) * r.sum(axis=1))[:, None]
    for _ in range(200):
        mid = lo + (hi - lo) / dtype(2)
        inside = (lo < mid) & (mid < hi)
        if not inside.any():
            break
        below = cdf(r, m, s, mid) < T
        lo = np.where(inside & below, mid, lo)
        hi = np.where(inside & ~below, mid, hi)
    return hi


def chain_error(c, parameters=None):
    """E_ikj of the module docstring from the longdouble restatement's conditioning -> N x K x dM (longdouble)."""
    mu_o, _, A, mu_m, _ = cref.condition(c["means"], c["covs"], c["observed"], LD)
    X = np.asarray(c["X_observed"], dtype=LD)
    dO = X.shape[1]
    z = np.abs(X[:, None, :] - mu_o[None])                       # N x K x dO
    reach = np.abs(mu_m)[None] + np.einsum("kjc,nkc->nkj", np.abs(A), z)
    n = dO + 2
    return LD(n * U / (1 - n * U)) * reach


def make_values(c, seed):
    """A value per (row, missing coordinate) where the mixture has its mass: the prediction of a component drawn for the row plus that
    component's scale times a normal deviate -- every eighth row 6 scales out, in the tails."""
    rng = np.random.default_rng(seed)
    m, s = c["f64"]["m"], scales(c["C64"])
    n, K, dM = m.shape
    k = rng.integers(0, K, size=n)
    dev = rng.standard_normal((n, dM))
    dev[::8] *= 6.0
    return np.ascontiguousarray(m[np.arange(n), k] + s[k] * dev)


@functools.lru_cache(maxsize=None)
def case(*key, model="full"):
    """vref.case(*key) with the scales, a block of values and the CDF there in both precisions beside it: "s64", "sld", "values", "F64",
    "Fld", "E" (chain_error). model = "diag": the case's covariances with everything off the diagonal struck out ("variances": K x d);
    "tied": every component with the first one's covariance ("tied": d x d); the rows stay the full model's. Computed once and shared;
    the arrays are not to be changed."""
    c = dict(vref.case(*key))
    if model != "full":
        covs = c["covs"]
        if model == "diag":
            c["variances"] = np.ascontiguousarray(np.diagonal(covs, axis1=1, axis2=2))
            c["covs"] = np.stack([np.diag(v) for v in c["variances"]])
        else:
            c["tied"] = np.ascontiguousarray(covs[0])
            c["covs"] = np.stack([covs[0]] * len(covs))
        c["f64"] = cref.conditional_mean(c["mixing"], c["means"], c["covs"], c["observed"], c["X_observed"])
        c["ld"] = cref.conditional_mean(c["mixing"], c["means"], c["covs"], c["observed"], c["X_observed"], LD)
        c["C64"] = vref.covariances(c["covs"], c["observed"])
        c["Cld"] = vref.covariances(c["covs"], c["observed"], LD)
    c["s64"], c["sld"] = scales(c["C64"]), scales(c["Cld"])
    c["values"] = make_values(c, 1000 + key[0])
    c["F64"] = cdf(c["f64"]["r"], c["f64"]["m"], c["s64"], c["values"])
    c["Fld"] = cdf(c["ld"]["r"], c["ld"]["m"], c["sld"], c["values"])
    c["E"] = chain_error(c)
    return c


def error(F, F_ld):
    """max |F - F_ld| / max |F_ld|."""
    return cref.error(F, F_ld)


def cdf_limit(c, values, r_estep, floor, F_ld=None, F_64=None):
    """The module docstring's CDF limit at `values` (N x dM) -> (limit, err_f64), relative to max |F_ld|."""
    r, m, s = c["ld"]["r"], c["ld"]["m"], c["sld"]
    v = np.asarray(values, dtype=LD)
    if F_ld is None:
        F_ld = cdf(r, m, s, v)
    if F_64 is None:
        F_64 = cdf(c["f64"]["r"], c["f64"]["m"], c["s64"], np.asarray(values, dtype=np.float64))
    scale = np.abs(F_ld).max()
    err_f64 = error(F_64, F_ld)
    a = (v[:, None, :] - m) / s[None]
    dr = np.abs(np.asarray(r_estep, dtype=LD) - r)
    moved_r = (dr[:, :, None] * ncdf_ld(a)).sum(axis=1).max()
    moved_t = (r[:, :, None] * npdf(a) / s[None] * c["E"]).sum(axis=1).max()
    return 4 * max(err_f64, floor) + float((moved_r + moved_t) / scale), err_f64


def displacement(c):
    """h_ij of the module docstring -> N x dM (longdouble)."""
    return c["E"].max(axis=1)


def certificate(c, v, p, r_estep, floor):
    """The module docstring's certificate for the device's quantiles v (N x dM) at probability p -> (ok: N x dM bool, worst: the largest
    of the two violations before the limit is granted, in units of the limit)."""
    r, m, s = c["ld"]["r"], c["ld"]["m"], c["sld"]
    v = np.asarray(v, dtype=LD)
    h = displacement(c)
    S = r.sum(axis=1)[:, None]
    T = LD(p) * S
    lim, _ = cdf_limit(c, v, r_estep, floor)
    lim = LD(lim) * np.abs(cdf(r, m, s, v)).max()
    low, high = cdf(r, m, s, v - h), cdf(r, m, s, v + h)
    ok = (low - lim <= T) & (T <= high + lim)
    worst = np.maximum(low - T, T - high) / lim
    return ok, float(worst.max())
