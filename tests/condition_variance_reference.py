"""numpy restatement of the conditional variance's definition (include/mlhip.h, mlhip_em_conditional_variances):
    Var[x_M | x_O] = sum_k r_k (C_k + (t_k - y)(t_k - y)^T)
in float64 and in np.longdouble, in both forms, and the limit a device result is held to against the longdouble form. The
responsibilities r, the component predictions t (named `m` there) and the mean y come from tests/condition_reference.py; the
conditioned covariances C_k = Sigma_k,MM - Y^T Y, L Y = Sigma_k,OM, L L^T = Sigma_k,OO are restated here. A helper, not a test, and it
imports nothing from the code under test.

The limit has the shape the mean's has (tests/hp_limits.py):
    err = max |v - v_ld| / max |v_ld|
    err <= 4 max(err_f64, FLOOR) + max_{i,a,b} sum_k |r^E_ik - r^ld_ik| |C^ld_k,ab + u^ld_ika u^ld_ikb| / max |v_ld|
err_f64 is the float64 restatement's own error; r^E are the responsibilities the existing E-step kernels give on the same handle --
the new kernel is not charged with their error. y's own error enters only at second order (sum_k r_k (t_k - y) = 0): no term."""
import functools

import numpy as np

import condition_reference as cref

LD = cref.LD


def covariances(covs, observed, dtype=np.float64):
    """C_k = Sigma_k,MM - Y^T Y with L Y = Sigma_k,OM and L L^T = Sigma_k,OO, in `dtype` -> K x dM x dM, symmetrised by copying the lower
    triangle."""
    covs = np.asarray(covs, dtype=dtype)
    K, d = covs.shape[0], covs.shape[1]
    O, M = [int(c) for c in observed], cref.missing_of(d, observed)
    out = np.empty((K, len(M), len(M)), dtype=dtype)
    for k in range(K):
        L = cref.cholesky(covs[k][O][:, O])
        Y = cref.forward(L, covs[k][O][:, M])
        C = covs[k][M][:, M] - Y.T @ Y
        out[k] = np.tril(C) + np.tril(C, -1).T
    return out


def variance(r, m, y, C):
    """The definition in the arrays' dtype -> dict: diag (N x dM), full (N x dM x dM), between (N x dM: sum_k r_k u_k^2, the part of the
    diagonal that comes from the spread of the component predictions), u (N x K x dM)."""
    u = m - y[:, None, :]
    dM = y.shape[1]
    Cd = C[:, np.arange(dM), np.arange(dM)]
    between = (r[:, :, None] * u * u).sum(axis=1)
    diag = (r[:, :, None] * (Cd[None] + u * u)).sum(axis=1)
    full = np.zeros((len(y), dM, dM), dtype=y.dtype)
    for k in range(r.shape[1]):                                  # (one component at a time: N x dM x dM is the largest array held)
        full += r[:, k, None, None] * (C[k][None] + u[:, k, :, None] * u[:, k, None, :])
    return {"diag": diag, "full": full, "between": between, "u": u}


@functools.lru_cache(maxsize=None)
def case(*key):
    """cref.case(*key) with the variance in both precisions beside it: keys "v64" and "vld" (variance()'s dicts), "C64" and "Cld". Computed
    once and shared; the arrays are not to be changed."""
    c = dict(cref.case(*key))
    c["C64"] = covariances(c["covs"], c["observed"])
    c["Cld"] = covariances(c["covs"], c["observed"], LD)
    c["v64"] = variance(c["f64"]["r"], c["f64"]["m"], c["f64"]["y"], c["C64"])
    c["vld"] = variance(c["ld"]["r"], c["ld"]["m"], c["ld"]["y"], c["Cld"])
    return c


def error(v, v_ld):
    """max |v - v_ld| / max |v_ld|."""
    return cref.error(v, v_ld)


def limit(err_f64, floor, r_estep, c, form):
    """The module docstring's limit for `form` ("diag" | "full") of case c."""
    dr = np.abs(np.asarray(r_estep, dtype=LD) - c["ld"]["r"])
    u, C = c["vld"]["u"], c["Cld"]
    dM = u.shape[2]
    if form == "diag":
        terms = np.abs(C[:, np.arange(dM), np.arange(dM)][None] + u * u)
        moved = (dr[:, :, None] * terms).sum(axis=1).max()
    else:
        moved = np.zeros((len(dr), dM, dM), dtype=LD)
        for k in range(dr.shape[1]):
            moved += dr[:, k, None, None] * np.abs(C[k][None] + u[:, k, :, None] * u[:, k, None, :])
        moved = moved.max()
    return 4 * max(err_f64, floor) + float(moved / np.abs(c["vld"][form]).max())


def between_share(c):
    """The share of the LARGEST variance of the case (longdouble, diagonal form) that comes from the between-component term."""
    v = c["vld"]["diag"]
    at = np.unravel_index(np.argmax(v), v.shape)
    return float(c["vld"]["between"][at] / v[at])


def brute_force(r, m, y, C):
    """sum_k r_k (C_k + t_k t_k^T) - y y^T: the uncentred second moment less the mean's square, in the arrays' dtype (N x dM x dM)."""
    second = np.zeros((len(y), y.shape[1], y.shape[1]), dtype=y.dtype)
    for k in range(r.shape[1]):
        second += r[:, k, None, None] * (C[k][None] + m[:, k, :, None] * m[:, k, None, :])
    return second - y[:, :, None] * y[:, None, :]
