"""numpy restatement of the conditional mean's definition (include/mlhip.h, mlhip_em_condition / mlhip_em_conditional_means): the
conditioned model with a Cholesky factorisation and substitutions of its own, the marginal log-weights, the responsibilities and
E[x_M | x_O], in float64 and in np.longdouble, and the limit a device result is held to against the longdouble form. A helper, not a
test, and it imports nothing from the code under test: tests/test_condition_host.py checks the host conditioning against it on the
CPU, tests/test_gpu_condition.py the kernels."""
import functools

import numpy as np

LD = np.longdouble


def model(seed, d, K):
    """(mixing, means K x d, covariances K x d x d): mu_k = 2.5 N(0, I), Sigma_k = A A^T / d + 0.5 I with a Gaussian A, pi ~ Dirichlet(4)."""
    rng = np.random.default_rng(seed)
    means = 2.5 * rng.standard_normal((K, d))
    covs = np.empty((K, d, d))
    for k in range(K):
        A = rng.standard_normal((d, d))
        S = A @ A.T / d + 0.5 * np.eye(d)
        covs[k] = 0.5 * (S + S.T)
    mixing = rng.dirichlet(np.full(K, 4.0))
    return mixing, means, covs


def rows(mixing, means, covs, n, seed):
    """n rows drawn from the model with numpy.random.default_rng(seed), C-contiguous float64."""
    rng = np.random.default_rng(seed)
    K, d = means.shape
    labels = rng.choice(K, size=n, p=mixing)
    L = np.linalg.cholesky(covs)
    z = rng.standard_normal((n, d))
    return np.ascontiguousarray(means[labels] + np.einsum("nij,nj->ni", L[labels], z))


def missing_of(d, observed):
    taken = set(int(c) for c in observed)
    return [j for j in range(d) if j not in taken]


def cholesky(S):
    """Lower factor of S in S's own dtype, left-looking, one column at a time."""
    d = S.shape[0]
    L = np.zeros_like(S)
    for j in range(d):
        s = S[j, j] - np.dot(L[j, :j], L[j, :j])
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, d):
            L[i, j] = (S[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    return L


def forward(L, B):
    """Y with L Y = B (B: d x m), row by row."""
    Y = np.zeros_like(B)
    for i in range(L.shape[0]):
        Y[i] = (B[i] - L[i, :i] @ Y[:i]) / L[i, i]
    return Y


def backward(L, Y):
    """X with L^T X = Y."""
    d = L.shape[0]
    X = np.zeros_like(Y)
    for i in range(d - 1, -1, -1):
        X[i] = (Y[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


def condition(means, covs, observed, dtype=np.float64):
    """(means_observed K x dO, covariances_observed K x dO x dO, maps K x dM x dO, means_missing K x dM, factors K x dO x dO) in `dtype`:
    A_k = (L^-T (L^-1 Sigma_k,OM))^T with L L^T = Sigma_k,OO."""
    means, covs = np.asarray(means, dtype=dtype), np.asarray(covs, dtype=dtype)
    K, d = means.shape
    O, M = [int(c) for c in observed], missing_of(d, observed)
    mu_o, mu_m = means[:, O], means[:, M]
    S_oo = covs[:, O][:, :, O]
    maps = np.empty((K, len(M), len(O)), dtype=dtype)
    factors = np.empty((K, len(O), len(O)), dtype=dtype)
    for k in range(K):
        L = cholesky(S_oo[k])
        factors[k] = L
        maps[k] = backward(L, forward(L, covs[k][O][:, M])).T
    return mu_o, S_oo, maps, mu_m, factors


def conditional_mean(mixing, means, covs, observed, X_observed, dtype=np.float64):
    """The definition in `dtype` -> dict: y (N x dM), log_density (N), r (N x K responsibilities), m (N x K x dM component predictions)."""
    mixing = np.asarray(mixing, dtype=dtype)
    X = np.asarray(X_observed, dtype=dtype)
    mu_o, _, maps, mu_m, factors = condition(means, covs, observed, dtype)
    K, dO = mu_o.shape
    n = X.shape[0]
    lw = np.empty((n, K), dtype=dtype)
    m = np.empty((n, K, mu_m.shape[1]), dtype=dtype)
    for k in range(K):
        z = X - mu_o[k]
        w = forward(factors[k], np.ascontiguousarray(z.T))
        lw[:, k] = np.log(mixing[k]) - np.log(np.diag(factors[k])).sum() - (w * w).sum(axis=0) / dtype(2)
        m[:, k] = mu_m[k] + z @ maps[k].T
    top = lw.max(axis=1)
    lse = top + np.log(np.exp(lw - top[:, None]).sum(axis=1))
    r = np.exp(lw - lse[:, None])
    y = (r[:, :, None] * m).sum(axis=1)
    two_pi = dtype(8) * np.arctan(dtype(1))
    return {"y": y, "log_density": lse - dtype(dO) * np.log(two_pi) / dtype(2), "r": r, "m": m}


@functools.lru_cache(maxsize=None)
def case(seed, d, K, observed, n, row_seed=None):
    """One test case, computed once and shared: the model of `seed`, n rows drawn with `row_seed` (default seed + 1), both restatements.
    `observed`: a tuple. The arrays are not to be changed."""
    mixing, means, covs = model(seed, d, K)
    X = rows(mixing, means, covs, n, seed + 1 if row_seed is None else row_seed)
    X_o = np.ascontiguousarray(X[:, list(observed)])
    f64 = conditional_mean(mixing, means, covs, observed, X_o)
    ld = conditional_mean(mixing, means, covs, observed, X_o, LD)
    return {"mixing": mixing, "means": means, "covs": covs, "X": X, "X_observed": X_o, "observed": list(observed), "f64": f64, "ld": ld}


def error(y, y_ld):
    """max |y - y_ld| / max |y_ld|."""
    y_ld = np.asarray(y_ld, dtype=LD)
    return float(np.abs(np.asarray(y, dtype=LD) - y_ld).max() / np.abs(y_ld).max())


def limit(err_f64, floor, r_estep, ld):
    """4 max(err_f64, floor) + max_i sum_k |r_ik^E - r_ik^ld| |m_ik^ld| / max |y_ld| (the largest over the missing coordinates): the
    float64 restatement's own error, and what the E-step kernels' error in the responsibilities -- theirs, not the new kernel's -- moves
    the result by."""
    dr = np.abs(np.asarray(r_estep, dtype=LD) - ld["r"])
    moved = (dr[:, :, None] * np.abs(ld["m"])).sum(axis=1).max()
    return 4 * max(err_f64, floor) + float(moved / np.abs(ld["y"]).max())
