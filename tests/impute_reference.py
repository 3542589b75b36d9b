"""numpy restatement of mlhip_em_impute's definition (include/mlhip.h), pattern by pattern, in float64 and in np.longdouble, built on
tests/condition_reference.py: the rows of a block with NaNs are grouped by their pattern of observed coordinates, every group is the
conditional mean of its pattern, the complete rows are the marginal mixture over all coordinates, the rows of all NaN the mixture's
mean. A helper, not a test; it imports nothing from the code under test."""
import functools
from fractions import Fraction

import numpy as np

import condition_reference as ref

LD = np.longdouble


def with_gaps(X, missing):
    """A copy of X with NaN where `missing` (a boolean array of X's shape) is set."""
    Y = np.array(X, dtype=np.float64, order="C")
    Y[np.asarray(missing, dtype=bool)] = np.nan
    return Y


def bernoulli_gaps(X, p, seed, complete=(), empty=()):
    """X with every entry missing with probability p, the rows `complete` left whole and the rows `empty` all NaN."""
    rng = np.random.default_rng(seed)
    missing = rng.random(X.shape) < p
    missing[list(complete)] = False
    missing[list(empty)] = True
    return with_gaps(X, missing)


def distinct_gaps(X):
    """X with a different pattern in every row: row i misses the coordinates of the set bits of i + 1 (N <= 2^d - 2, so no row is
    complete or empty)."""
    n, d = X.shape
    assert n <= 2 ** d - 2
    missing = np.array([[(i + 1) >> c & 1 for c in range(d)] for i in range(n)], dtype=bool)
    return with_gaps(X, missing)


def groups(X):
    """[(observed coordinates (a tuple, ascending), row indices (ascending))] of the patterns of X, in ascending order of the mask
    read as a number with bit c = coordinate c observed -- the library's plan order at d <= 64."""
    seen = {}
    for i, row in enumerate(np.isnan(X)):
        seen.setdefault(tuple(int(c) for c in np.nonzero(~row)[0]), []).append(i)
    return sorted(((o, np.array(r)) for o, r in seen.items()), key=lambda g: sum(1 << c for c in g[0]))


def fma(a, b, c):
    """fma(a, b, c) in float64, exactly rounded."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def prior_mean(mixing, means):
    """A row of all NaN: out_j = +0.0, then fma(pi_k, mu_k[j], out_j) for ascending k where pi_k != 0."""
    out = [0.0] * means.shape[1]
    for k, pi in enumerate(mixing):
        if pi != 0:
            out = [fma(pi, means[k, j], out[j]) for j in range(means.shape[1])]
    return np.array(out)


def impute(mixing, means, covs, X, dtype=np.float64):
    """The definition in `dtype` -> dict: out (N x d), log_density (N), r (N x K), and `groups`: per pattern with 1 <= dO <= d - 1 a
    triple (observed, rows, condition_reference.conditional_mean's dict for the group)."""
    mixing = np.asarray(mixing)
    n, d = X.shape
    K = len(mixing)
    out = np.array(X, dtype=dtype)
    dens, r, parts = np.zeros(n, dtype=dtype), np.zeros((n, K), dtype=dtype), []
    for observed, rows_of in groups(X):
        if not observed:
            out[rows_of] = np.asarray((np.asarray(mixing, dtype=dtype)[:, None] * np.asarray(means, dtype=dtype)).sum(axis=0))
            r[rows_of] = np.asarray(mixing, dtype=dtype)
            continue
        X_o = np.ascontiguousarray(X[rows_of][:, list(observed)])
        if len(observed) == d:
            # the marginal mixture over every coordinate: condition on all but the last and keep the first five steps
            res = full_density(mixing, means, covs, X_o, dtype)
            dens[rows_of], r[rows_of] = res["log_density"], res["r"]
            continue
        res = ref.conditional_mean(mixing, means, covs, observed, X_o, dtype)
        M = ref.missing_of(d, observed)
        for j, c in enumerate(M):
            out[rows_of, c] = res["y"][:, j]
        dens[rows_of], r[rows_of] = res["log_density"], res["r"]
        parts.append((observed, rows_of, res))
    return {"out": out, "log_density": dens, "r": r, "groups": parts}


def full_density(mixing, means, covs, X, dtype):
    """Steps 1 - 5 on complete rows in `dtype` -> dict: log_density (N), r (N x K)."""
    mixing = np.asarray(mixing, dtype=dtype)
    means, covs, X = np.asarray(means, dtype=dtype), np.asarray(covs, dtype=dtype), np.asarray(X, dtype=dtype)
    K, d = means.shape
    lw = np.empty((X.shape[0], K), dtype=dtype)
    for k in range(K):
        L = ref.cholesky(covs[k])
        w = ref.forward(L, np.ascontiguousarray((X - means[k]).T))
        lw[:, k] = np.log(mixing[k]) - np.log(np.diag(L)).sum() - (w * w).sum(axis=0) / dtype(2)
    top = lw.max(axis=1)
    lse = top + np.log(np.exp(lw - top[:, None]).sum(axis=1))
    two_pi = dtype(8) * np.arctan(dtype(1))
    return {"log_density": lse - dtype(d) * np.log(two_pi) / dtype(2), "r": np.exp(lw - lse[:, None])}


@functools.lru_cache(maxsize=None)
def case(seed, d, K, n, kind, covariance="full"):
    """One test case, computed once and shared: the model of condition_reference.model(seed, d, K) -- its diagonal (K x d variances)
    or its first matrix (tied) with `covariance` = 'diag' / 'tied' --, n rows drawn from the full model with seed + 1, the gaps of
    `kind`, and both restatements. `kind`: 'one' (one pattern: the odd coordinates missing), 'distinct' (every row its own),
    'bernoulli' (p = 0.3, row 0 -- and row 2 where there is one -- complete, row 1 all NaN where there is one), or a tuple of
    missing coordinates shared by all rows. The arrays are not to be changed."""
    mixing, means, covs = ref.model(seed, d, K)
    X = ref.rows(mixing, means, covs, n, seed + 1)
    if kind == "one":
        missing = np.zeros((n, d), dtype=bool)
        missing[:, 1::2] = True
        G = with_gaps(X, missing)
    elif kind == "distinct":
        G = distinct_gaps(X)
    elif kind == "bernoulli":
        G = bernoulli_gaps(X, 0.3, seed + 2, complete=[i for i in (0, 2) if i < n], empty=[1] if n > 1 else [])
    else:
        missing = np.zeros((n, d), dtype=bool)
        missing[:, list(kind)] = True
        G = with_gaps(X, missing)
    if covariance == "diag":
        given = np.ascontiguousarray(np.stack([np.diag(c) for c in covs]))
        covs = np.stack([np.diag(v) for v in given])
    elif covariance == "tied":
        given = np.ascontiguousarray(covs[0])
        covs = np.stack([given] * K)
    else:
        given = covs
    return {"mixing": mixing, "means": means, "covs": covs, "given": given, "covariance": covariance, "X": G,
            "f64": impute(mixing, means, covs, G), "ld": impute(mixing, means, covs, G, LD)}
