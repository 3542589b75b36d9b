"""numpy restatement of the conditional draw's definition (include/mlhip.h, mlhip_em_condition_covariances /
mlhip_em_conditional_samples) on top of tests/condition_reference.py (the conditioned model, the responsibilities) and
tests/sample_reference.py (Philox4x32-10, the uniform, Box-Muller): the covariances of the conditioned components and their factors,
the label rule, the normals on the draw's own generator stream and the row, in float64 and in np.longdouble, and the per-coordinate
tolerance a device result is held to against the longdouble form. A helper, not a test, and it imports nothing from the code under
test: tests/test_condition_sample_host.py checks it and the host helper on the CPU, tests/test_gpu_condition_sample.py the kernels."""
import functools

import numpy as np

import condition_reference as cref
import sample_reference as sref

LD = np.longdouble
EPS = sref.EPS
NO_LABEL = 0xFFFFFFFF
MARGIN = 2.0 ** -40                # rows with |u S - s_k| <= MARGIN S for a k with r_k > 0 are left out of a label comparison
STATISTICAL_BOUND = 5.0
# the statistical cases of the issue: (model seed, d, K, observed, n, row seed), and rows x draws
MOMENTS_CASE = (11, 6, 4, (4, 0, 1), 200000, 12)
DRAWS_CASE = (13, 6, 4, (4, 0, 1), 64, 14)
DRAWS = 4096


def row_words(seed, rows, block, stream):
    """Output words of row indices `rows` (uint64) for counter block `block` on generator stream `stream` (the fourth counter word:
    0 is mlhip_em_sample's, draw q of the conditional sampler is 1 + q)."""
    rows = np.asarray(rows, dtype=np.uint64)
    seed = int(seed)
    mask = np.uint64(sref.MASK)
    return sref.philox4x32_10((rows & mask, rows >> np.uint64(32), np.uint64(block), np.uint64(stream)), (seed & sref.MASK, seed >> 32))


def uniforms(seed, rows, q):
    """The label's uniform of every row for draw q."""
    w = row_words(seed, rows, 0, 1 + q)
    return sref.uniform(w[0], w[1])


def normals(seed, rows, dM, q, dtype=np.float64):
    """(zeta, rad): the dM normals of every row for draw q and the Box-Muller radius behind each of them, n x dM."""
    n = len(rows)
    z, r = np.empty((n, dM), dtype=dtype), np.empty((n, dM), dtype=dtype)
    two_pi = dtype(8) * np.arctan(dtype(1))
    for p in range((dM + 1) // 2):
        w = row_words(seed, rows, 1 + p, 1 + q)
        u1, u2 = sref.uniform(w[0], w[1], dtype), sref.uniform(w[2], w[3], dtype)
        rad = np.sqrt(dtype(-2) * np.log(u1))
        z[:, 2 * p] = rad * np.cos(two_pi * u2)
        r[:, 2 * p] = rad
        if 2 * p + 1 < dM:
            z[:, 2 * p + 1] = rad * np.sin(two_pi * u2)
            r[:, 2 * p + 1] = rad
    return z, r


def labels_of(r, u):
    """The label rule on float64 responsibilities r (n x K) and uniforms u (n) -> (labels uint32, margin): s_k the sequential prefix
    sums, S = s_{K-1}, label = the smallest k with u S < s_k, else the largest k with r_k != 0; NO_LABEL where S is a NaN. margin: per
    row min over the k with r_k > 0 of |u S - s_k| / S."""
    r = np.asarray(r, dtype=np.float64)
    n, K = r.shape
    s = np.empty_like(r)
    acc = np.zeros(n)
    for k in range(K):                                           # (sequential, ascending k: the order is part of the definition)
        acc = acc + r[:, k]
        s[:, k] = acc
    S = s[:, -1]
    target = np.asarray(u, dtype=np.float64) * S
    below = target[:, None] < s
    first = np.argmax(below, axis=1)
    share = r != 0
    last = K - 1 - np.argmax(share[:, ::-1], axis=1)
    labels = np.where(below.any(axis=1), first, last).astype(np.int64)
    labels[np.isnan(S) | ~share.any(axis=1)] = NO_LABEL
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = np.where(r > 0, np.abs(target[:, None] - s), np.inf).min(axis=1) / S
    return labels.astype(np.uint32), gap


def covariances(covs, observed, dtype=np.float64):
    """(C K x dM x dM, G K x dM x dM) in `dtype`: C_k = Sigma_k,MM - Y^T Y with L L^T = Sigma_k,OO, Y = L^-1 Sigma_k,OM, symmetrised as
    the definition builds it (the lower triangle, mirrored); G_k = the lower Cholesky factor of C_k."""
    covs = np.asarray(covs, dtype=dtype)
    K, d = covs.shape[0], covs.shape[1]
    O, M = [int(c) for c in observed], cref.missing_of(d, observed)
    C = np.empty((K, len(M), len(M)), dtype=dtype)
    G = np.empty_like(C)
    for k in range(K):
        L = cref.cholesky(covs[k][O][:, O])
        Y = cref.forward(L, covs[k][O][:, M])
        full = covs[k][M][:, M] - Y.T @ Y
        C[k] = np.tril(full) + np.tril(full, -1).T
        G[k] = cref.cholesky(C[k])
    return C, G


def rows_given(labels, X_observed, mu_o, maps, mu_m, factors, zeta, dtype=np.float64):
    """x~ = mu_k,M + A_k z + G_k zeta with k = labels, z = x_O - mu_k,O (a float64 subtraction, as the definition states it), in `dtype`;
    NaN where the label is NO_LABEL."""
    n, dM = zeta.shape
    out = np.full((n, dM), np.nan, dtype=dtype)
    for k in range(len(mu_m)):
        idx = np.nonzero(labels == k)[0]
        if not len(idx):
            continue
        z = (np.asarray(X_observed, dtype=np.float64)[idx] - np.asarray(mu_o[k], dtype=np.float64)).astype(dtype)
        out[idx] = (np.asarray(mu_m[k]).astype(dtype) + z @ np.asarray(maps[k]).astype(dtype).T
                    + np.asarray(zeta[idx], dtype=dtype) @ np.tril(np.asarray(factors[k])).astype(dtype).T)
    return out


def tolerance(labels, X_observed, mu_o, maps, mu_m, factors, zeta, rad):
    """|x~_j - ref_j| <= (dO + dM + 3) eps (|mu_M,j| + sum_c |A_jc| |z_c| + sum_c |G_jc| |zeta_c|) + 16 eps sum_c |G_jc| rad_c:
    sample_reference.tolerance with the dO terms of the map chain in front of the factor's (a chain of dO + dM + 1 fmas, the
    subtraction and the start), eps = 2^-52."""
    n, dM = zeta.shape
    dO = np.asarray(mu_o).shape[1]
    tol = np.full((n, dM), np.inf)
    for k in range(len(mu_m)):
        idx = np.nonzero(labels == k)[0]
        if not len(idx):
            continue
        z = np.abs(np.asarray(X_observed, dtype=np.float64)[idx] - mu_o[k])
        aG = np.abs(np.tril(factors[k]))
        chain = np.abs(mu_m[k])[None, :] + z @ np.abs(maps[k]).T + np.abs(np.asarray(zeta[idx], dtype=np.float64)) @ aG.T
        tol[idx] = (dO + dM + 3) * EPS * chain + 16 * EPS * (np.asarray(rad[idx], dtype=np.float64) @ aG.T)
    return tol


def sample(mixing, means, covs, observed, X_observed, n_draws=1, seed=0, first_row=0, first_draw=0, r=None):
    """The whole definition in float64 -> (X n_draws x n x dM, labels n_draws x n uint32, margins n_draws x n). `r`: responsibilities to
    draw the labels from (default: the float64 restatement's own)."""
    mu_o, _, maps, mu_m, _ = cref.condition(means, covs, observed)
    _, G = covariances(covs, observed)
    if r is None:
        r = cref.conditional_mean(mixing, means, covs, observed, X_observed)["r"]
    n = len(X_observed)
    rows = np.uint64(first_row) + np.arange(n, dtype=np.uint64)
    X = np.empty((n_draws, n, mu_m.shape[1]))
    labels = np.empty((n_draws, n), dtype=np.uint32)
    margins = np.empty((n_draws, n))
    for q in range(n_draws):
        labels[q], margins[q] = labels_of(r, uniforms(seed, rows, first_draw + q))
        zeta, _ = normals(seed, rows, mu_m.shape[1], first_draw + q)
        X[q] = rows_given(labels[q], X_observed, mu_o, maps, mu_m, G, zeta)
    return X, labels, margins


def moment_scores(X_observed, X_missing, X_drawn):
    """The largest deviation, in standard errors, of the first and second moments of (x_O, x~_M) from those of (x_O, x_M): per
    entry of the mean and of the second-moment matrix, |mean(a) - mean(b)| / (std(a - b) / sqrt(n)) over the rows -- the two samples
    share x_O, so the entries that involve only x_O agree exactly and are left out."""
    n = len(X_observed)
    A, B = np.hstack([X_observed, X_drawn]), np.hstack([X_observed, X_missing])
    dO = X_observed.shape[1]
    worst = 0.0
    for j in range(dO, A.shape[1]):
        diff = A[:, j] - B[:, j]
        worst = max(worst, abs(diff.mean()) / (diff.std(ddof=1) / np.sqrt(n)))
        for c in range(j + 1):
            diff = A[:, j] * A[:, c] - B[:, j] * B[:, c]
            worst = max(worst, abs(diff.mean()) / (diff.std(ddof=1) / np.sqrt(n)))
    return worst


def draw_mean_scores(X_draws, y):
    """The deviation of the mean over draws from the conditional mean y, in standard errors (the draws' own standard deviation over
    sqrt(draws)): draws x rows x dM against rows x dM -> the largest."""
    q = X_draws.shape[0]
    return float(np.max(np.abs(X_draws.mean(axis=0) - y) / (X_draws.std(axis=0, ddof=1) / np.sqrt(q))))


@functools.lru_cache(maxsize=None)
def case(seed, d, K, observed, n, row_seed=None):
    """condition_reference.case with the float64 and longdouble conditioned covariances and factors beside it; computed once, not to
    be changed."""
    c = dict(cref.case(seed, d, K, observed, n, row_seed))
    c["C"], c["G"] = covariances(c["covs"], observed)
    c["C_ld"], c["G_ld"] = covariances(c["covs"], observed, LD)
    return c
