"""Extended-precision reference of the operations the kernels and the CPU oracle compute (test infrastructure; numpy only).

Everything runs in numpy.longdouble with a 64-bit significand (x87 extended: eps = 2^-63, eleven more bits than fp64), written
the plain way -- log-domain densities, log-sum-exp about the maximum, two-pass statistics -- and NOT in anyone's operation order:
a kernel or the oracle is judged by its distance from these values (tests/test_hp_reference.py pins them against 50-digit
arithmetic). numpy.linalg does not take long double, so the Cholesky factorization and the triangular solve are explicit
loops over the dimension, vectorised over the other axis. Inputs are taken as the fp64 numbers they are (exactly
representable in long double); outputs are long double, cast by the caller.

Parameter conventions as in ml_amd/_lib.py: data N x d, means K x d, covariances K x d x d, variances K x d, mixing K."""
import numpy as np

LD = np.longdouble
if np.finfo(LD).nmant < 63:
    raise ImportError(f"numpy.longdouble has a {np.finfo(LD).nmant + 1}-bit significand here; the reference needs at least 64 "
                      "(x87 extended precision)")

EPS64 = 2.0 ** -53          # unit roundoff of fp64
_LOG_2PI = np.log(2 * np.arccos(LD(-1)))


def _ld(a):
    return np.ascontiguousarray(a, dtype=LD)


def cholesky(A):
    """Lower factor L of a symmetric positive definite matrix, L L^T = A (column by column)."""
    A = _ld(A)
    d = A.shape[0]
    L = np.zeros((d, d), LD)
    for j in range(d):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:
            raise ValueError("matrix is not positive definite")
        L[j:, j] = v / np.sqrt(v[0])
    return L


def solve_lower(L, B):
    """Y with L Y = B for lower triangular L (d x d) and B (d x m): row by row, all m columns at once."""
    B = _ld(B)
    Y = np.zeros_like(B)
    for i in range(L.shape[0]):
        Y[i] = (B[i] - L[i, :i] @ Y[:i]) / L[i, i]
    return Y


def _normalise(lw):
    """Responsibilities and per-sample log-sum-exp of a K x N block of log weights (rows of -inf allowed)."""
    m = lw.max(axis=0)
    with np.errstate(invalid="ignore"):
        e = np.exp(lw - m)
    lse = m + np.log(e.sum(axis=0))
    return e / e.sum(axis=0), lse


def _close(X, resp, diagonal):
    """Two-pass M-step: the means first, then the second moments about them. A component whose responsibilities are all exactly 0
    has no mean and no second moments: 0 / 0 = NaN in every entry, silently."""
    n = X.shape[0]
    s0 = resp.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        means = (resp @ X) / s0[:, None]
        K, d = means.shape
        second = np.empty((K, d) if diagonal else (K, d, d), LD)
        for k in range(K):
            c = X - means[k]
            second[k] = (resp[k][:, None] * c * c).sum(axis=0) / s0[k] if diagonal else (c.T * resp[k]) @ c / s0[k]
    return s0 / n, means, second


def log_weights(X, mixing, means, covs):
    """K x N block log(pi_k N(x_i; mu_k, Sigma_k)), full covariances."""
    X, mixing, means = _ld(X), _ld(mixing), _ld(means)
    n, d = X.shape
    lw = np.empty((len(mixing), n), LD)
    with np.errstate(divide="ignore"):
        log_pi = np.log(mixing)
    for k in range(len(mixing)):
        L = cholesky(covs[k])
        y = solve_lower(L, (X - means[k]).T)
        lw[k] = log_pi[k] - np.log(np.diag(L)).sum() - (y * y).sum(axis=0) / 2 - d * _LOG_2PI / 2
    return lw


def log_weights_diag(X, mixing, means, variances):
    X, mixing, means, variances = _ld(X), _ld(mixing), _ld(means), _ld(variances)
    n, d = X.shape
    lw = np.empty((len(mixing), n), LD)
    with np.errstate(divide="ignore"):
        log_pi = np.log(mixing)
    for k in range(len(mixing)):
        c = X - means[k]
        lw[k] = log_pi[k] - np.log(variances[k]).sum() / 2 - (c * c / variances[k]).sum(axis=1) / 2 - d * _LOG_2PI / 2
    return lw


def m_step(X, resp, diagonal=False):
    """(mixing, means, covariances or variances) from an N x K block of responsibilities; no ridge on the diagonal."""
    return _close(_ld(X), _ld(np.asarray(resp).T), diagonal)


def em_step(X, mixing, means, covs):
    """One E + M step. Returns (mean log-likelihood, responsibilities N x K, mixing, means, covariances). The covariances carry
    no + 1e-15 I (callers add it); mixing weights of 0 are allowed."""
    resp, lse = _normalise(log_weights(X, mixing, means, covs))
    return (lse.sum() / len(lse), resp.T) + _close(_ld(X), resp, False)


def em_step_diag(X, mixing, means, variances):
    """One E + M step with diagonal covariances. Returns (mean log-likelihood, responsibilities, mixing, means, variances)."""
    resp, lse = _normalise(log_weights_diag(X, mixing, means, variances))
    return (lse.sum() / len(lse), resp.T) + _close(_ld(X), resp, True)


def em_step_tied(X, mixing, means, cov, weights=None):
    """One E + M step with ONE covariance shared by all components (the tied mode). Returns (mean
    log-likelihood, responsibilities N x K, mixing, means, covariance d x d). Densities from one Cholesky factor of `cov`; the new
    covariance in its two-pass form  sum_k sum_i w_i r_ik (x_i - mu_k)(x_i - mu_k)^T / W  about the NEW means, W = sum_i w_i (row
    weights `weights`, all 1 when None; the log-likelihood is the weighted mean). No ridge; mixing weights of 0 are allowed. A
    component whose weighted responsibilities are all exactly 0 has no mean (0 / 0 = NaN) and adds nothing to the covariance: its
    term is a sum of exact zeros and is left out, as the limit is."""
    X, mixing, means = _ld(X), _ld(mixing), _ld(means)
    n, d = X.shape
    K = len(mixing)
    L = cholesky(cov)
    half_log_det = np.log(np.diag(L)).sum()
    with np.errstate(divide="ignore"):
        log_pi = np.log(mixing)
    Xt = np.ascontiguousarray(X.T)                   # d x N: rows contiguous over the samples
    lw = np.empty((K, n), LD)
    for k in range(K):
        y = solve_lower(L, Xt - means[k][:, None])
        lw[k] = log_pi[k] - half_log_det - (y * y).sum(axis=0) / 2 - d * _LOG_2PI / 2
    resp, lse = _normalise(lw)
    w = np.ones(n, LD) if weights is None else _ld(weights)
    total = w.sum()
    wr = resp * w
    s0 = wr.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        new_means = (wr @ X) / s0[:, None]
    second = np.zeros((d, d), LD)
    for k in np.nonzero(s0 > 0)[0]:
        c = Xt - new_means[k][:, None]
        second += np.einsum("an,bn->ab", c * wr[k], c)
    return (w * lse).sum() / total, resp.T, s0 / total, new_means, second / total


def squared_distances(X, centroids):
    """N x K block |x_i - c_k|^2."""
    X, centroids = _ld(X), _ld(centroids)
    out = np.empty((X.shape[0], centroids.shape[0]), LD)
    for k in range(centroids.shape[0]):
        c = X - centroids[k]
        out[:, k] = (c * c).sum(axis=1)
    return out


def min_squared_distances(X, centroids):
    return squared_distances(X, centroids).min(axis=1)


def kmeans_step(X, centroids):
    """Assignment + update. Returns (nearest squared distance N, label N (lowest index on a tie), runner-up margin N = second
    smallest distance - smallest (inf for K = 1), inertia, counts K, new centroids K x d (an empty cluster's is the origin))."""
    X = _ld(X)
    D2 = squared_distances(X, centroids)
    n, K = D2.shape
    label = D2.argmin(axis=1)
    dist = D2[np.arange(n), label]
    if K > 1:
        D2[np.arange(n), label] = np.inf
        margin = D2.min(axis=1) - dist
    else:
        margin = np.full(n, np.inf, LD)
    counts = np.bincount(label, minlength=K)
    new = np.zeros((K, X.shape[1]), LD)
    for k in np.nonzero(counts)[0]:
        new[k] = X[label == k].sum(axis=0) / counts[k]
    return dist, label, margin, dist.sum(), counts, new


def sample_covariance(X):
    """(mean, covariance with the 1 / (N - 1) factor), two passes."""
    X = _ld(X)
    mean = X.sum(axis=0) / X.shape[0]
    c = X - mean
    return mean, c.T @ c / (X.shape[0] - 1)


def xxt_xy(X, y):
    """The contractions sum_i x_i x_i^T (q x q) and sum_i x_i y_i (q) of an N x q block."""
    X, y = _ld(X), _ld(y)
    return X.T @ X, X.T @ y


def conditioning(shift, means, covs=None, variances=None):
    """The quantities the kernels' error models are stated in, per component, as fp64 arrays in a dict:

    ratio   max_j (mu_kj - shift_j)^2 / Sigma_k,jj   -- the cancellation of the shared-shift second moments (give the NEW
            means and covariances); the library refines a component above MLHIP_REFINE_RATIO = 1e4
    fold    max_j |W_k (mu_k - shift)|_j, W_k = L_k^-1  -- the E-step's FOLD form runs while every entry stays <= 64 (give the
            parameters the E-step is called with); full covariances only
    b2      sum_j (mu_kj - shift_j)^2 / var_kj   -- the diagonal mode's shift-centred forms (guards 64^2 and 1024)
    kappa   |L_k|_inf |L_k^-1|_inf (max(sigma) / min(sigma) for variances): how much the density's triangular solve amplifies a
            rounding error of its input

    `shift` is the statistics' shift, the data mean (Data.shift)."""
    shift, means = _ld(shift), _ld(means)
    K, d = means.shape
    off = means - shift
    out = {}
    if covs is not None:
        ratio, fold, kappa = np.empty(K), np.empty(K), np.empty(K)
        for k in range(K):
            S = _ld(covs[k])
            L = cholesky(S)
            W = solve_lower(L, np.eye(d, dtype=LD))
            ratio[k] = float((off[k] ** 2 / np.diag(S)).max())
            fold[k] = float(np.abs(W @ off[k]).max())
            kappa[k] = float(np.abs(L).sum(axis=1).max() * np.abs(W).sum(axis=1).max())
        out.update(ratio=ratio, fold=fold, kappa=kappa)
        variances = np.stack([np.diag(_ld(covs[k])) for k in range(K)])
    else:
        v = _ld(variances)
        out.update(ratio=(off ** 2 / v).max(axis=1).astype(np.float64),
                   kappa=np.sqrt(v.max(axis=1) / v.min(axis=1)).astype(np.float64))
    out["b2"] = (off ** 2 / _ld(variances)).sum(axis=1).astype(np.float64)
    return out


def tied_conditioning(X, shift, means, cov_old, cov_new, resp=None):
    """The quantities the tied kernel's error models are stated in, as floats in a dict. `means` and
    `cov_old` are the parameters the E-step is called with, `cov_new` the step's result, `shift` the statistics' shift (the data
    mean, Data.shift); with L L^T = cov_old, x~ = x - shift, y_i = L^-1 x~_i, m_k = L^-1 (mu_k - shift), z_ik = y_i - m_k:

    tratio  max_j (T / N)_jj / cov_new_jj, T = sum_i x~_i x~_i^T   -- the cancellation of Sigma = T / N - sum_k pi_k mu~_k mu~_k^T
    reach   max_k max_j |m_kj|                                      -- how far the whitening reaches from the shift
    whiten  max over the pairs with r_ik >= 1e-6 of  sum_j |z_ikj| (|y_ij| + |m_kj|)   -- the first-order coefficient of the
            whitening model (each y_j, m_kj carries an absolute error ~ 2^-53 of its size) in a log-responsibility;
            `resp`: the step's N x K responsibilities (only this entry needs them; left out when None)."""
    X, shift, means = _ld(X), _ld(shift), _ld(means)
    Xt = X - shift
    T = (Xt * Xt).sum(axis=0) / X.shape[0]
    L = cholesky(cov_old)
    Y = solve_lower(L, Xt.T).T                       # N x d
    M = solve_lower(L, (means - shift).T).T          # K x d
    out = {"tratio": float((T / np.diag(_ld(cov_new))).max()), "reach": float(np.abs(M).max())}
    if resp is not None:
        resp = np.asarray(resp, dtype=np.float64)
        worst = 0.0
        for k in range(means.shape[0]):
            rows = resp[:, k] >= 1e-6
            if rows.any():
                y = Y[rows]
                worst = max(worst, float((np.abs(y - M[k]) * (np.abs(y) + np.abs(M[k]))).sum(axis=1).max()))
        out["whiten"] = worst
    return out


def rel_err(got, ref):
    """Max-norm relative error max |got - ref| / max |ref| (DESIGN.md section 4's norm), in long double, as a float."""
    ref = _ld(ref)
    scale = np.abs(ref).max()
    return float(np.abs(_ld(got) - ref).max() / scale) if scale > 0 else float(np.abs(_ld(got)).max())


def abs_err(got, ref):
    return float(np.abs(_ld(got) - _ld(ref)).max())


def over_limit(got, ref, limit, absolute=False):
    """The comparison every error test makes: True when `got` is further than `limit` from `ref` in the max norm (relative to
    max |ref| unless `absolute`), or not finite where `ref` is."""
    got = np.asarray(got)
    if got.shape != np.shape(ref) or not np.all(np.isfinite(got.astype(np.float64)) == np.isfinite(np.asarray(ref, dtype=np.float64))):
        return True
    err = abs_err(got, ref) if absolute else rel_err(got, ref)
    return not err <= limit
