"""numpy restatement of the sampler's definition (include/mlhip.h, mlhip_em_sample): Philox4x32-10, the uniform, the label rule, the
Box-Muller normals and the triangular product, in float64 and in np.longdouble, and the per-coordinate tolerance a device result is
held to against the longdouble form. A helper, not a test: tests/test_sample_host.py checks it on the CPU, tests/test_gpu_sample.py
compares the kernels with it."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
EPS = 2.0 ** -52

# (n, d, K, seed): the cases whose statistics are checked on the restatement (CPU) and on the device's output (GPU)
STATISTICAL_CASES = [(4099, 2, 3, 1), (4099, 13, 5, 2), (4099, 32, 8, 3), (20000, 7, 40, 4), (4099, 65, 2, 5), (4099, 1, 1, 6)]
STATISTICAL_BOUND = 5.0


def philox4x32_10(counter, key):
    """counter: four arrays (or scalars) of 32-bit words, key: two. Returns the four output words as uint64 arrays < 2^32."""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & np.uint64(MASK) for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def row_words(seed, rows, block):
    """Output words of row indices `rows` (uint64) for one counter block."""
    rows = np.asarray(rows, dtype=np.uint64)
    seed = int(seed)
    return philox4x32_10((rows & np.uint64(MASK), rows >> np.uint64(32), np.uint64(block), np.uint64(0)), (seed & MASK, seed >> 32))


def uniform(lo, hi, dtype=np.float64):
    """U(lo, hi) = (((hi 2^32 + lo) >> 12) + 1/2) 2^-52: exact in float64 (and so in longdouble)."""
    v = ((hi << np.uint64(32)) | lo) >> np.uint64(12)
    return (v.astype(dtype) + dtype(0.5)) * dtype(2.0 ** -52)


def thresholds(mixing):
    """t_k = s_k / s_{K-1}, s the sequential float64 prefix sums."""
    s = np.empty(len(mixing))
    acc = 0.0
    for k, w in enumerate(np.asarray(mixing, dtype=np.float64)):
        acc = acc + float(w)
        s[k] = acc
    return s / s[-1]


def labels_of(mixing, seed, rows):
    w = row_words(seed, rows, 0)
    u = uniform(w[0], w[1])
    t = thresholds(mixing)
    return (u[:, None] >= t[None, :-1]).sum(axis=1).astype(np.uint32)


def normals(seed, rows, d, dtype=np.float64):
    """(z, r): the d normals of every row and the Box-Muller radius behind each of them, n x d."""
    n = len(rows)
    z, r = np.empty((n, d), dtype=dtype), np.empty((n, d), dtype=dtype)
    two_pi = dtype(8) * np.arctan(dtype(1))                      # (not np.pi: that is a float64)
    for p in range((d + 1) // 2):
        w = row_words(seed, rows, 1 + p)
        u1, u2 = uniform(w[0], w[1], dtype), uniform(w[2], w[3], dtype)
        rad = np.sqrt(dtype(-2) * np.log(u1))
        z[:, 2 * p] = rad * np.cos(two_pi * u2)
        r[:, 2 * p] = rad
        if 2 * p + 1 < d:
            z[:, 2 * p + 1] = rad * np.sin(two_pi * u2)
            r[:, 2 * p + 1] = rad
    return z, r


def sample(mixing, means, factors, n, seed=0, first_row=0, dtype=np.float64, with_tolerance=False):
    """Rows [first_row, first_row + n): (X, labels) -- and, with_tolerance, the per-coordinate bound of tolerance(). means: K x d,
    factors: K x d x d lower Cholesky factors (row j, column c)."""
    means, factors = np.asarray(means, dtype=np.float64), np.asarray(factors, dtype=np.float64)
    K, d = means.shape
    rows = np.uint64(first_row) + np.arange(n, dtype=np.uint64)
    labels = labels_of(mixing, seed, rows)
    z, r = normals(seed, rows, d, dtype)
    X = np.empty((n, d), dtype=dtype)
    tol = np.empty((n, d)) if with_tolerance else None
    for k in range(K):
        idx = np.nonzero(labels == k)[0]
        if not len(idx):
            continue
        L = np.tril(factors[k]).astype(dtype)
        X[idx] = means[k].astype(dtype)[None, :] + z[idx] @ L.T
        if with_tolerance:
            tol[idx] = tolerance(means[k], np.tril(factors[k]), z[idx], r[idx])
    return (X, labels, tol) if with_tolerance else (X, labels)


def tolerance(mean, L, z, r):
    """|x_j - ref_j| <= (d+2) eps (|mu_j| + sum_c |L_jc| |z_c|) + 16 eps sum_c |L_jc| r_c: the bound of a (d+1)-term fma chain, and an
    absolute error of 16 eps r for each normal (log 1 ulp, sqrt 1 ulp, sin / cos 2 ulp and the rounding of the angle, about doubled;
    relative to r, not |z|, because near a zero of the cosine only the absolute error is bounded)."""
    d = len(mean)
    aL = np.abs(L)
    chain = np.abs(mean)[None, :] + np.abs(np.asarray(z, dtype=np.float64)) @ aL.T
    return (d + 2) * EPS * chain + 16 * EPS * (np.asarray(r, dtype=np.float64) @ aL.T)


def parameters(d, K):
    """The mixtures of the checks: rng = default_rng(100 d + K); mu = 6 N(0, 1), Sigma_k = A A^T / d + I / 2, pi ~ U(0.5, 1.5) normalised."""
    rng = np.random.default_rng(100 * d + K)
    means = 6.0 * rng.standard_normal((K, d))
    covs = np.empty((K, d, d))
    for k in range(K):
        A = rng.standard_normal((d, d))
        covs[k] = A @ A.T / d + 0.5 * np.eye(d)
        covs[k] = 0.5 * (covs[k] + covs[k].T)
    mixing = rng.uniform(0.5, 1.5, K)
    return mixing / mixing.sum(), means, covs


def statistics(X, labels, mixing, means, factors):
    """The three statistical conditions of a draw: the largest z-score of a component count, sqrt(n) max |mean of the whitened
    residuals| and sqrt(n) max |Y^T Y / n - I|, Y = L_k^-1 (x - mu_k) row by row."""
    n, d = X.shape
    mixing = np.asarray(mixing, dtype=np.float64) / np.sum(mixing)
    Y = np.empty((n, d))
    count_z = 0.0
    for k in range(len(mixing)):
        idx = np.nonzero(labels == k)[0]
        var = n * mixing[k] * (1 - mixing[k])
        if var > 0:
            count_z = max(count_z, abs(len(idx) - n * mixing[k]) / np.sqrt(var))
        else:
            assert len(idx) == (n if mixing[k] == 1 else 0)
        if len(idx):
            Y[idx] = np.linalg.solve(np.tril(factors[k]), (np.asarray(X[idx], dtype=np.float64) - means[k]).T).T
    mean_dev = np.sqrt(n) * np.max(np.abs(Y.mean(axis=0)))
    cov_dev = np.sqrt(n) * np.max(np.abs(Y.T @ Y / n - np.eye(d)))
    return count_z, mean_dev, cov_dev
