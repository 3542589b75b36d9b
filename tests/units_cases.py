"""Power-of-two changes of units, shared by tests/test_units_cases.py (CPU) and tests/test_gpu_units.py (GPU); numpy only, no HIP.

Multiplying column j of the data by f_j = 2^(s_j) commutes with every fp64 operation the kernels perform (add, multiply, fma, divide,
sqrt, the fp64 matrix instruction, the fixed-point limbs whose grid follows frexp of the column maximum) until something leaves the
normal range or the code holds a constant that is absolute in the data's units. So a route's outputs on the rescaled problem, divided by
their powers of two again, must have the BITS of the unit-scale run -- no tolerance -- wherever no logarithm is involved.

The scalings (SCALINGS; `exponents`):

    U-300, U+300   uniform 2^-300 / 2^+300: squares are 2^-+600, d-fold sums of squares and N-fold sums of those stay normal
    M16            mixed, s_j seeded integers in [0, 16] (both ends present): ratios of the diagonal of W = L^-1 stay under 1e5 (device/em_screen_bound.hpp)
    M60            mixed, s_j seeded integers in [-60, 60] (both ends present)

The transforms: X f, mu f, Sigma -> diag(f) Sigma diag(f), variances f^2, centroids f; row weights and responsibilities unchanged; the
handle's covariance ridge (absolute, in squared data units) becomes ridge 2^(2 s) under a uniform scaling and 0 under a mixed one (`ridge`;
the unit-scale run a mixed scaling is compared with has ridge 0 as well).

The one thing that cannot be covariant is the density's log-constant coef_k = log pi_k - sum_j log L_jj (- d log(2 pi) / 2): under the
scaling it moves by sum_j ln f_j, a rounded number. It is formed with at most 2 d + 2 roundings -- d logarithms, d additions, log pi, its
addition -- plus two for the constant, each at most 2^-53 of the largest partial sum c = max_k |coef'_k| + |sum_j ln f_j| + max |lw'|
(primes: the scaled problem). `allowance` is

    U = 4 (2 d + 4) 2^-53 c,    absolute in a log-weight.

Per-row log-densities move by at most U, responsibilities by at most 2 U (two log-weights), the mean log-likelihood by at most U, and a
label can differ only on a row whose two largest unit-scale log-weights are within 2 U of each other.

Measured on the CPU (tests/test_units_cases.py asserts it and `python tests/test_units_cases.py` prints it): over EM_CASES x SCALINGS the
largest deviation of the whitening restatement's log-weights from their unit-scale values minus sum_j ln f_j stays below U / 51 (the
smallest ratio U / deviation: 51.7, at d = 2, K = 3 under M16; 64 to 4775 elsewhere) -- U covers the restatement with far more than the
factor of 4 asked for. No row of any case lies within 2 U of a tie, so the label checks leave out no row. These figures come from the CPU
restatement alone, never from a kernel."""
import math

import numpy as np

from oracle import hp_cases

SCALINGS = ("U-300", "U+300", "M16", "M60")
UNIFORM = ("U-300", "U+300")
DEFAULT_RIDGE = 1e-15


def exponents(name, d):
    """The integer exponents s_j of scaling `name` for d columns."""
    if name == "U-300":
        return np.full(d, -300, dtype=np.int64)
    if name == "U+300":
        return np.full(d, 300, dtype=np.int64)
    if name in ("M16", "M60"):
        lo, hi, seed = (0, 16, 1600) if name == "M16" else (-60, 60, 6000)
        s = np.random.default_rng(seed + d).integers(lo, hi + 1, d)
        if d >= 2:
            s[0], s[-1] = lo, hi                         # the whole span is there at every d: column maxima 2^16 / 2^120 apart
        return s
    raise ValueError(name)


def factors(name, d):
    """f_j = 2^(s_j), exact."""
    return np.ldexp(1.0, exponents(name, d).astype(np.int32))


def sum_ln_f(name, d):
    """sum_j ln f_j = ln 2 * sum_j s_j (the integer sum is exact; one rounding)."""
    return math.log(2.0) * int(exponents(name, d).sum())


def ridge(name, base=DEFAULT_RIDGE):
    """The handle's ridge under scaling `name`; 0 for a mixed one (a scalar ridge has no mixed-unit form)."""
    return base * 4.0 ** int(exponents(name, 1)[0]) if name in UNIFORM else 0.0


def unit_ridge(name, base=DEFAULT_RIDGE):
    """The ridge of the unit-scale run that scaling `name` is compared with."""
    return base if name in UNIFORM else 0.0


def points(A, f):
    """Rows of coordinates (data, means, centroids): A f."""
    return np.ascontiguousarray(np.asarray(A, dtype=np.float64) * f)


def covariances(S, f):
    """(..., d, d) covariances: diag(f) S diag(f)."""
    return np.ascontiguousarray(np.asarray(S, dtype=np.float64) * f[:, None] * f[None, :])


def variances(v, f):
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64) * f * f)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).tobytes()


def same_bits(a, b):
    """tobytes() equality of two float64 arrays (distinguishes -0.0 from 0.0, and NaN payloads)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bits(a) == bits(b)


def allowance(d, coef_scaled, ln_f, lw_scaled_max):
    """U = 4 (2 d + 4) 2^-53 (max_k |coef'_k| + |sum_j ln f_j| + max |lw'|)."""
    c = float(np.max(np.abs(coef_scaled))) + abs(float(ln_f)) + float(lw_scaled_max)
    return 4.0 * (2 * d + 4) * 2.0 ** -53 * c


# ---- fp64 restatements (in no kernel's operation order) -------------------------------------------------------------------------------

def whitened_q(X, mu, S):
    """q_ik = |W_k (x_i - mu_k)|^2 of hp_cases' whitening restatement (the host's Cholesky loops, forward substitution, ascending-j
    chains), N x K: the part of a log-weight that must keep its bits under a power-of-two scaling."""
    n, d = X.shape
    q = np.empty((n, len(mu)))
    for k in range(len(mu)):
        _, W = hp_cases.whitening_fp64(S[k])
        c = X - mu[k]
        acc = np.zeros(n)
        for i in range(d):
            y = W[i, 0] * c[:, 0]
            for j in range(1, i + 1):
                y = y + W[i, j] * c[:, j]
            acc = acc + y * y
        q[:, k] = acc
    return q


def log_constants(pi, S):
    """coef_k = log pi_k - sum_j log L_jj - d log(2 pi) / 2 of the restatement, fp64."""
    d = S.shape[-1]
    with np.errstate(divide="ignore"):
        return np.array([math.log(pi[k]) - np.log(np.diag(hp_cases.whitening_fp64(S[k])[0])).sum() - 0.5 * d * math.log(2 * math.pi)
                         for k in range(len(pi))])


def _two_prod(a, b):
    """a b = p + e exactly (Veltkamp / Dekker), elementwise."""
    p = a * b
    split = 134217729.0                                # 2^27 + 1
    ca, cb = split * a, split * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _fma(a, b, c):
    """fl(a b + c) from the exact product and the exact sum of its head with c (the tail's last half-ulp tie apart: a fixed sequence of
    fp64 operations either way, which is all covariance needs)."""
    p, e = _two_prod(a, b)
    s = p + c
    bb = s - p
    return s + (((p - (s - bb)) + (c - bb)) + e)


def direct_distances(X, C):
    """N x K squared distances in the reference's form: s = fma(t, t, s), t = x_j - c_kj, ascending j (ML/KMeans.cpp:155-163)."""
    out = np.empty((X.shape[0], C.shape[0]))
    for k in range(C.shape[0]):
        s = np.zeros(X.shape[0])
        for j in range(X.shape[1]):
            t = X[:, j] - C[k, j]
            s = _fma(t, t, s)
        out[:, k] = s
    return out


def two_pass_mstep(X, R, weights=None):
    """(mixing, means, covariances) from N x K responsibilities: the means first, the second moments about them (no ridge)."""
    n, d = X.shape
    Rw = R if weights is None else R * weights[:, None]
    total = float(n) if weights is None else weights.sum()
    s0 = Rw.sum(axis=0)
    mu = (Rw.T @ X) / s0[:, None]
    covs = np.empty((R.shape[1], d, d))
    for k in range(R.shape[1]):
        c = X - mu[k]
        covs[k] = (c * Rw[:, k][:, None]).T @ c / s0[k]
    return s0 / total, mu, covs


def diag_step_fp64(X, pi, mu, var):
    """One diagonal-covariance EM step in fp64 numpy, log domain, two-pass variances, no ridge: (ll, R, mixing, means, variances) --
    the yardstick where the oracle's linear-domain determinant leaves the fp64 range."""
    n, d = X.shape
    K = len(pi)
    lw = np.empty((n, K))
    for k in range(K):
        c = X - mu[k]
        lw[:, k] = math.log(pi[k]) - 0.5 * np.log(var[k]).sum() - 0.5 * (c * c / var[k]).sum(axis=1) - 0.5 * d * math.log(2 * math.pi)
    top = lw.max(axis=1)
    lse = top + np.log(np.exp(lw - top[:, None]).sum(axis=1))
    R = np.exp(lw - lse[:, None])
    s0 = R.sum(axis=0)
    mu1 = (R.T @ X) / s0[:, None]
    var1 = np.stack([(R[:, k][:, None] * (X - mu1[k]) ** 2).sum(axis=0) / s0[k] for k in range(K)])
    return lse.mean(), R, s0 / n, mu1, var1


def tied_step_fp64(X, pi, mu, S):
    """One tied step from the whitening restatement on K copies of S, pooled as sum_k pi_k Sigma_k in ascending k (no ridge)."""
    K = len(pi)
    ll, R, pi1, mu1, covs, _ = hp_cases.whitened_step_fp64(X, pi, mu, np.stack([S] * K))
    pooled = np.zeros_like(S)
    for k in range(K):
        pooled = pooled + pi1[k] * covs[k]
    return ll, R, pi1, mu1, pooled


def two_pass_covariance(X):
    mean = X.sum(axis=0) / X.shape[0]
    c = X - mean
    return mean, c.T @ c / (X.shape[0] - 1)


def responsibilities(n, K, seed):
    """Seeded responsibilities for the M-step-from-given-responsibilities cases: rows of a Dirichlet with a third of the entries set to
    exactly 0 (renormalised), as a screened E-step leaves them."""
    rng = np.random.default_rng(seed)
    R = rng.dirichlet(np.full(K, 0.7), n)
    if K > 1:
        R[rng.random((n, K)) < 1.0 / 3.0] = 0.0
        R[np.arange(n), rng.integers(0, K, n)] += 1e-3
        R /= R.sum(axis=1, keepdims=True)
    return np.ascontiguousarray(R)


# ---- the case lists -----------------------------------------------------------------------------------------------------------------------
# name, (d, K, N, offset), switches, route: one EM step per row of test_gpu_hp_edges.STEP_ROUTES (restated here, numpy only;
# tests/test_units_cases.py asserts that the copy equals the original), then d = 72 and d = 128
EM_CASES = [
    ("fused vector-unit, d=2 K=3", (2, 3, 3001, 0.0), {}, {"fused": True, "fused_form": "valu"}),
    ("fused scalar-feed, d=8 K=5", (8, 5, 3001, 3.0), {}, {"fused": True, "fused_form": "scalar_feed"}),
    ("fused LDS-feed, d=6 K=8", (6, 8, 3001, 2.0), {}, {"fused": True, "fused_form": "lds_feed"}),
    ("estep scalar-fed + split statistics, d=8", (8, 5, 3001, 3.0), {"MLHIP_FUSED": "0"}, {"estep": "scalar_fed", "fused": False, "self_norm": False}),
    ("matrix-core FOLD + self-norm dense, d=16", (16, 8, 4001, 2.0), {"MLHIP_MSTATS_SPARSE": "0"},
     {"estep": "matrix4", "fused": False, "fold_allowed": True, "self_norm": True, "sparse": False}),
    ("matrix-core FOLD + self-norm sparse, d=16", (16, 8, 4001, 2.0), {"MLHIP_MSTATS_SPARSE": "1"},
     {"estep": "matrix4", "fused": False, "fold_allowed": True, "self_norm": True, "sparse": True}),
    ("matrix-core exact form, d=16", (16, 8, 4001, 2.0), {"MLHIP_ESTEP_FOLD": "0"}, {"estep": "matrix4", "fused": False, "fold_allowed": False}),
    ("split statistics (MLHIP_SELF_NORM=0), d=16 K=24", (16, 24, 5001, 1.0), {"MLHIP_SELF_NORM": "0"},
     {"estep": "matrix4", "fused": False, "self_norm": False}),
    ("sparse K<64 masks, d=32 K=16", (32, 16, 6001, 0.0), {"MLHIP_MSTATS_SPARSE": "1"},
     {"estep": "matrix4", "fused": False, "fold_allowed": True, "self_norm": True, "sparse": True}),
    ("sparse, every slot a component, d=32 K=64", (32, 64, 2001, 0.0), {"MLHIP_MSTATS_SPARSE": "1"},
     {"estep": "matrix4", "fused": False, "fold_allowed": True, "self_norm": True, "sparse": True}),
    ("dense, d=32 K=64", (32, 64, 2001, 0.0), {"MLHIP_MSTATS_SPARSE": "0"},
     {"estep": "matrix4", "fused": False, "fold_allowed": True, "self_norm": True, "sparse": False}),
    ("matrix-core d=33 (above the FOLD range)", (33, 4, 3001, 0.0), {}, {"estep": "matrix4", "fused": False, "fold_allowed": False}),
    ("big-dim d=136 K=2", (136, 2, 1001, 0.0), {}, {"estep": "big_dim", "fused": False, "self_norm": False}),
    ("plain tier d=136 K=2", (136, 2, 1001, 0.0), {"MLHIP_BIG_DIM": "0"}, {"estep": "plain", "fused": False, "self_norm": False}),
    ("panelled closing shape, d=72 K=2", (72, 2, 2501, 0.0), {}, {"estep": "matrix4", "fused": False}),
    ("matrix-core d=128 K=3", (128, 3, 2001, 0.0), {}, {"estep": "matrix4", "fused": False, "fold_allowed": False}),
]
EM_SHAPES = sorted({c[1] for c in EM_CASES})
# the diagonal kernel's three shapes (K <= 16 two-operation, K = 17..64, d = 32), each also with MLHIP_DIAG_AB=0
DIAG_SHAPES = [(16, 8, 4001, 0.5), (7, 40, 4001, 0.0), (32, 8, 3001, 1.0)]
# tied: the kernel and the composed route on one problem
TIED_SHAPE = (7, 5, hp_cases.TIED_N)
# K-means, uniform scalings: name, (d, K, N), switches, route (the mixture samples of test_gpu_hp_error.py's K-means cases, the initial
# means as centroids). Quad tracking starts at K >= 16 d, the chunked table where K (d + 2) doubles leave the LDS budget.
KM_CASES = [
    ("direct, d=5 K=7", (5, 7, 3001), {}, {"kernel": "direct", "pad": False}),
    ("direct forced, d=16 K=10", (16, 10, 3001), {"MLHIP_KMEANS": "valu"}, {"kernel": "direct", "pad": False}),
    ("matrix-core, d=16 K=10", (16, 10, 3001), {}, {"kernel": "matrix", "pad": False}),
    ("matrix-core, d=72 K=6", (72, 6, 2001), {}, {"kernel": "matrix", "pad": False}),
    ("matrix-core on the padded copy, d=5 K=130", (5, 130, 6001), {}, {"kernel": "matrix", "pad": True}),
    ("matrix-core quad tracking, d=4 K=70", (4, 70, 3001), {}, {"kernel": "matrix", "pad": False}),
    ("matrix-core chunked table, d=4 K=3100", (4, 3100, 12001), {}, {"kernel": "matrix", "pad": False}),
    ("big-dim, d=192 K=5", (192, 5, 2001), {}, {"kernel": "big_dim", "pad": False}),
    ("plain tier, d=192 K=5", (192, 5, 2001), {"MLHIP_BIG_DIM": "0"}, {"kernel": "plain", "pad": False}),
]
KM_MIXED_CASES = [("direct, d=5 K=7", (5, 7, 3001), {}, {"kernel": "direct", "pad": False}),
                  ("matrix-core, d=16 K=10", (16, 10, 3001), {}, {"kernel": "matrix", "pad": False})]
KM_RESIDENT_SHAPE = (2, 5, 3001)
KM_WEIGHTED_SHAPE = (8, 9, 3001)
LATTICE_SHAPE = (8, 256, 3001)
# Data.shift / sample_covariance: the small, wide and big-dim statistics kernels at K = 1
DATA_SHAPES = [(6, 3001), (33, 3001), (136, 1001)]
# M-step from given responsibilities: (d, K, N, switches), one per statistics family
MSTEP_CASES = [(3, 4, 3001, {}), (8, 5, 3001, {}), (16, 8, 3001, {}), (16, 24, 3001, {}), (32, 64, 2001, {}), (72, 2, 2001, {}),
               (136, 2, 1001, {}), (136, 2, 1001, {"MLHIP_BIG_DIM": "0"})]
SILHOUETTE_SHAPES = [(2, 700), (8, 700), (32, 700), (40, 700)]
SCREEN_SHAPE = (32, 64, 3000)


def em_problem(shape, scaling=None, diagonal=False):
    """hp_cases.problem at `shape`, rescaled: (X, pi0, mu0, S0 or variances)."""
    d, K, n, offset = shape
    X, pi0, mu0, S0 = hp_cases.problem(d, K, n, offset, diagonal=diagonal)
    if scaling is None:
        return X, pi0, mu0, S0
    f = factors(scaling, d)
    return points(X, f), pi0, points(mu0, f), variances(S0, f) if diagonal else covariances(S0, f)


def tied_problem(scaling=None):
    d, K, n = TIED_SHAPE
    X, pi0, mu0, S0 = hp_cases.tied_problem(d, K, n, 2.0, 2.5)
    if scaling is None:
        return X, pi0, mu0, S0
    f = factors(scaling, d)
    return points(X, f), pi0, points(mu0, f), covariances(S0, f)


def km_problem(shape, scaling=None):
    """The K-means problems of test_gpu_hp_error.py (problem(d, K, n, 2.0), the initial means as centroids): (X, C0)."""
    d, K, n = shape
    X, _, C0, _ = hp_cases.problem(d, K, n, 2.0)
    if scaling is None:
        return X, C0
    f = factors(scaling, d)
    return points(X, f), points(C0, f)


def lattice_problem(scaling=None):
    """The input of test_kmeans_on_an_integer_lattice (exact ties everywhere) at d = 8, K = 256."""
    d, K, n = LATTICE_SHAPE
    rng = np.random.default_rng(77)
    C = rng.integers(-3, 4, (K, d)).astype(np.float64)
    X = np.ascontiguousarray(rng.integers(-3, 4, (n, d)).astype(np.float64))
    X[: n // 4] = C[rng.integers(0, K, n // 4)]
    if scaling is None:
        return X, C
    f = factors(scaling, d)
    return points(X, f), points(C, f)


def row_weights(n, seed=21):
    """Frequency weights with zeros among them (unchanged by a change of units)."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.25, 4.0, n)
    w[rng.random(n) < 0.05] = 0.0
    return w


def undecided_rows(lw_unit, U):
    """Rows whose two largest unit-scale log-weights (N x K) are within 2 U: the label may differ there."""
    if lw_unit.shape[1] < 2:
        return np.zeros(lw_unit.shape[0], dtype=bool)
    top = np.sort(lw_unit, axis=1)
    return (top[:, -1] - top[:, -2]) <= 2 * U
