"""Inputs shared by tests/test_hp_reference.py (CPU) and tests/test_gpu_hp_error.py / test_gpu_hp_edges.py (GPU): mixture problems,
the oracle's step in the reference's output form, the problems that sit just below / above a guard of DESIGN.md section 4, and the
inputs no plain sample holds -- a component without mass, rows far in a tail --, and the ill-conditioned mixtures of
tests/test_gpu_hp_ill.py with the fp64 restatement of the whitening form that is their yardstick (test infrastructure)."""
import importlib.util
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def _synth():
    spec = importlib.util.spec_from_file_location("mlamd_synth", os.path.join(ROOT, "ml_amd", "synth.py"))
    mod = importlib.util.module_from_spec(spec)     # (the package itself needs the built library; the generator does not)
    spec.loader.exec_module(mod)
    return mod


synth = _synth()

# the shapes of the GPU module's K-means cases (mixture samples, the initial means as centroids): the reference alone must leave
# out fewer than 0.1 % of the rows by its runner-up margin (checked on the CPU)
KMEANS_SHAPES = [(2, 5, 3001), (5, 7, 3001), (16, 10, 3001), (72, 6, 2001), (5, 130, 6001), (192, 5, 2001)]


def problem(d, K, n, offset, diagonal=False, seed=11):
    mix = synth.Mixture(d, K, seed=seed, diagonal=diagonal)
    X, _ = mix.sample(n, threads=1)
    X = np.ascontiguousarray(X + offset)
    mu0 = mix.initial_means() + offset
    S0 = np.tile(np.var(X, axis=0), (K, 1)) if diagonal else np.stack([np.cov(X.T)] * K)
    return X, np.full(K, 1.0 / K), mu0, S0


def oracle_step(orc, X, pi0, mu0, S0, diagonal=False):
    """(log-likelihood, responsibilities, mixing, means, covariances / variances) of the oracle, the ridge taken off again."""
    d = X.shape[1]
    em = orc.EM(len(pi0))
    if diagonal:
        em.set_covariance_type("diag")
        em.set_parameters(mu0, np.stack([np.diag(v) for v in S0]), pi0)
    else:
        em.set_parameters(mu0, S0, pi0)
    em.expectation_step(X)
    ll, resp = em.log_likelihood, em.responsibilities
    em.maximisation_step(X)
    S = em.covariances.astype(LD) - LD(1e-15) * np.eye(d, dtype=LD)
    if diagonal:
        S = np.stack([np.diag(s) for s in S])
    return ll, resp, em.mixing_probabilities, em.means, S


def refinement_problem(d, target, seed=3):
    """Two well separated unit-variance clusters (identity starting covariances: hard responsibilities), the smaller one placed so
    that its NEW mean sits sqrt(target) of its NEW standard deviations from the data mean along axis 0."""
    rng = np.random.default_rng(seed)
    n, n1 = 3001, 600
    z0, z1 = rng.standard_normal((n - n1, d)), rng.standard_normal((n1, d))
    f = n1 / n
    s1 = z1[:, 0].std()
    delta = math.sqrt(target) * s1 / (1 - f) - z1[:, 0].mean() + z0[:, 0].mean()
    z1[:, 0] += delta
    X = np.vstack([z0, z1]) + 1.5
    X = np.ascontiguousarray(X[rng.permutation(n)])
    mu0 = np.vstack([np.full(d, 1.5), np.full(d, 1.5)])
    mu0[1, 0] += delta
    return X, np.array([0.7, 0.3]), mu0, np.stack([np.eye(d)] * 2)


def edge_problem(d, reach, diagonal=False, seed=4):
    """Three components for a guard on the distance of a mean from the statistics' shift (the data mean), measured in the
    component's own whitened coordinates: a heavy cluster 0 (80 % of the rows) holds the shift, clusters 1 and 2 OVERLAP each other
    (centres one whitened unit apart, one shared covariance: responsibilities strictly inside (0, 1) on their rows) and sit
    `reach` away: W_1 (mu_1 - shift) = reach * u with u_0 = 1 and |u_j| = 1/2 elsewhere (full covariances: max-norm reach), or
    u = 1 / sqrt(d) on every axis (diagonal: B2_1 = reach^2); component 2 is one unit nearer to the shift, so component 1 carries
    the largest value. Covariances are dense random SPD matrices (diagonal mode: random variances), the starting parameters the
    clusters' own. Returns (X, mixing, means, covariances or variances)."""
    rng = np.random.default_rng(seed)
    n, n1 = 3001, 300
    n0 = n - 2 * n1
    if diagonal:
        var = rng.uniform(0.5, 2.0, (2, d))
        L = [np.diag(np.sqrt(v)) for v in var]
        u = np.full(d, 1 / math.sqrt(d))
        w = -u + 0.3 * np.where(np.arange(d) % 2 == 0, 1.0, -1.0) / math.sqrt(d)
    else:
        A = rng.standard_normal((2, d, d))
        S = [a @ a.T / d + 0.5 * np.eye(d) for a in A]
        L = [np.linalg.cholesky(s) for s in S]
        u = 0.5 * np.where(np.arange(d) % 2 == 0, 1.0, -1.0)
        u[0] = 1.0
        w = 0.3 * np.where(np.arange(d) % 3 == 0, 1.0, -1.0)
        w[0] = -1.0
    z0 = rng.standard_normal((n0, d)) @ L[0].T + 0.75
    z1 = rng.standard_normal((n1, d)) @ L[1].T
    z2 = rng.standard_normal((n1, d)) @ L[1].T + L[1] @ w
    f = 2 * n1 / n
    s_base = (z0.sum(axis=0) + z1.sum(axis=0) + z2.sum(axis=0)) / n          # the shift with clusters 1, 2 at the origin
    p = (s_base + reach * (L[1] @ u)) / (1 - f)                                # centre of cluster 1: p - shift = reach L_1 u
    X = np.vstack([z0, z1 + p, z2 + p])
    X = np.ascontiguousarray(X[rng.permutation(n)])
    mu0 = np.vstack([np.full(d, 0.75), p, p + L[1] @ w])
    second = np.stack([var[0], var[1], var[1]]) if diagonal else np.stack([S[0], S[1], S[1]])
    return X, np.array([n0 / n, n1 / n, n1 / n]), mu0, second


# ---- inputs no plain sample holds (tests/test_gpu_hp_edges.py on the GPU, their data conditions in tests/test_hp_reference.py) -----

MASSLESS_KINDS = ("zero_weight_first", "zero_weight_last", "far", "hole")
TAIL_ROWS = 20
TAIL_GAP = 8.0                    # a moved row's runner-up lies at least this far below its winner, in log-weight
HOLE_UNITS = 400.0
ZERO_ROWS = 40
# (d, K, N, offset) of the GPU module's cases: one step on every full-covariance route, the loops' extra shape, the diagonal routes
# (K <= 16 and K = 17..64) and the weighted routes
EDGE_SHAPES = [(2, 3, 3001, 0.0), (8, 5, 3001, 3.0), (6, 8, 3001, 2.0), (16, 8, 4001, 2.0), (16, 24, 5001, 1.0), (32, 16, 6001, 0.0),
               (32, 64, 2001, 0.0), (33, 4, 3001, 0.0), (136, 2, 1001, 0.0)]
EDGE_LOOP_SHAPES = [(72, 2, 2501, 0.0)]
EDGE_DIAG_SHAPES = [(16, 8, 4001, 0.5), (7, 40, 4001, 0.0)]
EDGE_WEIGHTED_SHAPES = [(16, 8, 4001, 2.0), (8, 5, 3001, 3.0)]
# (d, the dead component in front) of massless_refinement_problem: the fused kernel, the matrix-core E-step + statistics kernel
MASSLESS_REFINEMENT_CASES = [(8, True), (32, False)]


def tail_window(d):
    """The open interval a moved tail row's largest log-weight must lie in: (-900, -750) -- below the underflow of a linear-domain
    density, yet of the size the 40 whitened units are chosen for. At d = 136 the density's constant -d/2 log 2 pi = -125 alone puts
    the same 40 units at -943: (-950, -750) there."""
    return (-950.0 if d >= 136 else -900.0), -750.0


def tail_row_is_clear(k, top, gap, winner, d):
    """The condition on ONE moved row (tests/test_hp_reference.py asserts it for every row): won by its own component, inside
    tail_window(d), the runner-up at least TAIL_GAP below."""
    lo, hi = tail_window(d)
    return bool(winner == k and lo < top < hi and gap >= TAIL_GAP)


def _factors(S0, diagonal):
    return [np.diag(np.sqrt(v)) for v in S0] if diagonal else [np.linalg.cholesky(s) for s in S0]


def massless_problem(kind, d, K, n, offset, diagonal=False):
    """problem(d, K, n, offset, diagonal) with ONE component that takes no mass in the step: (X, pi0, mu0, S0, k).
    `zero_weight_first` / `zero_weight_last`: pi_k = 0 for k = 0 / K - 1, the rest renormalised. `far`: mu_(K-1) = shift +
    1e4 sqrt(diag Sigma_(K-1)), shift the fp64 data mean -- beyond every reach guard, so the exact density forms run. `hole`:
    mu_(K-1) = shift and Sigma_(K-1) = tiny^2 I with tiny = (the smallest distance of a row from the shift) / 400 -- at reach 0
    (fold = b2 = 0: the FOLD and two-operation forms stay on), yet every row at least 400 of its whitened units away."""
    X, pi0, mu0, S0 = problem(d, K, n, offset, diagonal)
    pi0, mu0, S0 = pi0.copy(), mu0.copy(), S0.copy()
    shift = X.mean(axis=0)
    k = 0 if kind == "zero_weight_first" else K - 1
    if kind in ("zero_weight_first", "zero_weight_last"):
        pi0[k] = 0.0
        pi0 /= pi0.sum()
    elif kind == "far":
        mu0[k] = shift + 1e4 * np.sqrt(S0[k] if diagonal else np.diag(S0[k]))
    elif kind == "hole":
        tiny = np.linalg.norm(X - shift, axis=1).min() / HOLE_UNITS
        mu0[k] = shift
        S0[k] = np.full(d, tiny ** 2) if diagonal else tiny ** 2 * np.eye(d)
    else:
        raise ValueError(kind)
    return X, pi0, mu0, S0, k


def tail_problem(d, K, n, offset, diagonal=False, only_clear=False, seed=5):
    """problem(...) with TAIL_ROWS seeded rows moved 40 whitened units straight out behind a mean: for t = 0 .. TAIL_ROWS - 1 and
    k = t mod K the row becomes mu_k + 40 L_k u, u = unit(L_k^-1 (mu_k - shift)) (log-weights near -800, where a linear-domain
    sum has underflowed). `only_clear` (K above TAIL_ROWS, where neighbours crowd): a row is moved only if tail_row_margins() of
    its new place passes. Returns (X, pi0, mu0, S0, rows, their components)."""
    X, pi0, mu0, S0 = problem(d, K, n, offset, diagonal)
    X = X.copy()
    shift = X.mean(axis=0)
    L = _factors(S0, diagonal)
    picked = np.random.default_rng(seed).choice(n, TAIL_ROWS, replace=False)
    rows, comps = [], []
    for t, row in enumerate(picked):
        k = t % K
        u = np.linalg.solve(L[k], mu0[k] - shift)
        x = mu0[k] + 40.0 * (L[k] @ (u / np.linalg.norm(u)))
        if only_clear:
            top, gap, winner = tail_row_margins(x[None], pi0, mu0, S0, diagonal)
            if not tail_row_is_clear(k, top[0], gap[0], winner[0], d):
                continue
        X[row] = x
        rows.append(int(row))
        comps.append(k)
    return np.ascontiguousarray(X), pi0, mu0, S0, np.array(rows), np.array(comps)


def tail_row_margins(rows, pi0, mu0, S0, diagonal=False):
    """(largest log-weight, its distance to the runner-up, the winner) of each row, from the extended-precision log-weights."""
    from oracle import hp_reference as hp
    lw = (hp.log_weights_diag if diagonal else hp.log_weights)(rows, pi0, mu0, S0)
    order = np.sort(lw, axis=0)
    return order[-1].astype(np.float64), (order[-1] - order[-2]).astype(np.float64), lw.argmax(axis=0)


def zero_weight_rows_problem(d, K, n, offset, w, seed=6):
    """A component alive on the block and exactly massless on the WEIGHTED sample: mu_(K-1) = shift + 200 L e_0 (L the factor of
    Sigma_(K-1): 200 whitened units from the data mean), ZERO_ROWS seeded rows overwritten with mu_(K-1) + 0.05 L z and given
    weight 0; every other row keeps its weight in `w`. Returns (X, weights, pi0, mu0, S0, the rows)."""
    X, pi0, mu0, S0 = problem(d, K, n, offset)
    X, mu0, w = X.copy(), mu0.copy(), np.array(w, dtype=np.float64)
    rng = np.random.default_rng(seed)
    L = np.linalg.cholesky(S0[K - 1])
    mu0[K - 1] = X.mean(axis=0) + 200.0 * L[:, 0]
    rows = np.sort(rng.choice(n, ZERO_ROWS, replace=False))
    X[rows] = mu0[K - 1] + 0.05 * rng.standard_normal((ZERO_ROWS, d)) @ L.T
    w[rows] = 0.0
    return np.ascontiguousarray(X), w, pi0, mu0, S0, rows


def massless_refinement_problem(d, target, first):
    """refinement_problem(d, target) -- one live component at `target` x its variance from the shift, above MLHIP_REFINE_RATIO for
    target > 1e4 -- with a third component of mixing weight 0 put in front (`first`) or behind: the refinement pass must run for the
    live component above the guard and skip the dead one. Returns (X, pi0, mu0, S0, k)."""
    X, pi0, mu0, S0 = refinement_problem(d, target)
    k = 0 if first else 2
    dead_mu, dead_S = X.mean(axis=0)[None], np.eye(d)[None]
    order = (lambda dead, live: np.concatenate([dead, live])) if first else (lambda dead, live: np.concatenate([live, dead]))
    return X, order(np.zeros(1), pi0), order(dead_mu, mu0), order(dead_S, S0), k


def massless_pattern(step, k):
    """True when a step's (ll, resp, mixing, means, second moments) shows the documented pattern of a component without mass
    (DESIGN.md section 4.1): column k of the responsibilities exactly 0, pi_k = 0, mu_k and Sigma_k / var_k NaN in every entry,
    everything else (the log-likelihood included) finite. `resp` may be None."""
    ll, resp, mixing, means, second = step
    f = lambda a: np.asarray(a, dtype=np.float64)   # noqa: E731
    live = np.arange(len(f(mixing))) != k
    ok = bool(np.isfinite(float(ll))) and f(mixing)[k] == 0 and bool(np.isfinite(f(mixing)).all())
    if resp is not None:
        ok = ok and not f(resp)[:, k].any() and bool(np.isfinite(f(resp)).all())
    return bool(ok and np.isnan(f(means)[k]).all() and np.isfinite(f(means)[live]).all()
                and np.isnan(f(second)[k]).all() and np.isfinite(f(second)[live]).all())


# ---- tied covariance: tests/test_gpu_tied_hp.py on the GPU, the data conditions in tests/test_hp_reference.py ----

TIED_N = 709                      # 12 tiles of 64 rows with a ragged last one, in 3 workgroups
# every padded dimension of em_tied_kernel (1, 2, 3, 4, 6, 8, 12, 16, 20, 24, 28, 32) at the largest d below it that still pads to
# it, d = D itself at D = 20, 24, 28, each with 1, 2 and 3 row blocks of components; then the other row-block boundaries
TIED_CODE_OBJECT_CASES = ([(d, K) for d in (1, 2, 3, 4, 5, 7, 11, 15, 17, 21, 25, 29, 20, 24, 28) for K in (5, 17, 33)] +
                          [(d, K) for d in (7, 21) for K in (16, 32, 48, 49, 64)])
# (offset, separation) at d = 8, K = 5, N = 3001
TIED_SWEEP_CASES = [(0.0, 2.5), (0.0, 30.0), (0.0, 300.0), (50.0, 30.0)]
TIED_REACHES = [0.9 * 64, 1.1 * 64, 10 * 64]
# The whitening model's constant (section 4): the largest ratio of tied_kernel_log_resp()'s log-responsibility error to
# 2^-53 * whiten over TIED_SWEEP_CASES and TIED_REACHES is 1.21 (tests/test_hp_reference.py measures it), rounded up to the next
# integer. It comes from this CPU restatement, never from what the kernel gives.
C_WHITEN = 2


def tied_problem(d, K, n, offset=0.0, sep=2.5, seed=None):
    """A tied mixture sample and a perturbed start (X, pi0, mu0, Sigma0) -- tests/test_gpu_tied.py's tied_sample with the component
    means `sep` apart per axis and everything moved `offset` from the origin."""
    rng = np.random.default_rng(100 * d + K + n if seed is None else seed)
    means = sep * rng.standard_normal((K, d))
    A = rng.standard_normal((d, d))
    Sigma = A @ A.T / d + 0.5 * np.eye(d)
    X = means[rng.integers(0, K, n)] + rng.standard_normal((n, d)) @ np.linalg.cholesky(Sigma).T
    B = 0.1 * rng.standard_normal((d, d))
    pi0 = rng.dirichlet(4 * np.ones(K))
    mu0 = means + 0.2 * rng.standard_normal((K, d))
    return np.ascontiguousarray(X + offset), pi0, mu0 + offset, Sigma + B @ B.T + 0.1 * np.eye(d)


def tied_reach_problem(reach):
    """edge_problem(16, reach) -- components 1 and 2 share one covariance and overlap, `reach` of their whitened units from the
    shift -- with its three covariances pooled as the one starting covariance."""
    X, pi0, mu0, S = edge_problem(16, reach)
    return X, pi0, mu0, np.einsum("k,kab->ab", pi0, S)


def tied_edge_problem(kind):
    """d = 7, K = 5, N = 709 with one input no plain sample holds. `zero_weight`: pi_2 = 0. `empty`: component 4's mean 1e4 whitened
    units from the data mean, so that every one of its responsibilities underflows to exactly 0 (in long double too). `tail`: twenty
    rows moved out along random directions until the NEAREST mean is 40 whitened units away (log-densities near -800)."""
    d, K, n = 7, 5, TIED_N
    X, pi0, mu0, S0 = tied_problem(d, K, n, 2.0, 2.5)
    L = np.linalg.cholesky(S0)
    if kind == "zero_weight":
        pi0 = pi0.copy()
        pi0[2] = 0.0
        pi0 /= pi0.sum()
    elif kind == "empty":
        mu0 = mu0.copy()
        mu0[4] = X.mean(axis=0) + 1e4 * L[:, 0]
    elif kind == "tail":
        rng = np.random.default_rng(5)
        X = X.copy()
        centre = X.mean(axis=0)
        M = np.linalg.solve(L, (mu0 - centre).T).T
        for row in rng.choice(n, 20, replace=False):
            u = rng.standard_normal(d)
            u /= np.linalg.norm(u)
            lo, hi = 0.0, 200.0                       # (the nearest mean's distance grows with t beyond the means themselves)
            for _ in range(60):
                t = (lo + hi) / 2
                lo, hi = (t, hi) if np.linalg.norm(t * u - M, axis=1).min() < 40 else (lo, t)
            X[row] = centre + L @ (hi * u)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(X), pi0, mu0, S0


def oracle_tied_step(orc, X, pi0, mu0, S0):
    """The CPU yardstick of a tied step, in em_step_tied's output form: the oracle's full-covariance step on K copies of the
    covariance, pooled as sum_k pi_k Sigma_k in ascending k in fp64 (the composed route's arithmetic, runtime/em.cpp), the ridge --
    every Sigma_k carries it and the weights sum to 1 -- taken off once."""
    K, d = len(pi0), X.shape[1]
    em = orc.EM(K)
    em.set_parameters(mu0, np.stack([S0] * K), pi0)
    em.expectation_step(X)
    ll, resp = em.log_likelihood, em.responsibilities
    em.maximisation_step(X)
    pi1, covs = em.mixing_probabilities, em.covariances
    pooled = np.zeros((d, d))
    for k in range(K):
        pooled = pooled + pi1[k] * covs[k]
    return ll, resp, pi1, em.means, pooled.astype(LD) - LD(1e-15) * np.eye(d, dtype=LD)


def tied_kernel_log_resp(X, pi0, mu0, S0):
    """em_tied_kernel's density arithmetic restated in fp64 numpy (device/em_tied.hip, host::build_tied_params): W = L^-1,
    x~ = x - shift, y_i = sum_(j <= i) W_ij x~_j and m_ki = sum_(j <= i) W_ij (mu_kj - shift_j) as ascending-j chains without
    fused multiply-adds, z = y - m_k, q = sum_j z_j^2 ascending, lw_k = (log pi_k - sum_j log L_jj) - q / 2, then the
    log-sum-exp about the maximum. Returns the N x K log-responsibilities."""
    n, d = X.shape
    shift = X.mean(axis=0)
    L = np.linalg.cholesky(S0)
    W = np.linalg.solve(L, np.eye(d))
    Xt = X - shift
    Y = np.empty((n, d))
    for i in range(d):
        t = W[i, 0] * Xt[:, 0]
        for j in range(1, i + 1):
            t = t + W[i, j] * Xt[:, j]
        Y[:, i] = t
    with np.errstate(divide="ignore"):
        coef = np.log(pi0) - np.log(np.diag(L)).sum()
    lw = np.empty((n, len(pi0)))
    for k in range(len(pi0)):
        q = np.zeros(n)
        for i in range(d):
            m = 0.0
            for j in range(i + 1):
                m = m + W[i, j] * (mu0[k, j] - shift[j])
            z = Y[:, i] - m
            q = q + z * z
        lw[:, k] = coef[k] - 0.5 * q
    top = lw.max(axis=1)
    lse = top + np.log(np.exp(lw - top[:, None]).sum(axis=1))
    return lw - lse[:, None]


def tied_whitening_ratio(X, pi0, mu0, S0):
    """(the restatement's largest log-responsibility error over the pairs with r_ik >= 1e-6) / (2^-53 * whiten), and whiten."""
    from oracle import hp_reference as hp
    ref = hp.em_step_tied(X, pi0, mu0, S0)
    whiten = hp.tied_conditioning(X, X.astype(LD).mean(axis=0), mu0, S0, ref[4], resp=ref[1])["whiten"]
    pairs = ref[1] >= 1e-6
    err = np.abs(tied_kernel_log_resp(X, pi0, mu0, S0).astype(LD)[pairs] - np.log(ref[1][pairs])).max()
    return float(err) / (hp.EPS64 * whiten), whiten


def tied_step_fp64(X, pi, mu, S):
    """One tied EM step in fp64 numpy for blocks too long for the long-double reference: whitens the sample ONCE, one N x d
    temporary per component, the covariance in its two-pass form + 1e-15 I. Returns (ll, responsibilities, pi1, mu1, Sigma1)."""
    n, d = X.shape
    K = len(pi)
    L = np.linalg.cholesky(S)
    Y = np.linalg.solve(L, X.T).T
    M = np.linalg.solve(L, mu.T).T
    lw = np.empty((n, K))
    for k in range(K):
        Z = Y - M[k]
        lw[:, k] = np.log(pi[k]) - np.log(np.diag(L)).sum() - 0.5 * (Z * Z).sum(axis=1) - 0.5 * d * math.log(2 * math.pi)
    top = lw.max(axis=1)
    lse = top + np.log(np.exp(lw - top[:, None]).sum(axis=1))
    R = np.exp(lw - lse[:, None])
    s0 = R.sum(axis=0)
    mu1 = R.T @ X / s0[:, None]
    S1 = np.zeros((d, d))
    for k in range(K):
        D = X - mu1[k]
        S1 += (D * R[:, k][:, None]).T @ D
    return lse.mean(), R, s0 / n, mu1, S1 / n + 1e-15 * np.eye(d)


def tied_grid(d, K, n, num_cus):
    """Workgroups in x of an em_tied_kernel launch (device/em_tied.hip, em_tied_grid): one or two per CU by registers and LDS,
    halved when the components need two row-block groups, never more than the 64-row tiles fill at 4 waves each."""
    padded = next(p for p in (1, 2, 3, 4, 6, 8, 12, 16, 20, 24, 28, 32) if p >= d)
    row_blocks = (K + 15) // 16
    per_cu = 2 if padded <= 16 and row_blocks <= 2 else 1
    grid = per_cu * num_cus // (2 if row_blocks >= 3 else 1)
    return max(1, min(grid, ((n + 63) // 64 + 3) // 4))


def tied_many_tiles_rows(d, K, num_cus):
    """N at which every wave of the launch takes two whole tiles and the first ones a third, ragged one."""
    return 64 * 4 * tied_grid(d, K, 2 ** 31, num_cus) * 2 + 37


# ---- ill-conditioned covariances: tests/test_gpu_hp_ill.py on the GPU, the data conditions and the constants in
# ---- tests/test_hp_reference.py ----------------------------------------------------------------------------------------------------

ILL_CONDS = (1e6, 1e8)
# (d, K, N): every E-step / statistics family, the closings (registers to d = 32, LDS to 64, panelled above) and the tiers above d = 128
ILL_SHAPES = [(2, 3, 3001), (3, 4, 3001), (8, 5, 3001), (6, 8, 3001), (16, 8, 4001), (24, 6, 3001), (32, 16, 6001), (33, 4, 3001),
              (64, 4, 3001), (72, 3, 2501), (128, 3, 2001), (136, 3, 2001)]
# seed 7 unless the case needs another one for max |W (mu - shift)| to stay 5 % clear of the FOLD guard (tests/test_hp_reference.py)
ILL_SEEDS = {(16, 8, 4001, 1e8): 8, (33, 4, 3001, 1e8): 8}          # (seed 7 gives 63.6 and 65.0)
# The whitening model's constants (section 4): per output 4 x the largest constant whitened_step_fp64() needs over ILL_SHAPES x
# ILL_CONDS in units of sqrt(N_k) 2^-53 kappa_k (tests/test_hp_reference.step_errors; an entry below the floor of its limit --
# tests/hp_limits.ill_limits -- needs none). `lse`: the per-row log-density, absolute, in the responsibilities' unit -- far above
# `resp`, because the light components share W and x, so that most of a row's error in y is common to their log-weights and
# leaves the responsibilities, yet stays in the density; `ll2`: the log-likelihood of a second E-step on the restatement's own new
# parameters (+ the ridge), in units of sqrt(N) 2^-53 max kappa(new covariances). Measured on this CPU restatement (largest values:
# ll 0.040, resp 0.964, mixing 0.008, means 0.072, covs 0.233, lse 27.5, ll2 0.0092; tests/test_hp_reference.py asserts them,
# `python tests/test_hp_reference.py` prints them, oracle/README.md holds the per-case figures), never on a kernel.
C_ILL = {"ll": 4 * 0.05, "resp": 4 * 1.0, "mixing": 4 * 0.01, "means": 4 * 0.08, "covs": 4 * 0.3, "lse": 4 * 30.0, "ll2": 4 * 0.01}


def ill_seed(d, K, n, cond):
    return ILL_SEEDS.get((d, K, n, cond), 7)


def ill_problem(d, K, n, cond, seed=7, sep=1.0, offset=1.5):
    """A heavy, well conditioned component 0 (60 % of the rows, S = A A^T / d + I / 2, centred at the origin) and K - 1 light ones
    that share S1 = Q diag(logspace(0, -log10 cond, d)) Q^T (condition number `cond`, kappa ~ sqrt(cond)) and OVERLAP: centres
    3 Q[:, 0] + j sep L1 u, j = 0 .. K - 2, u a random unit vector -- a chain `sep` whitened units apart, responsibilities strictly
    inside (0, 1) on their rows. Rows shuffled, everything moved by `offset`, the starting parameters the clusters' own. One
    default_rng(seed), drawn in the order Q, A, u, heavy rows, light rows, permutation. Returns (X, pi0, mu0, S0)."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    A = rng.standard_normal((d, d))
    u = rng.standard_normal(d)
    u /= np.linalg.norm(u)
    S_heavy = A @ A.T / d + 0.5 * np.eye(d)
    S1 = (Q * np.logspace(0, -math.log10(cond), d)) @ Q.T
    S1 = (S1 + S1.T) / 2
    L0, L1 = np.linalg.cholesky(S_heavy), np.linalg.cholesky(S1)
    n1 = int(0.4 * n / (K - 1))
    n0 = n - (K - 1) * n1
    centres = np.vstack([np.zeros(d)] + [3 * Q[:, 0] + j * sep * (L1 @ u) for j in range(K - 1)])
    blocks = [rng.standard_normal((n0, d)) @ L0.T]
    for j in range(1, K):
        blocks.append(rng.standard_normal((n1, d)) @ L1.T + centres[j])
    X = np.vstack(blocks)[rng.permutation(n)]
    pi0 = np.array([n0 / n] + [n1 / n] * (K - 1))
    return np.ascontiguousarray(X + offset), pi0, centres + offset, np.stack([S_heavy] + [S1] * (K - 1))


def whitening_fp64(S):
    """(L, W = L^-1) of one covariance in fp64: the left-looking Cholesky loops and the forward substitution of host/em_math.cpp
    -- every entry receives its terms in ascending l, one product and one subtraction at a time --, vectorised over the row index
    (the factor) and over the column of W."""
    d = S.shape[0]
    L = np.zeros((d, d))
    for j in range(d):
        col = S[j:, j].copy()
        for l in range(j):
            col -= L[j:, l] * L[j, l]
        L[j, j] = math.sqrt(col[0])
        L[j + 1:, j] = col[1:] / L[j, j]
    W = np.zeros((d, d))
    for i in range(d):
        t = np.zeros(d)
        t[i] = 1.0
        for l in range(i):
            t -= L[i, l] * W[l]
        W[i] = t / L[i, i]
    return L, np.tril(W)


def _whitened_log_weights_fp64(X, pi, mu, S):
    n, d = X.shape
    lw = np.empty((n, len(pi)))
    for k in range(len(pi)):
        L, W = whitening_fp64(S[k])
        c = X - mu[k]
        q = np.zeros(n)
        for i in range(d):
            y = W[i, 0] * c[:, 0]
            for j in range(1, i + 1):
                y = y + W[i, j] * c[:, j]
            q = q + y * y
        lw[:, k] = -0.5 * q + math.log(pi[k]) - np.log(np.diag(L)).sum() - 0.5 * d * math.log(2 * math.pi)
    top = lw.max(axis=1)
    return lw, top + np.log(np.exp(lw - top[:, None]).sum(axis=1))


def whitened_log_likelihood_fp64(X, pi, mu, S):
    """The density part of whitened_step_fp64 alone: (mean log-likelihood, the per-row log-sum-exp)."""
    lse = _whitened_log_weights_fp64(X, pi, mu, S)[1]
    return lse.mean(), lse


def whitened_step_fp64(X, pi0, mu0, S0):
    """The kernels' algorithm restated in fp64 numpy, in no kernel's operation order (the whitening model's yardstick, as
    tied_kernel_log_resp is the tied kernel's): L by the host's Cholesky loops and W = L^-1 by forward substitution,
    y = W (x - mu) accumulated by ascending column, q = sum_j y_j^2, lw = -q / 2 + log pi - sum_j log L_jj - d log(2 pi) / 2, the
    log-sum-exp about the maximum, then the shared-shift statistics s0 = sum r, s1 = sum r x~, S2 = sum r x~ x~^T about the data
    mean (x~ = x - shift) closed as host::finalize_mstep closes them -- m = s1 / s0, mu = shift + m, Sigma = (S2 - s1 m^T) / s0 --
    without the ridge. Returns (ll, responsibilities N x K, mixing, means, covariances, the per-row log-sum-exp)."""
    n, d = X.shape
    lw, lse = _whitened_log_weights_fp64(X, pi0, mu0, S0)
    R = np.exp(lw - lse[:, None])
    shift = X.mean(axis=0)
    Xt = X - shift
    s0 = R.sum(axis=0)
    s1 = R.T @ Xt
    m = s1 / s0[:, None]
    covs = np.empty((len(pi0), d, d))
    for k in range(len(pi0)):
        S2 = (Xt * R[:, k][:, None]).T @ Xt
        covs[k] = (S2 - np.outer(s1[k], m[k])) / s0[k]
        covs[k] = np.tril(covs[k]) + np.tril(covs[k], -1).T
    return lse.mean(), R, s0 / n, shift + m, covs, lse
