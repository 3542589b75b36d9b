"""Inputs shared by tests/test_hp_reference.py (CPU) and tests/test_gpu_hp_error.py (GPU): mixture problems, the oracle's step in
the reference's output form, and the problems that sit just below / above a guard of DESIGN.md section 4 (test infrastructure)."""
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
