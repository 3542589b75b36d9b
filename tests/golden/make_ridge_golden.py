"""Fixtures of the covariance ridge (mlhip_data_set_covariance_ridge, scikit-learn's reg_covar): one EM step of scikit-learn's
GaussianMixture with reg_covar = 1e-3 in the three covariance types, from a perturbed start, with an independent scipy E-step.
Mirrors make_golden.py's make_em_onestep / make_em_onestep_diag and make_tied_golden.py's make_em_onestep_tied; each file holds
`ridge` beside their fields.

    python tests/golden/make_ridge_golden.py        ->  tests/golden/em_ridge_onestep_<type>_<tag>.npz
(not em_onestep_* / em_tied_onestep_*: the suites of the default ridge take every file of those names for a case of theirs)
"""
import os
import warnings

import numpy as np
import scipy.special
import scipy.stats
import sklearn.mixture

HERE = os.path.dirname(os.path.abspath(__file__))
RIDGE = 1e-3


def make(covariance_type, tag, seed, n, d, K, sep):
    rng = np.random.default_rng(seed)
    means = sep * rng.standard_normal((K, d))
    if covariance_type == "diag":
        covs = np.stack([np.diag(v) for v in rng.uniform(0.5, 2.0, (K, d))])
    else:
        covs = np.empty((K, d, d))
        for k in range(K):
            A = rng.standard_normal((d, d))
            covs[k] = A @ A.T / d + 0.5 * np.eye(d)
        if covariance_type == "tied":
            covs[:] = covs[0]
    w = rng.uniform(0.5, 1.5, K)
    w /= w.sum()
    comp = rng.choice(K, size=n, p=w)
    X = np.empty((n, d))
    for k in range(K):
        idx = np.where(comp == k)[0]
        X[idx] = means[k] + rng.standard_normal((idx.size, d)) @ np.linalg.cholesky(covs[k]).T
    # Perturbed starting point (so the step actually moves).
    mu0 = means + 0.3 * rng.standard_normal((K, d))
    pi0 = rng.uniform(0.5, 1.5, K)
    pi0 /= pi0.sum()
    if covariance_type == "diag":
        var0 = np.stack([np.diag(c) for c in covs]) * rng.uniform(0.8, 1.3, (K, d)) + 0.05
        Sigma0 = np.stack([np.diag(v) for v in var0])
        start, precisions = {"var0": var0}, 1.0 / var0
    elif covariance_type == "tied":
        B = rng.standard_normal((d, d)) * 0.1
        S = covs[0] + B @ B.T + 0.1 * np.eye(d)
        Sigma0 = np.stack([S] * K)
        start, precisions = {"Sigma0": S}, np.linalg.inv(S)
    else:
        Sigma0 = np.empty_like(covs)
        for k in range(K):
            B = rng.standard_normal((d, d)) * 0.1
            Sigma0[k] = covs[k] + B @ B.T + 0.1 * np.eye(d)
        start, precisions = {"Sigma0": Sigma0}, np.linalg.inv(Sigma0)

    # Independent E-step (scipy): log N(x | mu0_k, Sigma0_k) + log pi0_k. The ridge plays no part in it: parameters a caller gives are used as given.
    logw = np.stack([scipy.stats.multivariate_normal(mu0[k], Sigma0[k]).logpdf(X) + np.log(pi0[k]) for k in range(K)], axis=1)
    logw = logw.reshape(n, K)
    lse = scipy.special.logsumexp(logw, axis=1)
    R0 = np.exp(logw - lse[:, None])
    ll0 = lse.mean()
    labels0 = np.argmax(R0, axis=1).astype(np.uint32)
    srt = np.sort(R0, axis=1)
    margin = (srt[:, -1] - srt[:, -2]).min() if K > 1 else 1.0

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gmm = sklearn.mixture.GaussianMixture(K, covariance_type=covariance_type, tol=0.0, max_iter=1, reg_covar=RIDGE,
                                              weights_init=pi0, means_init=mu0, precisions_init=precisions, random_state=0)
        gmm.fit(X)
    assert abs(gmm.lower_bound_ - ll0) < 1e-10 * max(1, abs(ll0)), (gmm.lower_bound_, ll0)
    out = {"var1" if covariance_type == "diag" else "Sigma1": gmm.covariances_}
    name = f"em_ridge_onestep_{covariance_type}_{tag}"
    np.savez(os.path.join(HERE, name + ".npz"), X=X, pi0=pi0, mu0=mu0, ll0=ll0, sklearn_lower_bound=gmm.lower_bound_, R0=R0,
             labels0=labels0, label_margin=margin, pi1=gmm.weights_, mu1=gmm.means_, ridge=RIDGE, **start, **out)
    print(f"{name}: n={n} d={d} K={K} ll0={ll0:.12g} min label margin={margin:.3g}")


if __name__ == "__main__":
    make("full", "d4_K3", 51, 800, 4, 3, 2.5)
    make("diag", "d7_K5", 52, 700, 7, 5, 2.5)
    make("tied", "d13_K5", 53, 600, 13, 5, 2.0)
