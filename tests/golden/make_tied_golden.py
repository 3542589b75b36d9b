"""Fixtures of the tied-covariance mode: one EM step of scikit-learn's GaussianMixture(covariance_type="tied") from a perturbed
start, with an independent scipy E-step. Mirrors make_golden.py's make_em_onestep with ONE shared covariance A A^T / d + 0.5 I.

    python tests/golden/make_tied_golden.py        ->  tests/golden/em_tied_onestep_<tag>.npz
(not em_onestep_tied_*: the full-covariance suites take every em_onestep_*.npz for a case of theirs)
"""
import os
import warnings

import numpy as np
import scipy.special
import scipy.stats
import sklearn.mixture

HERE = os.path.dirname(os.path.abspath(__file__))


def make_em_onestep_tied(tag, seed, n, d, K, sep):
    rng = np.random.default_rng(seed)
    means = sep * rng.standard_normal((K, d))
    A = rng.standard_normal((d, d))
    Sigma = A @ A.T / d + 0.5 * np.eye(d)
    w = rng.uniform(0.5, 1.5, K)
    w /= w.sum()
    comp = rng.choice(K, size=n, p=w)
    X = means[comp] + rng.standard_normal((n, d)) @ np.linalg.cholesky(Sigma).T
    # Perturbed starting point (so the step actually moves).
    mu0 = means + 0.3 * rng.standard_normal((K, d))
    B = rng.standard_normal((d, d)) * 0.1
    Sigma0 = Sigma + B @ B.T + 0.1 * np.eye(d)
    pi0 = rng.uniform(0.5, 1.5, K)
    pi0 /= pi0.sum()

    # Independent E-step (scipy): log N(x | mu0_k, Sigma0) + log pi0_k.
    logw = np.stack([scipy.stats.multivariate_normal(mu0[k], Sigma0).logpdf(X) + np.log(pi0[k]) for k in range(K)], axis=1)
    logw = logw.reshape(n, K)
    lse = scipy.special.logsumexp(logw, axis=1)
    R0 = np.exp(logw - lse[:, None])
    ll0 = lse.mean()
    labels0 = np.argmax(R0, axis=1).astype(np.uint32)
    srt = np.sort(R0, axis=1)
    margin = (srt[:, -1] - srt[:, -2]).min() if K > 1 else 1.0

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gmm = sklearn.mixture.GaussianMixture(K, covariance_type="tied", tol=0.0, max_iter=1, reg_covar=1e-15,
                                              weights_init=pi0, means_init=mu0, precisions_init=np.linalg.inv(Sigma0), random_state=0)
        gmm.fit(X)
    assert abs(gmm.lower_bound_ - ll0) < 1e-10 * max(1, abs(ll0)), (gmm.lower_bound_, ll0)
    np.savez(os.path.join(HERE, f"em_tied_onestep_{tag}.npz"), X=X, pi0=pi0, mu0=mu0, Sigma0=Sigma0,
             ll0=ll0, sklearn_lower_bound=gmm.lower_bound_, R0=R0, labels0=labels0, label_margin=margin,
             pi1=gmm.weights_, mu1=gmm.means_, Sigma1=gmm.covariances_)
    print(f"em_tied_onestep_{tag}: n={n} d={d} K={K} ll0={ll0:.12g} min label margin={margin:.3g} cond(Sigma1)={np.linalg.cond(gmm.covariances_):.3g}")


if __name__ == "__main__":
    make_em_onestep_tied("d4_K3", 41, 800, 4, 3, 2.5)
    make_em_onestep_tied("d16_K16", 42, 1500, 16, 16, 2.0)
    make_em_onestep_tied("d32_K8", 43, 1000, 32, 8, 1.5)
    make_em_onestep_tied("d7_K40", 44, 1200, 7, 40, 2.5)
    make_em_onestep_tied("d13_K5", 45, 600, 13, 5, 2.0)
