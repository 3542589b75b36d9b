"""Writes tests/golden/score_mousie_sklearn.npz: a held-out 'mousie' sample scored by scikit-learn's GaussianMixture under the
parameters already pinned in mousie_sklearn.npz -- score_samples, predict, predict_proba. Needs scikit-learn; run by hand:

    python tests/golden/make_score_golden.py
"""
import os

import numpy as np
import sklearn.mixture
from sklearn.mixture._gaussian_mixture import _compute_precision_cholesky

from make_golden import mousie_numpy

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    g = np.load(os.path.join(HERE, "mousie_sklearn.npz"))
    Y = mousie_numpy(seed=1000, sample_size=500)            # (the fit's sample is seed 999)
    gmm = sklearn.mixture.GaussianMixture(3, covariance_type="full")
    gmm.weights_, gmm.means_, gmm.covariances_ = g["sklearn_weights"], g["sklearn_means"], g["sklearn_covariances"]
    gmm.precisions_cholesky_ = _compute_precision_cholesky(gmm.covariances_, "full")
    np.savez(os.path.join(HERE, "score_mousie_sklearn.npz"), Y=Y, sklearn_score_samples=gmm.score_samples(Y),
             sklearn_predict=gmm.predict(Y).astype(np.uint32), sklearn_predict_proba=gmm.predict_proba(Y))
    proba = np.sort(gmm.predict_proba(Y), axis=1)
    print("held-out mousie: mean log-density", gmm.score(Y), "smallest top-two posterior gap", (proba[:, -1] - proba[:, -2]).min())


if __name__ == "__main__":
    main()
