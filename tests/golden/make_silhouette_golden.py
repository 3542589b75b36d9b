"""Writes tests/golden/silhouette_*.npz from sklearn.metrics.silhouette_samples (scikit-learn 1.7.2): the third-party pin of the
silhouette's definition and conventions (singletons score 0, unused labels are ignored). The data are CENTRED, so scikit-learn's
expansion |x|^2 + |y|^2 - 2 x.y, which cancels far from the origin, is not what is being measured. Run from the repository root:
    python tests/golden/make_silhouette_golden.py"""
import os

import numpy as np
import sklearn
from sklearn.metrics import silhouette_samples

HERE = os.path.dirname(os.path.abspath(__file__))

# name: (N, d, K, seed, relabel)
CASES = {
    "blobs_d2_K3": (300, 2, 3, 1, None),
    "blobs_d5_K4": (257, 5, 4, 2, None),
    "blobs_d17_K6": (200, 17, 6, 3, None),
    "singletons_d3_K5": (120, 3, 5, 4, "singletons"),
    "unused_labels_d4_K9": (150, 4, 3, 5, "unused"),
}


def make(n, d, K, seed, relabel):
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(K, d)) * 3
    labels = rng.integers(0, K, size=n)
    X = centres[labels] + rng.normal(size=(n, d))
    X -= X.mean(axis=0)
    if relabel == "singletons":
        labels[3], labels[77] = K, K + 1            # two rows alone in their clusters
    if relabel == "unused":
        labels = labels * 3 + 1                     # labels 1, 4, 7: the others stay unused
    return np.ascontiguousarray(X), labels.astype(np.int64)


def main():
    for name, spec in CASES.items():
        X, labels = make(*spec)
        s = silhouette_samples(X, labels, metric="euclidean")
        np.savez_compressed(os.path.join(HERE, f"silhouette_{name}.npz"), X=X, labels=labels, s=s, sklearn_version=sklearn.__version__)
        print(name, X.shape, "mean s", s.mean())


if __name__ == "__main__":
    main()
