"""scikit-learn's score_samples / predict / predict_proba of a held-out 'mousie' sample (tests/golden/score_mousie_sklearn.npz, under
the parameters pinned in mousie_sklearn.npz) against the CPU oracle: log-densities 1e-12 relative, posteriors 1e-12, labels equal.
tests/test_gpu_score.py holds the GPU's side of the same fixture. CPU only."""
import numpy as np

from conftest import load_golden
from test_score_cases import oracle_density_rows, oracle_labels


def test_oracle_matches_sklearn_on_the_held_out_mousie_sample(oracle):
    g, s = load_golden("mousie_sklearn.npz"), load_golden("score_mousie_sklearn.npz")
    pi, mu, S, Y = g["sklearn_weights"], g["sklearn_means"], g["sklearn_covariances"], np.ascontiguousarray(s["Y"])
    dens = oracle_density_rows(oracle, Y, pi, mu, S, np.arange(len(Y)))
    labels, resp = oracle_labels(oracle, Y, pi, mu, S)
    assert np.max(np.abs(dens - s["sklearn_score_samples"]) / np.abs(s["sklearn_score_samples"])) <= 1e-12
    assert np.max(np.abs(resp - s["sklearn_predict_proba"])) <= 1e-12
    assert np.array_equal(labels, s["sklearn_predict"])
