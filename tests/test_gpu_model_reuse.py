"""One model object reused across fits (the facade behind cppyml.clustering keeps a device context, the last fit's handle and its
results): after every fit of a sequence -- full, tied, diagonal, weighted, full again, three initialisations, another ridge and back,
another data block -- the object must hold the BITS a fresh object holds that was given the same setters and that fit alone.
Between the fits the used object samples, conditions, scores and predicts; those results are compared too. The same for KMeans.
No tolerance: tests/test_gpu_handle_transitions.py's rule, one level up."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEFAULT_RIDGE = 1e-15


def _blobs(n, d, seed):
    rng = np.random.default_rng(seed)
    centres = 4.0 * rng.standard_normal((3, d))
    return np.ascontiguousarray(centres[rng.integers(0, 3, n)] + rng.standard_normal((n, d)) + 2.0)


def _same(a, b):
    if np.ndim(a) == 0 and np.ndim(b) == 0:
        return np.float64(a).tobytes() == np.float64(b).tobytes()
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _em_state(em, X):
    """What a fit leaves on the object, then what the object computes from it."""
    K = em.number_components
    observed = [0, 2]
    X_obs = np.ascontiguousarray(X[:300, observed])
    out = [em.log_likelihood, em.means, em.mixing_probabilities, *[em.covariance(k) for k in range(K)], em.labels, em.steps_done,
           em.converged, em.best_initialisation, em.initialisation_log_likelihoods]
    out += [*em.sample(257, seed=3), *em.conditional_mean(X_obs, observed, return_log_density=True),
            *em.conditional_sample(X_obs, observed, n_draws=2, seed=9, return_labels=True), em.score_samples(X[:500]),
            em.predict(X[:500])]
    return out


def _configure_em(em, spec, have=None):
    """The setters of `spec`; with `have` (the spec the object was last given) only those that change."""
    changed = lambda key: have is None or have[key] != spec[key]
    if have is None:
        em.set_absolute_tolerance(1e-8)
        em.set_relative_tolerance(1e-8)
        em.set_maximum_steps(25)
    if changed("covariance"):
        em.set_covariance_type(spec["covariance"])
    if changed("initialisations"):
        em.set_number_initialisations(spec["initialisations"])
    if changed("ridge"):
        em.set_covariance_regularisation(spec["ridge"])


def test_em_object_reused_across_fits():
    from cppyml import clustering as cl
    X1, X2 = _blobs(2000, 4, 1), _blobs(1501, 6, 2)
    w = np.random.default_rng(3).uniform(0.25, 3.0, len(X1))
    base = {"covariance": "full", "initialisations": 1, "ridge": DEFAULT_RIDGE, "data": X1, "weights": None}
    sequence = [("full", {}), ("tied", {"covariance": "tied"}), ("diag", {"covariance": "diag"}), ("full, weighted", {"weights": w}),
                ("full again", {}), ("three initialisations", {"initialisations": 3}), ("ridge 1e-3", {"ridge": 1e-3}),
                ("default ridge again", {}), ("another data block", {"data": X2})]
    used, have = cl.EM(3), None
    differing = []
    for i, (name, changes) in enumerate(sequence):
        spec = dict(base, **changes)
        seed = 100 + i
        _configure_em(used, spec, have)
        have = spec
        used.set_seed(seed)
        got = [used.fit(spec["data"], sample_weight=spec["weights"]), *_em_state(used, spec["data"])]
        fresh = cl.EM(3)
        _configure_em(fresh, spec)
        fresh.set_seed(seed)
        want = [fresh.fit(spec["data"], sample_weight=spec["weights"]), *_em_state(fresh, spec["data"])]
        assert len(got) == len(want)
        differing += ["%s [%d]" % (name, j) for j, (a, b) in enumerate(zip(got, want)) if not _same(a, b)]
    assert not differing, differing


def _kmeans_state(km, X):
    return [km.centroids, km.labels_array, km.inertia, km.steps_done, km.converged, *km.predict(X[:500], return_distances=True)]


def test_kmeans_object_reused_across_fits():
    from cppyml import clustering as cl
    X1, X2 = _blobs(2000, 4, 5), _blobs(1501, 6, 6)
    w = np.random.default_rng(7).uniform(0.25, 3.0, len(X1))
    sequence = [("unweighted", X1, None, None), ("weighted", X1, w, None), ("unweighted again", X1, None, None),
                ("another initialiser", X1, None, "KPP"), ("another data block", X2, None, "KPP")]
    used, have = cl.KMeans(4), None
    used.set_maximum_steps(50)
    differing = []
    for i, (name, X, weights, initialiser) in enumerate(sequence):
        seed = 200 + i
        if initialiser != have:
            used.set_centroids_initialiser(getattr(cl, initialiser)())
        have = initialiser
        used.set_seed(seed)
        got = [used.fit(X, sample_weight=weights), *_kmeans_state(used, X)]
        fresh = cl.KMeans(4)
        fresh.set_maximum_steps(50)
        if initialiser:
            fresh.set_centroids_initialiser(getattr(cl, initialiser)())
        fresh.set_seed(seed)
        want = [fresh.fit(X, sample_weight=weights), *_kmeans_state(fresh, X)]
        differing += ["%s [%d]" % (name, j) for j, (a, b) in enumerate(zip(got, want)) if not _same(a, b)]
    assert not differing, differing
