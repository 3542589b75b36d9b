"""Clustering algorithms -- same classes, methods, properties and argument conventions as the reference's
pybind11 module `cppyml.clustering` (cppyml/clustering.cpp:75-185), running on an MI355X through libmlhip.so.

Conventions kept from the reference:
  * `fit(data)` takes a float64 C-contiguous `N x d` array and refuses anything else with TypeError
    (`py::arg("data").noconvert()`, clustering.cpp:115,161);
  * `EM.means` is `d x K` (NOT transposed, clustering.cpp:126), `KMeans.centroids` is `K x d` (clustering.cpp:66-69,172);
  * `KMeans.labels` is a Python list (pybind11/stl.h conversion, clustering.cpp:173);
  * std::invalid_argument / std::domain_error surface as ValueError.
Extensions (not in the reference surface): `silhouette_samples`, `silhouette_score` (module level: exact silhouette values on the GPU,
for the labels of either model), `EM.number_parameters`, `EM.bic`, `EM.aic`, `EM.impute`, `EM.conditional_mean`, `EM.conditional_variance`, `EM.conditional_cdf`, `EM.conditional_quantile`, `EM.conditional_sample`, `EM.conditional_covariances`, `EM.sample`, `EM.score_samples`, `EM.score`, `EM.predict`, `EM.predict_proba`, `KMeans.predict`, `EM.labels`, `EM.converged`, `EM.steps_done`, `EM.responsibilities_rows`, `KMeans.converged`,
`KMeans.steps_done`, `KMeans.labels_array`, `FixedCentroids`, `FixedPointKPP`, `EM.fit(..., sample_weight=)`,
`KMeans.fit(..., sample_weight=)`, `EM.set_covariance_regularisation`, `EM.covariance_regularisation`, `EM.set_number_initialisations`,
`EM.number_initialisations`, `EM.best_initialisation`, `EM.initialisation_log_likelihoods`, `EM.initialisation_steps`,
`EM.initialisation_converged`.
"""
import ctypes as C
import math

import numpy as np

from .. import _lib

_l = _lib.lib
_check = _lib.check
_dp = _lib.dptr
_get = _lib._get


def _require_data(data):
    if not _lib._is_block(data):
        raise TypeError("fit(): incompatible function arguments. data must be a C-contiguous float64 array of shape (N, d)")
    return data


def _vector(x):
    return np.ascontiguousarray(x, dtype=np.float64).ravel()


def _created(create, *args):
    """The handle create(*args, &handle) makes."""
    h = C.c_void_p()
    _check(create(*args, C.byref(h)))
    return h


def _deleter(destroy):
    """A __del__ that frees self._h with the library's `destroy`, once."""
    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            destroy(h)
            self._h = None
    return __del__


class CentroidsInitialiser:
    """Abstract centroids initialiser."""

    def __init__(self, *args, **kwargs):
        raise TypeError(f"{type(self).__module__}.{type(self).__qualname__}: No constructor defined!")

    __del__ = _deleter(_l.mlpp_centroids_initialiser_destroy)

    def _run(self, data, number_components, seed=None):
        """Test hook: runs the initialiser on N x d data, returns K x d centroids."""
        data = _require_data(data)
        n, d = data.shape
        out = np.empty((number_components, d))
        _check(_l.mlpp_centroids_initialiser_run(self._h, _dp(data), n, d, number_components, seed is not None, seed or 0, _dp(out)))
        return out

    def _run_on_device(self, data, number_components, seed=None):
        """Test hook: the same through the path `fit` takes (data uploaded, the O(N) passes on the GPU)."""
        data = _require_data(data)
        n, d = data.shape
        out = np.empty((number_components, d))
        _check(_l.mlpp_centroids_initialiser_run_on_device(self._h, _dp(data), n, d, number_components, seed is not None, seed or 0, _dp(out)))
        return out


class ResponsibilitiesInitialiser:
    """Abstract responsibilities initialiser."""

    def __init__(self, *args, **kwargs):
        raise TypeError(f"{type(self).__module__}.{type(self).__qualname__}: No constructor defined!")

    __del__ = _deleter(_l.mlpp_responsibilities_initialiser_destroy)

    def _run(self, data, number_components, seed=None):
        data = _require_data(data)
        n, d = data.shape
        out = np.empty((n, number_components), order="F")
        _check(_l.mlpp_responsibilities_initialiser_run(self._h, _dp(data), n, d, number_components, seed is not None, seed or 0, _dp(out)))
        return out


class Forgy(CentroidsInitialiser):
    """Forgy initialisation algorithm."""

    def __init__(self):
        self._h = _created(_l.mlpp_forgy_create)


class RandomPartition(CentroidsInitialiser):
    """Random Partition initialisation algorithm."""

    def __init__(self):
        self._h = _created(_l.mlpp_random_partition_create)


class KPP(CentroidsInitialiser):
    """KMeans++ initialisation algorithm."""

    def __init__(self):
        self._h = _created(_l.mlpp_kpp_create)


class FixedPointKPP(CentroidsInitialiser):
    """Extension: K-means++ seeding from exact integer cumulative weights. Same D^2 distribution as KPP, different draws (KPP
    reproduces the reference's draws bit for bit); on the GPU every draw stays on the device, whatever the sample size."""

    def __init__(self):
        self._h = _created(_l.mlpp_fixed_point_kpp_create)


class FixedCentroids(CentroidsInitialiser):
    """Extension: returns the given centroids (K x d)."""

    def __init__(self, centroids):
        c = np.ascontiguousarray(centroids, dtype=np.float64)
        if c.ndim != 2:
            raise ValueError("centroids must be K x d")
        self._h = _created(_l.mlpp_fixed_centroids_create, _dp(c), c.shape[0], c.shape[1])


class ClosestCentroid(ResponsibilitiesInitialiser):
    """Assigns points to closest centroid."""

    def __init__(self, centroids_initialiser):
        if centroids_initialiser is not None and not isinstance(centroids_initialiser, CentroidsInitialiser):
            raise TypeError("centroids_initialiser must be a CentroidsInitialiser")
        self._ci = centroids_initialiser
        self._h = _created(_l.mlpp_closest_centroid_create, centroids_initialiser._h if centroids_initialiser is not None else None)


class EM:
    """Gaussian Expectation-Maximisation algorithm."""

    def __init__(self, number_components):
        self._h = _created(_l.mlpp_em_create, int(number_components))
        self._keep = []

    __del__ = _deleter(_l.mlpp_em_destroy)

    def set_seed(self, seed):
        """Sets PRNG seed."""
        _check(_l.mlpp_em_set_seed(self._h, seed))

    def set_absolute_tolerance(self, absolute_tolerance):
        """Sets absolute tolerance."""
        _check(_l.mlpp_em_set_absolute_tolerance(self._h, absolute_tolerance))

    def set_relative_tolerance(self, relative_tolerance):
        """Sets relative tolerance."""
        _check(_l.mlpp_em_set_relative_tolerance(self._h, relative_tolerance))

    def set_maximum_steps(self, maximum_steps):
        """Sets maximum number of iterations."""
        _check(_l.mlpp_em_set_maximum_steps(self._h, maximum_steps))

    def set_means_initialiser(self, means_initialiser):
        """Sets the algorithm to initialise component means."""
        _check(_l.mlpp_em_set_means_initialiser(self._h, means_initialiser._h if means_initialiser is not None else None))
        self._keep.append(means_initialiser)

    def set_responsibilities_initialiser(self, responsibilities_initialiser):
        """Sets the algorithm to initialise responsibilities for data points."""
        _check(_l.mlpp_em_set_responsibilities_initialiser(
            self._h, responsibilities_initialiser._h if responsibilities_initialiser is not None else None))
        self._keep.append(responsibilities_initialiser)

    def set_verbose(self, verbose):
        """Turns on/off the verbose mode."""
        _check(_l.mlpp_em_set_verbose(self._h, bool(verbose)))

    def set_maximise_first(self, maximise_first):
        """Turns on/off doing an initial maximisation step before the E-M iterations."""
        _check(_l.mlpp_em_set_maximise_first(self._h, bool(maximise_first)))

    def set_covariance_type(self, covariance_type):
        """Extension (not in the reference surface): "full" (default, the reference's only mode), "diag" -- every
        covariance restricted to its diagonal; `covariance(k)` then returns a diagonal matrix -- or "tied" -- one covariance
        shared by all components (scikit-learn's 'tied'); `covariance(k)` then returns the same matrix for every k. One fused
        kernel per iteration for d <= 32, K <= 64 (tied: unweighted fits); other shapes run the full-covariance kernels."""
        codes = {"full": 0, "diag": 1, "tied": 2}
        if covariance_type not in codes:
            raise ValueError("covariance_type must be 'full', 'diag' or 'tied'")
        _check(_l.mlpp_em_set_covariance_type(self._h, codes[covariance_type]))

    def set_covariance_regularisation(self, covariance_regularisation):
        """Extension (scikit-learn's `reg_covar`): the value every M-step of the next fit adds to the diagonal of each covariance
        it forms ("full": every component's; "diag": every variance; "tied": the one covariance, once). Default 1e-15, the
        reference's constant; 0 is allowed. ValueError for a negative or non-finite value (the model keeps its value)."""
        _check(_l.mlpp_em_set_covariance_regularisation(self._h, covariance_regularisation))

    @property
    def covariance_regularisation(self):
        """Extension: the value set by `set_covariance_regularisation` (1e-15 unless set)."""
        return _get(_l.mlpp_em_covariance_regularisation, self._h, C.c_double)

    def set_number_initialisations(self, number_initialisations):
        """Extension (scikit-learn's `n_init`; the reference's EM has no restarts): `fit` runs this many EM loops on the one
        uploaded sample and keeps the best. Start r is what a solo fit would begin from, drawn from the seeded PRNG in order -- the
        starts of that many consecutive `fit` calls on one object after one `set_seed`. Among the loops that converged the greatest
        log-likelihood wins, the first of equals; if none converged, the same over all. Default 1. ValueError for 0."""
        _check(_l.mlpp_em_set_number_initialisations(self._h, number_initialisations))

    @property
    def number_initialisations(self):
        """Extension: the value set by `set_number_initialisations` (1 unless set)."""
        return _get(_l.mlpp_em_number_initialisations, self._h, C.c_uint32)

    @property
    def best_initialisation(self):
        """Extension: the initialisation the fitted state (parameters, log-likelihood, labels, responsibilities) belongs to."""
        return _get(_l.mlpp_em_best_initialisation, self._h, C.c_uint32)

    def _per_initialisation(self, getter, dtype, ctype):
        count = C.c_uint32()
        _check(getter(self._h, None, 0, C.byref(count)))
        out = np.empty(count.value, dtype=dtype)
        if count.value:
            _check(getter(self._h, out.ctypes.data_as(C.POINTER(ctype)), count, C.byref(count)))
        return out

    @property
    def initialisation_log_likelihoods(self):
        """Extension: the final log-likelihood of every initialisation of the last fit, in order."""
        return self._per_initialisation(_l.mlpp_em_initialisation_log_likelihoods, np.float64, C.c_double)

    @property
    def initialisation_steps(self):
        """Extension: the iterations every initialisation of the last fit ran."""
        return self._per_initialisation(_l.mlpp_em_initialisation_steps, np.uint32, C.c_uint32)

    @property
    def initialisation_converged(self):
        """Extension: whether each initialisation of the last fit converged (bool array)."""
        return self._per_initialisation(_l.mlpp_em_initialisation_converged, np.int32, C.c_int).astype(bool)

    def fit(self, data, sample_weight=None):
        """Fits the components to the data (2D array with data points in rows). Returns True if EM converged.

        Extension: `sample_weight`, a 1-D C-contiguous float64 array with one frequency weight >= 0 per row (integer weights: the
        fit of the data with row i repeated sample_weight[i] times, without the copies). TypeError for another type or dtype,
        ValueError for a wrong length, a negative or non-finite weight or a total that is not positive. The log-likelihood and
        every M-step are weighted; `responsibilities` and `labels` stay per row; initialisers see rows, not weights."""
        data = _require_data(data)
        n, d = data.shape
        conv = C.c_int()
        if sample_weight is None:
            _check(_l.mlpp_em_fit(self._h, _dp(data), n, d, C.byref(conv)))
        else:
            w = _lib.require_weights(sample_weight, n)
            _check(_l.mlpp_em_fit_weighted(self._h, _dp(data), _dp(w), n, d, C.byref(conv)))
        return bool(conv.value)

    def _dims(self):
        d, n = C.c_uint32(), C.c_uint64()
        _check(_l.mlpp_em_dims(self._h, C.byref(d), C.byref(n)))
        return d.value, n.value

    @property
    def number_components(self):
        """Number of Gaussian components."""
        return _get(_l.mlpp_em_number_components, self._h, C.c_uint32)

    @property
    def means(self):
        """Fitted means (d x K)."""
        d, _ = self._dims()
        out = np.empty((d, self.number_components), order="F")
        _check(_l.mlpp_em_means(self._h, _dp(out)))
        return out

    @property
    def responsibilities(self):
        """Fitted responsibilities (N x K)."""
        _, n = self._dims()
        out = np.empty((n, self.number_components), order="F")
        _check(_l.mlpp_em_responsibilities(self._h, _dp(out)))
        return out

    def responsibilities_rows(self, first_row, number_rows):
        """Extension: rows [first_row, first_row + number_rows) of `responsibilities` without fetching the whole N x K block
        from the device (5 GB at N=10M, K=64)."""
        out = np.empty((int(number_rows), self.number_components), order="F")
        _check(_l.mlpp_em_responsibilities_rows(self._h, int(first_row), int(number_rows), _dp(out)))
        return out

    @property
    def log_likelihood(self):
        """Maximised log-likelihood."""
        return _get(_l.mlpp_em_log_likelihood, self._h, C.c_double)

    @property
    def mixing_probabilities(self):
        """Mixing probabilities of components."""
        out = np.empty(self.number_components)
        _check(_l.mlpp_em_mixing_probabilities(self._h, _dp(out)))
        return out

    def covariance(self, k):
        """Returns k-th covariance matrix."""
        d, _ = self._dims()
        out = np.empty((d, d), order="F")
        _check(_l.mlpp_em_covariance(self._h, int(k), _dp(out)))
        return out

    def assign_responsibilities(self, x):
        """Given a data point x, calculate each component's responsibilities for x and return them."""
        x = _vector(x)
        u = np.empty(self.number_components)
        _check(_l.mlpp_em_assign_responsibilities(self._h, _dp(x), x.size, _dp(u), u.size))
        return u

    # ---- extensions ----
    def score_samples(self, X):
        """Extension: log-density of every row of X (N x d, what `fit` takes) under the fitted mixture, on the GPU."""
        X = _require_data(X)
        n, d = X.shape
        out = np.empty(n)
        _check(_l.mlpp_em_score_samples(self._h, _dp(X), n, d, _dp(out)))
        return out

    def score(self, X):
        """Extension: mean of score_samples(X), summed sequentially in row order (comparable with `log_likelihood`); NaN for
        an empty X, like the C++ `mean_log_density`."""
        v = self.score_samples(X)
        if not len(v):
            return float("nan")
        total = 0.0
        for x in v.tolist():
            total += x
        return total / len(v)

    def predict(self, X):
        """Extension: component of the largest log-responsibility for every row of X (first maximum wins), uint32 array."""
        X = _require_data(X)
        n, d = X.shape
        out = np.empty(n, dtype=np.uint32)
        _check(_l.mlpp_em_predict(self._h, _dp(X), n, d, _lib.u32ptr(out)))
        return out

    def predict_proba(self, X):
        """Extension: posterior component probabilities of every row of X (N x K, Fortran order like `responsibilities`)."""
        X = _require_data(X)
        n, d = X.shape
        out = np.empty((n, self.number_components), order="F")
        _check(_l.mlpp_em_predict_proba(self._h, _dp(X), n, d, _dp(out)))
        return out

    def sample(self, n_samples, seed=0):
        """Extension (scikit-learn's GaussianMixture.sample): n_samples points drawn from the fitted mixture on the GPU. Returns
        (X, labels): X (n_samples, d) C-contiguous float64 -- what `fit` takes --, labels the uint32 component of every row. Row i is
        a pure function of (seed, i) and the fitted parameters: one seed gives one sample, a longer draw starts with the shorter
        one. The model's own random engine is not touched. ValueError for a negative n_samples or a model that was not fitted."""
        n = int(n_samples)
        if n < 0:
            raise ValueError("sample(): n_samples must not be negative")
        d, _ = self._dims()
        X, labels = np.empty((n, d)), np.empty(n, dtype=np.uint32)
        _check(_l.mlpp_em_sample(self._h, n, int(seed), _dp(X), _lib.u32ptr(labels)))
        return X, labels

    def _observed(self, observed, name):
        """The checks of `observed` that conditional_mean, conditional_variance, conditional_cdf, conditional_quantile, conditional_sample and conditional_covariances share -> (coordinates, d)."""
        try:
            coordinates = [int(c) for c in observed]
        except TypeError:
            raise TypeError(name + "(): observed must be a sequence of coordinate indices") from None
        if any(c != o for c, o in zip(coordinates, observed)):
            raise TypeError(name + "(): observed must hold integers")
        d, _ = self._dims()
        if d == 0:
            raise ValueError(name + "(): the model has not been fitted")
        if not 1 <= len(coordinates) <= d - 1:
            raise ValueError(name + "(): between 1 and d - 1 coordinates must be observed")
        if min(coordinates) < 0 or max(coordinates) >= d:
            raise ValueError(name + "(): observed coordinate out of range")
        if len(set(coordinates)) != len(coordinates):
            raise ValueError(name + "(): observed coordinate given twice")
        return coordinates, d

    def conditional_mean(self, X_observed, observed, return_log_density=False):
        """Extension (Gaussian-mixture regression, imputation): E[x_M | x_O] under the fitted mixture for every row of X_observed, on
        the GPU. `observed`: distinct coordinate indices in any order, at least one and not all of them; column c of X_observed
        (N x len(observed), C-contiguous float64 like what `fit` takes) holds coordinate observed[c]. Returns an (N, d - len(observed))
        C-contiguous float64 array, the missing coordinates in ascending order -- with return_log_density=True a pair of it and the N
        log-densities of the rows under the marginal mixture. TypeError / ValueError before any device work."""
        X = _require_data(X_observed)
        coordinates, d = self._observed(observed, "conditional_mean")
        n, columns = X.shape
        if columns != len(coordinates):
            raise ValueError("conditional_mean(): X_observed must have one column per observed coordinate")
        index = np.array(coordinates, dtype=np.uint32)
        out = np.empty((n, d - len(coordinates)))
        dens = np.empty(n) if return_log_density else None
        _check(_l.mlpp_em_conditional_means(self._h, _lib.u32ptr(index), len(index), _dp(X), n, _dp(out), _dp(dens)))
        return _lib._with_optional(out, dens)

    def impute(self, X, return_log_density=False, return_responsibilities=False):
        """Extension (imputation of a table with gaps): a copy of X (N x d, C-contiguous float64 like what `fit` takes) in which every
        NaN is replaced by E[x_j | the coordinates that row has] under the fitted mixture, on the GPU. Every row has its own pattern
        of NaNs; observed entries keep their bits, a complete row comes back as it is, a row of all NaN as the mixture's mean. With
        return_log_density=True and / or return_responsibilities=True a tuple of the array, the N log-densities of the rows' observed
        coordinates under the marginal mixture, and the (N, K) C-contiguous posterior memberships given what each row has -- what
        predict_proba cannot give for an incomplete row --, in that order. A row's results do not depend on the other rows or their
        order. TypeError / ValueError before any device work."""
        X = _require_data(X)
        d, _ = self._dims()
        if d == 0:
            raise ValueError("impute(): the model has not been fitted")
        n, columns = X.shape
        if columns != d:
            raise ValueError("impute(): X must have one column per coordinate of the model")
        out = np.empty((n, d))
        dens = np.empty(n) if return_log_density else None
        resp = np.empty((n, self.number_components)) if return_responsibilities else None
        _check(_l.mlpp_em_impute(self._h, _dp(X), n, d, _dp(out), _dp(dens), _dp(resp)))
        return _lib._with_optional(out, dens, resp)

    def conditional_variance(self, X_observed, observed, covariance=False, return_mean=False):
        """Extension (error bars on an imputed value, heteroscedastic regression bands): the predictive variance Var[x_M | x_O] under
        the fitted mixture for every row of X_observed, on the GPU: sum_k r_k (Sigma_k,M|O + (t_k - y)(t_k - y)^T) with y =
        conditional_mean. X_observed and `observed` as for conditional_mean. Returns an (N, d - len(observed)) C-contiguous float64
        array, the missing coordinates in ascending order -- with covariance=True the (N, dM, dM) symmetric matrices, whose diagonal
        has the bits of the default form; with return_mean=True a pair of that and conditional_mean's (N, dM) result, bit for bit.
        TypeError / ValueError before any device work."""
        X = _require_data(X_observed)
        coordinates, d = self._observed(observed, "conditional_variance")
        n, columns = X.shape
        if columns != len(coordinates):
            raise ValueError("conditional_variance(): X_observed must have one column per observed coordinate")
        index = np.array(coordinates, dtype=np.uint32)
        dM = d - len(coordinates)
        out = np.empty((n, dM, dM) if covariance else (n, dM))
        mean = np.empty((n, dM)) if return_mean else None
        _check(_l.mlpp_em_conditional_variances(self._h, _lib.u32ptr(index), len(index), _dp(X), n, bool(covariance), _dp(out), _dp(mean)))
        return _lib._with_optional(out, mean)

    def conditional_cdf(self, X_observed, observed, values):
        """Extension (exceedance probabilities, the probability integral transform, p-values of an observed value): the predictive
        CDF P(x_j <= values[i, j] | x_O) of every missing coordinate under the fitted mixture for every row of X_observed, on the
        GPU. Given x_O, coordinate j follows the one-dimensional mixture sum_k r_k N(t_kj, Sigma_k,M|O[j][j]). X_observed and
        `observed` as for conditional_mean; `values`: a C-contiguous float64 (N, d - len(observed)) array, the missing coordinates in
        ascending order. Returns an array of that shape. TypeError / ValueError before any device work."""
        X = _require_data(X_observed)
        coordinates, d = self._observed(observed, "conditional_cdf")
        n, columns = X.shape
        if columns != len(coordinates):
            raise ValueError("conditional_cdf(): X_observed must have one column per observed coordinate")
        dM = d - len(coordinates)
        if not (isinstance(values, np.ndarray) and values.dtype == np.float64 and values.ndim == 2 and values.flags.c_contiguous):
            raise TypeError("conditional_cdf(): values must be a C-contiguous float64 array of shape (N, dM)")
        if values.shape != (n, dM):
            raise ValueError("conditional_cdf(): values must have one row per row of X_observed and one column per missing coordinate")
        index = np.array(coordinates, dtype=np.uint32)
        out = np.empty((n, dM))
        _check(_l.mlpp_em_conditional_cdfs(self._h, _lib.u32ptr(index), len(index), _dp(X), n, _dp(values), _dp(out)))
        return out

    def conditional_quantile(self, X_observed, observed, probabilities):
        """Extension (exact predictive intervals and medians): the quantiles of x_j | x_O, the inverse of conditional_cdf, for every
        row of X_observed at every probability, on the GPU -- exact where mean +- z sqrt(variance) is wrong (a mixture's conditional
        is skewed or multimodal) and without the 1 / sqrt(n_draws) error of quantiles taken from conditional_sample draws.
        `probabilities`: a 1-D sequence of floats strictly inside (0, 1). Returns a (len(probabilities), N, d - len(observed))
        C-contiguous float64 array, the missing coordinates in ascending order. A pure function of the row, the parameters and the
        probability. TypeError / ValueError before any device work."""
        X = _require_data(X_observed)
        coordinates, d = self._observed(observed, "conditional_quantile")
        n, columns = X.shape
        if columns != len(coordinates):
            raise ValueError("conditional_quantile(): X_observed must have one column per observed coordinate")
        try:
            p = np.array([float(q) for q in probabilities], dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("conditional_quantile(): probabilities must be a 1-D sequence of floats") from None
        if not np.all((p > 0.0) & (p < 1.0)):
            raise ValueError("conditional_quantile(): every probability must lie strictly inside (0, 1)")
        index = np.array(coordinates, dtype=np.uint32)
        out = np.empty((len(p), n, d - len(coordinates)))
        _check(_l.mlpp_em_conditional_quantiles(self._h, _lib.u32ptr(index), len(index), _dp(X), n, _dp(p), len(p), _dp(out)))
        return out

    def conditional_covariances(self, observed):
        """Extension: the covariances of the conditioned components, Sigma_k,M|O = Sigma_k,MM - Sigma_k,MO Sigma_k,OO^-1 Sigma_k,OM, as a
        (K, dM, dM) float64 array, the missing coordinates in ascending order. `observed` as for conditional_mean. Host only: no GPU."""
        coordinates, d = self._observed(observed, "conditional_covariances")
        index = np.array(coordinates, dtype=np.uint32)
        dM = d - len(coordinates)
        out = np.empty((self.number_components, dM, dM))
        _check(_l.mlpp_em_conditional_covariances(self._h, _lib.u32ptr(index), len(index), _dp(out)))
        return out

    def conditional_sample(self, X_observed, observed, n_draws=1, seed=0, return_labels=False):
        """Extension (multiple imputation, predictive intervals): n_draws draws from p(x_M | x_O) under the fitted mixture for every
        row of X_observed, on the GPU. X_observed and `observed` as for conditional_mean. Returns an (n_draws, N, d - len(observed))
        C-contiguous float64 array, the missing coordinates in ascending order -- with return_labels=True a pair of it and the
        (n_draws, N) uint32 components the rows were drawn from. Draw q of row i is a pure function of (seed, i, q), the row and the
        parameters; a seed shared with `sample` shares no random number with it, and the model's own random engine is not touched.
        TypeError / ValueError before any device work."""
        X = _require_data(X_observed)
        coordinates, d = self._observed(observed, "conditional_sample")
        n, columns = X.shape
        if columns != len(coordinates):
            raise ValueError("conditional_sample(): X_observed must have one column per observed coordinate")
        if isinstance(n_draws, bool) or not isinstance(n_draws, (int, np.integer)):
            raise TypeError("conditional_sample(): n_draws must be an integer")
        if n_draws < 0 or n_draws > 2 ** 32 - 1:
            raise ValueError("conditional_sample(): n_draws must lie in 0 .. 2^32 - 1")
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
            raise TypeError("conditional_sample(): seed must be an integer")
        if not 0 <= seed < 2 ** 64:
            raise ValueError("conditional_sample(): seed must lie in 0 .. 2^64 - 1")
        index = np.array(coordinates, dtype=np.uint32)
        out = np.empty((int(n_draws), n, d - len(coordinates)))
        labels = np.empty((int(n_draws), n), dtype=np.uint32) if return_labels else None
        _check(_l.mlpp_em_conditional_samples(self._h, _lib.u32ptr(index), len(index), _dp(X), n, int(n_draws), int(seed), _dp(out),
                                              _lib.u32ptr(labels)))
        return _lib._with_optional(out, labels)

    @property
    def labels(self):
        _, n = self._dims()
        out = np.empty(n, dtype=np.uint32)
        _check(_l.mlpp_em_labels(self._h, _lib.u32ptr(out)))
        return out

    @property
    def converged(self):
        return bool(_get(_l.mlpp_em_converged, self._h, C.c_int))

    @property
    def steps_done(self):
        return _get(_l.mlpp_em_steps_done, self._h, C.c_uint32)

    @property
    def number_parameters(self):
        """Extension (model selection; scikit-learn's `_n_parameters`): the free parameters of the fitted mixture in the covariance
        mode it was fitted in -- full K d (d + 1) / 2, diag K d, tied d (d + 1) / 2, each plus K d + K - 1. No GPU needed.
        ValueError for a model that was not fitted."""
        return _get(_l.mlpp_em_number_parameters, self._h, C.c_uint64)

    def bic(self, X):
        """Extension: the Bayesian information criterion of the fitted model on X (N x d, what `fit` takes), as scikit-learn defines
        it: -2 N score(X) + number_parameters log N (lower is better). Runs the scoring pass of score_samples."""
        n = len(_require_data(X))
        p = self.number_parameters
        return -2.0 * n * self.score(X) + p * math.log(n) if n else float("nan")

    def aic(self, X):
        """Extension: the Akaike information criterion on X: -2 N score(X) + 2 number_parameters."""
        n = len(_require_data(X))
        p = self.number_parameters
        return -2.0 * n * self.score(X) + 2.0 * p


def silhouette_samples(X, labels, rows=None):
    """Extension (scikit-learn's silhouette_samples): the exact silhouette value of every row of X (N x d, what `fit` takes) under
    `labels`, Euclidean distance, computed on the GPU -- or of the rows listed in `rows` (any order, repeats allowed), each scored
    against ALL N rows. Returns float64 values, N or len(rows) of them. labels: a 1-D integer array or a list (`KMeans.labels`,
    `EM.labels` go straight in), K = max + 1; a label no row carries is ignored; a row alone in its cluster scores 0.
    s = (b - a) / max(a, b) with a the mean distance to the other rows of the own cluster and b the smallest mean distance to
    another cluster. The distances are formed directly, sqrt(sum (x - y)^2), never from |x|^2 + |y|^2 - 2 x.y, so data far from the
    origin lose no accuracy; the order of every sum is fixed (include/mlhip.h, mlhip_silhouette).
    TypeError / ValueError before any device work: X or labels of a wrong type, a wrong number of labels, a negative label, fewer
    than two clusters, a row index outside [0, N)."""
    X = _require_data(X)
    n, d = X.shape
    labels, K, rows = _lib.silhouette_arguments(n, labels, rows)
    out = np.empty(n if rows is None else len(rows))
    _check(_l.mlpp_silhouette_samples(_dp(X), n, d, _lib.u32ptr(labels), K, None if rows is None else rows.ctypes.data_as(C.POINTER(C.c_uint64)),
                                      0 if rows is None else len(rows), _dp(out)))
    return out


def silhouette_score(X, labels, sample_size=None, seed=0):
    """Extension (scikit-learn's silhouette_score): the mean of silhouette_samples, summed sequentially in row order. With
    sample_size = m the rows are np.sort(np.random.default_rng(seed).choice(N, m, replace=False)) and those m rows are scored
    against ALL N rows: exact silhouette values of a subsample. (scikit-learn scores the subsample against ITSELF, an estimate
    from m^2 pairs; here the m values are the ones the full computation gives.) ValueError for a sample_size outside 1 .. N."""
    X = _require_data(X)
    n = len(X)
    rows = None
    if sample_size is not None:
        m = int(sample_size)
        if not 1 <= m <= n:
            raise ValueError("silhouette_score(): sample_size must lie in 1 .. N")
        _lib.silhouette_arguments(n, labels)
        rows = np.sort(np.random.default_rng(seed).choice(n, m, replace=False))
    total = 0.0
    values = silhouette_samples(X, labels, rows)
    for v in values.tolist():
        total += v
    return total / len(values)


class KMeans:
    """Naive K-Means algorithm."""

    def __init__(self, number_clusters):
        self._h = _created(_l.mlpp_kmeans_create, int(number_clusters))
        self._keep = []

    __del__ = _deleter(_l.mlpp_kmeans_destroy)

    def set_seed(self, seed):
        """Sets the PRNG seed."""
        _check(_l.mlpp_kmeans_set_seed(self._h, seed))

    def set_absolute_tolerance(self, absolute_tolerance):
        """Sets absolute tolerance."""
        _check(_l.mlpp_kmeans_set_absolute_tolerance(self._h, absolute_tolerance))

    def set_maximum_steps(self, maximum_steps):
        """Sets maximum number of iterations."""
        _check(_l.mlpp_kmeans_set_maximum_steps(self._h, maximum_steps))

    def set_centroids_initialiser(self, centroids_initialiser):
        """Sets the algorithm to initialise cluster centroids."""
        _check(_l.mlpp_kmeans_set_centroids_initialiser(
            self._h, centroids_initialiser._h if centroids_initialiser is not None else None))
        self._keep.append(centroids_initialiser)

    def set_number_initialisations(self, centroids_initialiser):
        """Sets number of initialisations to try, to find the clusters with lowest inertia.
        (The keyword really is `centroids_initialiser` in the reference: cppyml/clustering.cpp:159.)"""
        _check(_l.mlpp_kmeans_set_number_initialisations(self._h, centroids_initialiser))

    def set_verbose(self, verbose):
        """Turns on/off the verbose mode."""
        _check(_l.mlpp_kmeans_set_verbose(self._h, bool(verbose)))

    def fit(self, data, sample_weight=None):
        """Fits the clusters to the data (2D array with data points in rows). Returns True if the algorithm converged.

        Extension: `sample_weight`, a 1-D C-contiguous float64 array with one frequency weight >= 0 per row (integer weights: the
        fit of the data with row i repeated sample_weight[i] times, without the copies). TypeError for another type or dtype,
        ValueError for a wrong length, a negative or non-finite weight or a total that is not positive -- all before any device
        work. Centroids are weighted means (a cluster of total weight 0 goes to the origin), `inertia` is sum_i w_i dist_i;
        `labels` stay per row; initialisers see rows, not weights."""
        data = _require_data(data)
        n, d = data.shape
        conv = C.c_int()
        if sample_weight is None:
            _check(_l.mlpp_kmeans_fit(self._h, _dp(data), n, d, C.byref(conv)))
        else:
            w = _lib.require_weights(sample_weight, n)
            _check(_l.mlpp_kmeans_fit_weighted(self._h, _dp(data), _dp(w), n, d, C.byref(conv)))
        return bool(conv.value)

    def _dims(self):
        d, n = C.c_uint32(), C.c_uint64()
        _check(_l.mlpp_kmeans_dims(self._h, C.byref(d), C.byref(n)))
        return d.value, n.value

    @property
    def number_clusters(self):
        """Number of clusters."""
        return _get(_l.mlpp_kmeans_number_clusters, self._h, C.c_uint32)

    @property
    def centroids(self):
        """Fitted centroids (K x d)."""
        d, _ = self._dims()
        out = np.empty((self.number_clusters, d))
        _check(_l.mlpp_kmeans_centroids(self._h, _dp(out)))
        return out

    @property
    def labels(self):
        """Fitted labels."""
        _, n = self._dims()
        out = np.empty(n, dtype=np.uint32)
        _check(_l.mlpp_kmeans_labels(self._h, _lib.u32ptr(out)))
        return out.tolist()

    @property
    def labels_array(self):
        """Extension: the fitted labels as a numpy uint32 array (the reference surface converts to a Python list, which
        costs seconds and gigabytes at N = 1e8)."""
        _, n = self._dims()
        out = np.empty(n, dtype=np.uint32)
        _check(_l.mlpp_kmeans_labels(self._h, _lib.u32ptr(out)))
        return out

    @property
    def inertia(self):
        """Minimised inertia."""
        return _get(_l.mlpp_kmeans_inertia, self._h, C.c_double)

    def assign_label(self, x):
        """Given a data point x, assigns it to the closest cluster: (label, squared distance)."""
        x = _vector(x)
        label, dist = C.c_uint32(), C.c_double()
        _check(_l.mlpp_kmeans_assign_label(self._h, _dp(x), x.size, C.byref(label), C.byref(dist)))
        return label.value, dist.value

    # ---- extensions ----
    def predict(self, X, return_distances=False):
        """Extension: `assign_label` for every row of X on the GPU: uint32 labels, and with return_distances=True also the
        squared distance of every row to its centroid."""
        X = _require_data(X)
        n, d = X.shape
        labels = np.empty(n, dtype=np.uint32)
        dist = np.empty(n) if return_distances else None
        _check(_l.mlpp_kmeans_predict(self._h, _dp(X), n, d, _lib.u32ptr(labels), _dp(dist)))
        return _lib._with_optional(labels, dist)

    @property
    def converged(self):
        return bool(_get(_l.mlpp_kmeans_converged, self._h, C.c_int))

    @property
    def steps_done(self):
        return _get(_l.mlpp_kmeans_steps_done, self._h, C.c_uint32)
