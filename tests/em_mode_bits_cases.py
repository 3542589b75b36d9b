"""EM in its three covariance modes against its own recorded bits: the cases and the runner shared by
tests/test_gpu_em_mode_bits.py and tests/golden/make_em_mode_bits_golden.py. The per-step, loop, restarts and scoring entry points are
called through ml_amd._lib, the facade through ml_amd.cppyml.EM.

Every sample is a seeded normal mixture (not on a grid) of at most 9000 rows, so every grid is set by n, not by the number of compute
units, and the start parameters are exact small numbers (no BLAS product decides them). The fixture holds, per case, what each call
returned; arrays of more than 1024 elements are recorded as the CRC-32 of their bytes. Every case reports the differences between
the route it means to exercise and the route the library reports."""
import contextlib
import os
import tempfile
import zlib

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "em_mode_bits.npz")

DIAG_KERNEL = (3, 2, 777)        # the one-kernel diagonal route
DIAG_FALLBACK = (40, 3, 1000)    # d > 32: the full-covariance kernels, the diagonal taken on the host
TIED = (5, 3, 1500)
FULL = (4, 3, 2000)
FACADE = (3, 3, 2000)
FACADE_SEED = 20241
VERBOSE_SEED = {"diag": 5, "tied": 4}     # seeds whose best initialisation of 3 is not the last one (the generator asserts it)


def make_inputs(d, K, n):
    """A seeded normal mixture and a start: uniform mixing, K rows of X as means, one positive definite matrix per component."""
    rng = np.random.default_rng(7919 * d + 101 * K + n)
    centres = 4.0 * rng.standard_normal((K, d))
    X = np.ascontiguousarray(centres[rng.integers(0, K, size=n)] + rng.standard_normal((n, d)))
    w = np.exp(rng.standard_normal(n))
    mu0 = X[rng.permutation(n)[:K]].copy()
    off = 1.0 - np.eye(d)
    full = np.stack([(2.0 + k) * np.eye(d) + 0.25 * off for k in range(K)])
    return X, w, np.full(K, 1.0 / K), mu0, full


def mode_covariance(full, mode):
    """The start covariances in the array form of `mode`: K x d x d, K x d variances, or the one d x d matrix."""
    if mode == "diag":
        return np.ascontiguousarray(np.stack([np.diag(m) for m in full]))
    return full[0].copy() if mode == "tied" else full


def restart_starts(X, K, R, mode, full):
    rng = np.random.default_rng(len(X) + R)
    mu0 = np.stack([X[rng.permutation(len(X))[:K]] for _ in range(R)])
    return np.full((R, K), 1.0 / K), mu0, np.stack([mode_covariance(full, mode)] * R)


@contextlib.contextmanager
def switches(env):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@contextlib.contextmanager
def captured_stdout(into):
    """File descriptor 1 into a temporary file for the block (the facade's verbose lines come from C++); into['out'] = the bytes."""
    import sys
    sys.stdout.flush()
    saved = os.dup(1)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 1)
        try:
            yield
        finally:
            sys.stdout.flush()
            os.dup2(saved, 1)
            os.close(saved)
            f.seek(0)
            into["out"] = f.read()


def _crc(a):
    return np.uint32(zlib.crc32(np.ascontiguousarray(a).tobytes()))


def _pin(a):
    a = np.ascontiguousarray(a)
    return a if a.size <= 1024 else _crc(a)


def _kind(mode):
    return {"full": {}, "diag": {"diagonal": True}, "tied": {"tied": True}}[mode]


def _route_mismatch(dt, K, mode, expected):
    """{query: (reported, expected)} for every expected entry the library reports differently. expected: 'tied' -> the tied route,
    'restarts' -> (R, kind), 'score' -> the scoring kernel, every other key a field of em_route(K, mode)."""
    wrong = {}
    for key, want in expected.items():
        if key == "tied":
            got = dt.em_tied_route(K)
        elif key == "restarts":
            got, want = dt.em_restarts_route(K, want[0], mode)[0], want[1]
        elif key == "score":
            got = dt.em_score_route(K)
        else:
            got = dt.em_route(K, "diag" if mode == "diag" else "full")[key]
        if got != want:
            wrong[key] = (got, want)
    return wrong


def _left_behind(dt, K, out, tag):
    """What the call left on the handle: the labels and the first 64 rows of the responsibilities (the E-step records of the
    mode, expanded to full covariances where the per-row kernels need them)."""
    out[tag + "/labels_crc"] = _crc(dt.em_labels(K))
    out[tag + "/responsibilities"] = _pin(dt.em_responsibilities_rows(K, 0, 64))


def _put_step(out, tag, result):
    ll, pi, mu, cov = result
    out[tag + "/log_likelihood"] = np.float64(ll)
    out[tag + "/mixing"], out[tag + "/means"], out[tag + "/covariances"] = _pin(pi), _pin(mu), _pin(cov)


def _put_loop(out, tag, result):
    steps, converged, ll, pi, mu, cov, history = result
    out[tag + "/steps"], out[tag + "/converged"], out[tag + "/log_likelihood"] = np.uint32(steps), np.bool_(converged), np.float64(ll)
    out[tag + "/mixing"], out[tag + "/means"], out[tag + "/covariances"] = _pin(pi), _pin(mu), _pin(cov)
    out[tag + "/history"] = _pin(history)


# (name, mode, (d, K, n), environment switches, weighted, expected route): two steps of the mode's per-step entry point
STEP_CASES = [
    ("step_diag_kernel", "diag", DIAG_KERNEL, {}, False, {"diag_kernel": True}),
    ("step_diag_fallback", "diag", DIAG_FALLBACK, {}, False, {"diag_kernel": False}),
    ("step_tied_kernel", "tied", TIED, {"MLHIP_TIED": "kernel"}, False, {"tied": "kernel"}),
    ("step_tied_composed", "tied", TIED, {"MLHIP_TIED": "composed"}, False, {"tied": "composed"}),
    ("step_tied_weighted", "tied", TIED, {}, True, {"tied": "composed"}),
]

# (name, mode, shape, switches, device ids of a group or None, expected route): em_iterate, 30 steps, atol = rtol = 1e-10
ITERATE_CASES = [
    ("iterate_full", "full", FULL, {}, None, {"diag_kernel": False, "device_close": True}),
    ("iterate_diag_kernel", "diag", DIAG_KERNEL, {}, None, {"diag_kernel": True, "device_close": True}),
    ("iterate_diag_fallback", "diag", DIAG_FALLBACK, {}, None, {"diag_kernel": False, "device_close": False}),
    ("iterate_tied_kernel", "tied", TIED, {"MLHIP_TIED": "kernel"}, None, {"tied": "kernel"}),
    ("iterate_tied_composed", "tied", TIED, {"MLHIP_TIED": "composed"}, None, {"tied": "composed"}),
    ("iterate_diag_two_shards", "diag", DIAG_KERNEL, {}, [0, 0], {"diag_kernel": True}),
    ("iterate_tied_two_shards", "tied", TIED, {}, [0, 0], {"tied": "kernel"}),
]

# (name, mode, shape, expected route): em_iterate_restarts with R = 3
RESTARTS_CASES = [
    ("restarts_diag", "diag", DIAG_KERNEL, {"restarts": (3, "sequential")}),
    ("restarts_tied", "tied", TIED, {"restarts": (3, "sequential")}),
]

SCORE_CASES = [("score_diag", "diag", TIED, {"score": "scalar_fed"}), ("score_tied", "tied", TIED, {"score": "scalar_fed"})]

# (name, covariance type, number_initialisations, maximise_first, verbose)
FACADE_CASES = [(f"facade_{mode}_R{R}" + ("_maximise_first" if mf else ""), mode, R, mf, False)
                for mode in ("full", "diag", "tied") for R in (1, 3) for mf in (False, True)]
FACADE_CASES += [("facade_diag_verbose", "diag", 3, False, True), ("facade_tied_verbose", "tied", 3, False, True)]


def run_step_case(ctx, case):
    from ml_amd import _lib
    name, mode, (d, K, n), env, weighted, expected = case
    X, w, pi0, mu0, full = make_inputs(d, K, n)
    out = {}
    with switches(env):
        dt = _lib.Data(ctx, X)
        try:
            if weighted:
                dt.set_weights(w)
            wrong = _route_mismatch(dt, K, mode, expected)
            step = dt.em_step_diag if mode == "diag" else dt.em_step_tied
            first = step(pi0, mu0, mode_covariance(full, mode))
            _put_step(out, name + "/step1", first)
            _left_behind(dt, K, out, name + "/step1")
            _put_step(out, name + "/step2", step(*first[1:]))
            _left_behind(dt, K, out, name + "/step2")
        finally:
            dt.close()
    return out, wrong


def run_iterate_case(ctx, case):
    from ml_amd import _lib
    name, mode, (d, K, n), env, devices, expected = case
    X, _, pi0, mu0, full = make_inputs(d, K, n)
    out = {}
    with switches(env):
        owner = _lib.Context.group(len(devices), device_ids=devices) if devices else ctx
        try:
            dt = _lib.Data(owner, X)
            try:
                wrong = _route_mismatch(dt, K, mode, expected)
                _put_loop(out, name, dt.em_iterate(pi0, mu0, mode_covariance(full, mode), 30, 1e-10, 1e-10, **_kind(mode)))
                out[name + "/labels_crc"] = _crc(dt.em_labels(K))
            finally:
                dt.close()
        finally:
            if devices:
                owner.close()
    return out, wrong


def run_restarts_case(ctx, case):
    from ml_amd import _lib
    name, mode, (d, K, n), expected = case
    X, _, _, _, full = make_inputs(d, K, n)
    out = {}
    dt = _lib.Data(ctx, X)
    try:
        wrong = _route_mismatch(dt, K, mode, expected)
        restarts, best = dt.em_iterate_restarts(*restart_starts(X, K, 3, mode, full), 30, 1e-10, 1e-10, **_kind(mode))
        out[name + "/best"] = np.uint32(best)
        for r, result in enumerate(restarts):
            _put_loop(out, f"{name}/restart{r}", result)
        out[name + "/labels_crc"] = _crc(dt.em_labels(K))
    finally:
        dt.close()
    return out, wrong


def run_score_case(ctx, case):
    from ml_amd import _lib
    name, mode, (d, K, n), expected = case
    X, _, pi0, mu0, full = make_inputs(d, K, n)
    out = {}
    dt = _lib.Data(ctx, X)
    try:
        wrong = _route_mismatch(dt, K, mode, expected)
        densities, labels = dt.em_score(pi0, mu0, mode_covariance(full, mode), **_kind(mode))
        out[name + "/densities_crc"], out[name + "/labels_crc"] = _crc(densities), _crc(labels)
        out[name + "/densities_head"] = densities[:64].copy()
    finally:
        dt.close()
    return out, wrong


def run_facade_case(ctx, case):
    """One ml_amd.cppyml.EM fit (the facade owns its device context; `ctx` is not used)."""
    from ml_amd.cppyml import clustering as cl
    name, mode, R, maximise_first, verbose = case
    d, K, n = FACADE
    X = make_inputs(d, K, n)[0]
    em = cl.EM(K)
    em.set_seed(VERBOSE_SEED[mode] if verbose else FACADE_SEED)
    em.set_maximum_steps(40)
    em.set_covariance_type(mode)
    em.set_number_initialisations(R)
    if maximise_first:
        em.set_maximise_first(True)
        em.set_responsibilities_initialiser(cl.ClosestCentroid(cl.KPP()))
    out, printed = {}, {}
    if verbose:
        em.set_verbose(True)
        with captured_stdout(printed):
            converged = em.fit(X)
        out[name + "/stdout_crc"] = np.uint32(zlib.crc32(printed["out"]))
    else:
        converged = em.fit(X)
    out[name + "/fit_returned"] = np.bool_(converged)
    out[name + "/mixing"], out[name + "/means"] = em.mixing_probabilities, em.means
    out[name + "/covariances"] = np.stack([em.covariance(k) for k in range(K)])
    out[name + "/log_likelihood"], out[name + "/steps_done"] = np.float64(em.log_likelihood), np.uint32(em.steps_done)
    out[name + "/converged"], out[name + "/best_initialisation"] = np.bool_(em.converged), np.uint32(em.best_initialisation)
    out[name + "/initialisation_log_likelihoods"] = em.initialisation_log_likelihoods
    out[name + "/initialisation_steps"] = em.initialisation_steps
    out[name + "/initialisation_converged"] = em.initialisation_converged
    out[name + "/labels_crc"] = _crc(em.labels)
    out[name + "/responsibilities"] = _pin(em.responsibilities_rows(0, 64))
    # a verbose fit must have put the winner's E-step back (the mode-to-full conversion): that needs a winner before the last start
    wrong = {"best_initialisation": (int(em.best_initialisation), "not 2")} if verbose and em.best_initialisation == 2 else {}
    return out, wrong


def all_cases():
    return ([(c[0], run_step_case, c) for c in STEP_CASES] + [(c[0], run_iterate_case, c) for c in ITERATE_CASES] +
            [(c[0], run_restarts_case, c) for c in RESTARTS_CASES] + [(c[0], run_score_case, c) for c in SCORE_CASES] +
            [(c[0], run_facade_case, c) for c in FACADE_CASES])
