"""Restarts of EM (mlhip_em_iterate_restarts): R loops from R starts in one call, the best of them left on the handle.

Every comparison is BIT for bit, against the solo loop mlhip_em_iterate from the same start on the same handle with
MLHIP_RESIDENT=0 (the three-launch loop, which tests/test_gpu_iterate.py pins to the oracle and tests/test_gpu_resident.py ties the
one-launch loop to). The batched route (em_restarts.hip) runs the solo launches' pass, grid, reduction order and closing arithmetic
with the restart as the second grid dimension; what these tests would catch is a wrong grid, a wrong reduction order, a stale record
slot, or a restart that kept running after it had converged.

The batch exists where the solo iteration is the fused kernel's vector-unit form. Below 2^20 rows the routing prefers that form for
K F <= 64 accumulators only (F = (d + 1)(d + 2) / 2); the shapes above it -- (4, 7, 1025), (2, 16, 4097) and LARGE_SHAPES -- are run
with MLHIP_FUSED_VALU=2 (the vector-unit form wherever it is built), for the solo reference and the batched call alike, so that
they reach the batched kernels too. Every batched case asserts the route it took."""
import contextlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(2, 3, 100), (2, 3, 1000), (2, 3, 10000), (4, 3, 10000), (1, 16, 5000), (1, 1, 300), (3, 6, 7000), (6, 2, 3000), (3, 1, 64),
          (2, 5, 65), (2, 3, 63), (2, 3, 257), (4, 7, 1025), (2, 16, 4097)]
RESTARTS = [1, 2, 3, 5]
# the three ways a pair is run: (max_steps, atol) -- restarts stopping at different iterations; exactly 7 iterations; exactly 1
MODES = {"converge": (60, 1e-9), "seven": (7, 0.0), "one": (1, 0.0)}


@contextlib.contextmanager
def _env(**values):
    old = {k: os.environ.get(k) for k in values}
    try:
        for k, v in values.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctx():
    from ml_amd import _lib
    c = _lib.Context()
    yield c
    c.close()


def _problem(d, K, n, seed, R=5, spread=3.0):
    """A K-cluster sample and R starts: the cluster centres jittered more and more (so the loops stop at different iterations)."""
    rng = np.random.default_rng(seed)
    means = spread * rng.standard_normal((K, d))
    comp = rng.integers(0, K, n)
    X = np.ascontiguousarray(means[comp] + rng.standard_normal((n, d)))
    mu0 = np.stack([means + (0.2 + 0.4 * r) * rng.standard_normal((K, d)) for r in range(R)])
    return X, mu0


def _same(a, b):
    assert a[0] == b[0] and a[1] == b[1]
    assert a[2] == b[2] or (np.isnan(a[2]) and np.isnan(b[2]))
    assert np.array_equal(a[6], b[6], equal_nan=True)
    for x, y in zip(a[3:6], b[3:6]):
        assert np.array_equal(x, y, equal_nan=True)


def _form(d, K):
    """The switch a shape needs for its solo iteration to be the vector-unit form (see the module's docstring)."""
    return {"MLHIP_FUSED_VALU": "2"} if K * (d + 1) * (d + 2) // 2 > 64 else {}


def _solo(dt, K, pi0, mu0, S0, max_steps, atol, **kind):
    """The solo loop from every start, one after the other: per start (result, labels, responsibilities)."""
    out = []
    with _env(MLHIP_RESIDENT="0", **_form(dt.d, K)):
        for r in range(len(pi0)):
            res = dt.em_iterate(pi0[r], mu0[r], S0[r], max_steps, atol, 0.0, **kind)
            out.append((res, dt.em_labels(K), dt.em_responsibilities(K)))
    return out


_reference = {}


def _shape_reference(ctx, d, K, n):
    """Sample, five starts and their solo runs in the three modes: computed once per shape, shared by the R cases, left unchanged."""
    key = (d, K, n)
    if key not in _reference:
        from ml_amd import _lib
        X, mu0 = _problem(d, K, n, 31 * d + K + n)
        dt = _lib.Data(ctx, X)
        _, cov = dt.sample_covariance()
        pi0, S0 = np.full((5, K), 1.0 / K), np.stack([np.stack([cov] * K)] * 5)
        solo = {mode: _solo(dt, K, pi0, mu0, S0, *MODES[mode]) for mode in MODES}
        dt.close()
        _reference[key] = (X, pi0, mu0, S0, solo)
    return _reference[key]


def _restarts(dt, K, *args, **kind):
    """em_iterate_restarts, and the E-step state it leaves on the handle: (restarts, best, labels, responsibilities)."""
    restarts, best = dt.em_iterate_restarts(*args, **kind)
    return restarts, best, dt.em_labels(K), dt.em_responsibilities(K)


def _check_call(call, solo):
    """Every restart equals its solo run; best is the rule's; the handle was left holding the winner's E-step state."""
    from ml_amd import _lib
    restarts, best, labels, resp = call
    assert len(restarts) == len(solo)
    for got, (ref, _, _) in zip(restarts, solo):
        _same(got, ref)
    assert best == _lib.em_select_restart([r[2] for r in restarts], [r[1] for r in restarts])
    assert np.array_equal(labels, solo[best][1])
    assert np.array_equal(resp, solo[best][2], equal_nan=True)


@pytest.mark.parametrize("R", RESTARTS)
@pytest.mark.parametrize("d,K,n", SHAPES)
def test_batched_restarts_are_bit_identical_to_the_solo_loops(ctx, d, K, n, R):
    from ml_amd import _lib
    X, pi0, mu0, S0, solo = _shape_reference(ctx, d, K, n)
    dt = _lib.Data(ctx, X)
    with _env(MLHIP_EM_RESTARTS="batch", **_form(d, K)):
        assert dt.em_route(K)["fused_form"] == "valu" and dt.em_restarts_route(K, R)[0] == "batched"
        for mode, (max_steps, atol) in MODES.items():
            call = _restarts(dt, K, pi0[:R], mu0[:R], S0[:R], max_steps, atol, 0.0)
            _check_call(call, solo[mode][:R])
        assert [r[0] for r in call[0]] == [1] * R
        # a second call on the same handle, other starts: the rings and the scratch are reused
        mu1 = mu0[:R] + 0.05
        call = _restarts(dt, K, pi0[:R], mu1, S0[:R], 9, 0.0, 0.0)
    _check_call(call, _solo(dt, K, pi0[:R], mu1, S0[:R], 9, 0.0))
    dt.close()


# the largest instantiation of every dimension (K = valu_max_k(d): K F = 96 ... 112 accumulators per lane), and one more per dimension
LARGE_SHAPES = [(1, 32, 700), (1, 22, 257), (2, 11, 900), (3, 10, 900), (3, 7, 300), (4, 5, 1000), (6, 4, 500), (6, 3, 321)]


@pytest.mark.parametrize("d,K,n", LARGE_SHAPES)
def test_batched_restarts_of_the_largest_instantiations(ctx, d, K, n):
    """The pass kernels the routing selects only from 2^20 rows on (or under MLHIP_FUSED_VALU=2): three restarts, the three modes."""
    from ml_amd import _lib
    assert _form(d, K)
    R = 3
    X, mu0 = _problem(d, K, n, 13 * d + K, R=R)
    dt = _lib.Data(ctx, X)
    _, cov = dt.sample_covariance()
    pi0, S0 = np.full((R, K), 1.0 / K), np.stack([np.stack([cov] * K)] * R)
    for max_steps, atol in MODES.values():
        solo = _solo(dt, K, pi0, mu0, S0, max_steps, atol)
        with _env(MLHIP_EM_RESTARTS="batch", **_form(d, K)):
            assert dt.em_restarts_route(K, R)[0] == "batched"
            call = _restarts(dt, K, pi0, mu0, S0, max_steps, atol, 0.0)
        _check_call(call, solo)
    dt.close()


def test_more_restarts_than_one_launch_carries(ctx):
    from ml_amd import _lib
    d, K, n = 2, 3, 300
    X, mu0 = _problem(d, K, n, 77, R=2)
    dt = _lib.Data(ctx, X)
    _, cov = dt.sample_covariance()
    with _env(MLHIP_EM_RESTARTS="batch"):
        route, cap = dt.em_restarts_route(K, 1000)
    assert route == "batched" and 1 <= cap <= 32
    R = cap + 2
    pick = np.arange(R) % 2                                         # two start sets, alternated: two solo runs are the reference
    pi0, S0 = np.full((2, K), 1.0 / K), np.stack([np.stack([cov] * K)] * 2)
    solo = _solo(dt, K, pi0, mu0, S0, 40, 1e-9)
    with _env(MLHIP_EM_RESTARTS="batch"):
        call = _restarts(dt, K, pi0[pick], mu0[pick], S0[pick], 40, 1e-9, 0.0)
    _check_call(call, [solo[p] for p in pick])
    assert call[1] in (0, 1)                                           # the first of equals
    dt.close()


def test_a_batched_iteration_is_three_launches_however_many_restarts(ctx):
    from ml_amd import _lib
    d, K, n, R, S = 2, 3, 5000, 4, 12
    X, mu0 = _problem(d, K, n, 5, R=R)
    dt = _lib.Data(ctx, X)
    _, cov = dt.sample_covariance()
    pi0, S0 = np.full((R, K), 1.0 / K), np.stack([np.stack([cov] * K)] * R)
    ctx.timing_enable(True)
    ctx.timing_reset()
    with _env(MLHIP_EM_RESTARTS="batch"):
        assert dt.em_restarts_route(K, R)[0] == "batched"
        restarts, _ = dt.em_iterate_restarts(pi0, mu0, S0, S, 0.0, 0.0)
    launches = {name: ctx.timing_get(name)[1] for name in ("em_restarts_pass", "em_restarts_reduce", "em_restarts_close", "em_fused",
                                                           "em_resident")}
    ctx.timing_enable(False)
    assert [r[0] for r in restarts] == [S] * R
    assert launches == {"em_restarts_pass": S, "em_restarts_reduce": S, "em_restarts_close": S, "em_fused": 0, "em_resident": 0}, launches
    dt.close()


def test_a_restart_that_needs_the_refinement_pass_leaves_the_batch(ctx):
    """Components far from the data mean and tight (tests/test_gpu_resident.py's construction; tests/test_gpu_hp_edges.py's refinement
    sample has ONE far cluster, which every start that resolves it flags): the solo loop from the `tight` start runs the host's
    refinement pass (checked on the solo runs first), the two `flat` starts -- every component the whole sample's Gaussian, which EM
    leaves as it is -- never do. Batched together with one more start, the flat ones stay in the launches for all iterations, the
    tight one is handed to the solo loop, and every restart still equals its solo run."""
    from ml_amd import _lib
    d, K, n, S = 2, 3, 12000, 6
    rng = np.random.default_rng(11)
    centres = np.array([[0.0] * d, [300.0] * d, [-200.0] * d])
    sig = np.array([1.0, 1e-3, 1e-2])
    comp = rng.integers(0, K, n)
    X = np.ascontiguousarray(centres[comp] + rng.standard_normal((n, d)) * sig[comp][:, None])
    dt = _lib.Data(ctx, X)
    _, cov = dt.sample_covariance()
    tight_mu = centres + 0.1 * sig[:, None] * rng.standard_normal((K, d))
    tight_S = np.stack([np.eye(d) * v * 1.5 for v in sig ** 2])
    flat_mu, wide = np.tile(X.mean(axis=0), (K, 1)), np.stack([cov] * K)
    mu0 = np.stack([centres + 20.0 * rng.standard_normal((K, d)), tight_mu, flat_mu, flat_mu])
    S0 = np.stack([wide, tight_S, wide, wide])
    pi0 = np.array([[1 / 3, 1 / 3, 1 / 3], [1 / 3, 1 / 3, 1 / 3], [0.2, 0.3, 0.5], [0.6, 0.3, 0.1]])
    ctx.timing_enable(True)
    refined = []
    for r in range(4):
        ctx.timing_reset()
        dt.em_iterate(pi0[r], mu0[r], S0[r], S, 0.0, 0.0)
        refined.append(ctx.timing_get("em_refine")[1])
    ctx.timing_enable(False)
    assert refined[1] >= 1 and refined[2] == 0 and refined[3] == 0, refined
    solo = _solo(dt, K, pi0, mu0, S0, S, 0.0)
    ctx.timing_enable(True)
    ctx.timing_reset()
    with _env(MLHIP_EM_RESTARTS="batch"):
        assert dt.em_restarts_route(K, 4)[0] == "batched"
        restarts, best = dt.em_iterate_restarts(pi0, mu0, S0, S, 0.0, 0.0)
    launches = {name: ctx.timing_get(name)[1] for name in ("em_restarts_pass", "em_resident", "em_fused", "em_refine")}
    ctx.timing_enable(False)
    call = (restarts, best, dt.em_labels(K), dt.em_responsibilities(K))
    assert launches["em_restarts_pass"] == S, launches                          # the flat restarts stayed in the launches to the end
    assert launches["em_resident"] + launches["em_fused"] >= 1, launches        # the batch handed a restart to the solo loop ...
    assert launches["em_refine"] >= 1, launches                                 # ... which ran the refinement pass
    _check_call(call, solo)
    dt.close()


def test_route(ctx):
    """Batched where the solo iteration is the vector-unit pass on at most one workgroup per CU; sequential everywhere else; the
    switch forces either route where the batch exists and is ignored where it does not."""
    from ml_amd import _lib
    rng = np.random.default_rng(2)

    def block(n, d, context=ctx):
        return _lib.Data(context, rng.standard_normal((n, d)))

    plain = block(4000, 2)
    with _env(MLHIP_EM_RESTARTS="batch"):
        assert plain.em_route(3)["fused_form"] == "valu"
        route, cap = plain.em_restarts_route(3, 4)
        assert route == "batched" and 1 <= cap <= 32
        assert plain.em_restarts_route(3, 1) == ("batched", cap)
        assert plain.em_restarts_route(3, 4, "diag") == ("sequential", 1)
        assert plain.em_restarts_route(3, 4, "tied") == ("sequential", 1)
        assert plain.em_restarts_route(17, 4) == ("sequential", 1)             # K above valu_max_k(2) = 16
        assert plain.em_restarts_route(16, 4) == ("sequential", 1)             # built, but not the solo route at this N (K F = 96 > 64)
        weighted = block(4000, 2)
        weighted.set_weights(rng.uniform(0.5, 2.0, 4000))
        assert weighted.em_restarts_route(3, 4) == ("sequential", 1)
        for d in (8, 5):
            other = block(4000, d)
            assert other.em_restarts_route(2, 4) == ("sequential", 1), d
            other.close()
        large = block(100000, 2)                                               # more than one workgroup per CU (256 rows each)
        assert large.em_route(3)["fused_form"] == "valu" and large.em_restarts_route(3, 4) == ("sequential", 1)
        group = _lib.Context.group(2, device_ids=[0, 0])
        sharded = block(4000, 2, group)
        assert sharded.em_restarts_route(3, 4) == ("sequential", 1)
        sharded.close()
        group.close()
    with _env(MLHIP_EM_RESTARTS="sequential"):
        assert plain.em_restarts_route(3, 32) == ("sequential", 1)
    with _env(MLHIP_EM_RESTARTS=None):
        assert plain.em_restarts_route(3, 1) == ("sequential", 1)
        assert plain.em_restarts_route(3, AUTOMATIC_BATCH_FROM - 1) == ("sequential", 1)
        assert plain.em_restarts_route(3, AUTOMATIC_BATCH_FROM) == ("batched", cap)
        assert large.em_restarts_route(3, 32) == ("sequential", 1)
    for dt in (plain, weighted, large):
        dt.close()


AUTOMATIC_BATCH_FROM = 4      # MLHIP_RESTARTS_BATCH_FROM (mlhip.h; measured: profiles/em_restarts_timing.txt)

SEQUENTIAL_KINDS = ["diag", "tied", "weighted", "d16"]


def _sequential_case(kind, context):
    """(handle, K, starts, keyword arguments of em_iterate) of a fit the batch does not exist for: n = 2000, R = 3."""
    from ml_amd import _lib
    d, K = (16, 4) if kind == "d16" else (4, 3)
    n, R = 2000, 3
    X, mu0 = _problem(d, K, n, 100 + d, R=R)
    dt = _lib.Data(context, X)
    if kind == "weighted":
        dt.set_weights(np.random.default_rng(9).uniform(0.25, 3.0, n))
    cov = np.cov(X.T)
    pi0 = np.full((R, K), 1.0 / K)
    if kind == "diag":
        return dt, K, (pi0, mu0, np.stack([np.tile(np.diag(cov), (K, 1))] * R)), {"diagonal": True}
    if kind == "tied":
        return dt, K, (pi0, mu0, np.stack([cov] * R)), {"tied": True}
    return dt, K, (pi0, mu0, np.stack([np.stack([cov] * K)] * R)), {}


def _check_sequential(kind, context):
    dt, K, (pi0, mu0, S0), how = _sequential_case(kind, context)
    solo = _solo(dt, K, pi0, mu0, S0, 40, 1e-9, **how)
    call = _restarts(dt, K, pi0, mu0, S0, 40, 1e-9, 0.0, **how)
    _check_call(call, solo)
    best = call[1]
    # a winner that is not the last restart run: its kept state is what comes back
    order = [best] + [r for r in range(len(pi0)) if r != best]
    call = _restarts(dt, K, pi0[order], mu0[order], S0[order], 40, 1e-9, 0.0, **how)
    _check_call(call, [solo[r] for r in order])
    assert call[1] == 0
    dt.close()


@pytest.mark.parametrize("kind", SEQUENTIAL_KINDS)
def test_sequential_restarts_equal_the_solo_calls(ctx, kind):
    _check_sequential(kind, ctx)


@pytest.mark.parametrize("kind", SEQUENTIAL_KINDS)
def test_sequential_restarts_on_a_device_group(kind):
    from ml_amd import _lib
    group = _lib.Context.group(2, device_ids=[0, 0])
    try:
        _check_sequential(kind, group)
    finally:
        group.close()


def _three_clusters(n=3000, seed=4):
    rng = np.random.default_rng(seed)
    centres = np.array([[0.0, 0.0], [6.0, 1.0], [-2.0, 7.0]])
    comp = rng.integers(0, 3, n)
    return np.ascontiguousarray(centres[comp] + rng.standard_normal((n, 2)) * np.array([1.0, 0.6, 1.4])[comp][:, None])


def _configure(em, seed, maximise_first):
    from ml_amd.cppyml import clustering as cl
    em.set_seed(seed)
    em.set_maximum_steps(200)
    if maximise_first:
        em.set_maximise_first(True)
        em.set_responsibilities_initialiser(cl.ClosestCentroid(cl.KPP()))


def _fitted(em):
    return {"converged": em.converged, "steps_done": em.steps_done, "log_likelihood": em.log_likelihood, "means": em.means,
            "mixing": em.mixing_probabilities, "covariances": np.stack([em.covariance(k) for k in range(em.number_components)]),
            "labels": em.labels, "responsibilities": em.responsibilities}


@pytest.mark.parametrize("maximise_first", [False, True])
def test_facade_fit_with_restarts_reproduces_consecutive_solo_fits(maximise_first):
    """EM(3), set_seed(s), set_number_initialisations(4), fit(X) == the same seed fitted four times in a row on one object."""
    from ml_amd.cppyml import clustering as cl
    from ml_amd import _lib
    X, seed, R = _three_clusters(), 12345, 4
    em1 = cl.EM(3)
    _configure(em1, seed, maximise_first)
    solo = []
    for _ in range(R):
        converged = em1.fit(X)
        solo.append(_fitted(em1))
        assert converged == solo[-1]["converged"]
        assert em1.number_initialisations == 1 and em1.best_initialisation == 0
        assert np.array_equal(em1.initialisation_log_likelihoods, [solo[-1]["log_likelihood"]])      # the default: one entry, today's result
        assert list(em1.initialisation_steps) == [solo[-1]["steps_done"]] and list(em1.initialisation_converged) == [converged]
    em = cl.EM(3)
    _configure(em, seed, maximise_first)
    em.set_number_initialisations(R)
    converged = em.fit(X)
    assert np.array_equal(em.initialisation_log_likelihoods, [s["log_likelihood"] for s in solo])
    assert list(em.initialisation_steps) == [s["steps_done"] for s in solo]
    assert list(em.initialisation_converged) == [s["converged"] for s in solo]
    best = em.best_initialisation
    assert best == _lib.em_select_restart([s["log_likelihood"] for s in solo], [s["converged"] for s in solo])
    got, want = _fitted(em), solo[best]
    assert converged == want["converged"]
    for key, value in want.items():
        assert np.array_equal(got[key], value), key


def test_verbose_fit_with_restarts_keeps_the_winner_of_the_verbose_solo_fits(capfd):
    """Verbose mode runs the initialisations one after the other through the per-step entry points: with full covariances the fit
    equals the verbose solo fit `best_initialisation` names -- the winner's E-step state is put back by one E-step on the inputs of
    its last one, the same records through the same E-step kernel."""
    from ml_amd.cppyml import clustering as cl
    from ml_amd import _lib
    X, seed, R = _three_clusters(1500, seed=8), 99, 3
    em1 = cl.EM(3)
    _configure(em1, seed, False)
    em1.set_verbose(True)
    solo = []
    for _ in range(R):
        em1.fit(X)
        solo.append(_fitted(em1))
    em = cl.EM(3)
    _configure(em, seed, False)
    em.set_verbose(True)
    em.set_number_initialisations(R)
    converged = em.fit(X)
    out = capfd.readouterr().out
    assert all(f"Initialisation {r}\n" in out for r in range(R))
    assert np.array_equal(em.initialisation_log_likelihoods, [s["log_likelihood"] for s in solo])
    assert list(em.initialisation_steps) == [s["steps_done"] for s in solo]
    best = em.best_initialisation
    assert best == _lib.em_select_restart([s["log_likelihood"] for s in solo], [s["converged"] for s in solo])
    got, want = _fitted(em), solo[best]
    assert converged == want["converged"]
    for key, value in want.items():
        assert np.array_equal(got[key], value), key
