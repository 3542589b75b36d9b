"""Row weights on the GPU (mlhip_data_set_weights): a weighted step, fit or piece against the UNWEIGHTED extended-precision
reference on the replicated sample (row i repeated w_i times; tests/test_weights_cases.py), with the CPU oracle on that same
sample as the yardstick and the limits of tests/test_gpu_hp_error.py unchanged: err_gpu <= 4 max(err_cpu, 8 * 2^-53), covariances
per component by that module's model. Each case asserts its route first and prints one `HPERR` line.
Needs a GPU: `timeout -k 10 1800 pytest tests/test_gpu_weights.py -m gpu -x -s`.

A weighted block runs the E-step tier of its shape and, at d = 12 ... 128 with K <= 64, the self-normalising statistics kernel in its
weighted form (self_norm = True); under MLHIP_SELF_NORM=0 and on the other tiers one pass writes w_i r_ik for the statistics kernel
of the shape."""
import numpy as np
import pytest

from oracle import hp_reference as hp
from oracle.hp_cases import refinement_problem
from test_gpu_hp_error import FLOOR, _assert_route, _errors, _report_and_check, _ridge_off, _setenv
from test_weights_cases import DIAG_SHAPE, SHAPES, case, references, replicate, weights

pytestmark = pytest.mark.gpu
LD = np.longdouble


@pytest.fixture(scope="module")
def ctx():
    from ml_amd import _lib
    c = _lib.Context()
    yield c
    c.close()


def _block(ctx, X, w=None):
    from ml_amd import _lib
    dt = _lib.Data(ctx, np.ascontiguousarray(X, dtype=np.float64))
    if w is not None:
        dt.set_weights(w)
    return dt


def _ratio(X, ref, diagonal=False):
    """Refinement ratios of the new parameters about the block's shift (the UNWEIGHTED column mean of the block)."""
    shift = X.astype(LD).mean(axis=0)
    return hp.conditioning(shift, ref[3], **({"variances": ref[4]} if diagonal else {"covs": ref[4]}))["ratio"]


WEIGHTED_ROUTE = {"fused": False, "sparse": False, "resident": False, "diag_kernel": False}
# name, shape, switches, E-step tier, whether the statistics kernel normalises (and weights) the log-responsibilities itself
STEP_CASES = [(f"weighted step d={s[0]} K={s[1]}", s, {}, tier, tier == "matrix4") for s, tier in SHAPES] + [
    ("weighted step d=13 K=5, MLHIP_SELF_NORM=0", (13, 5, 3001, 0.0), {"MLHIP_SELF_NORM": "0"}, "matrix4", False),
    ("weighted step d=16 K=8, MLHIP_SELF_NORM=0", (16, 8, 4001, 2.0), {"MLHIP_SELF_NORM": "0"}, "matrix4", False),
    ("weighted step d=32 K=16, MLHIP_SELF_NORM=0", (32, 16, 6001, 0.0), {"MLHIP_SELF_NORM": "0"}, "matrix4", False),
    ("weighted step d=64 K=4, MLHIP_SELF_NORM=0", (64, 4, 3001, 3.0), {"MLHIP_SELF_NORM": "0"}, "matrix4", False),
    ("weighted step d=16 K=8, MLHIP_ESTEP=valu", (16, 8, 4001, 2.0), {"MLHIP_ESTEP": "valu"}, "scalar_fed", False),
    ("weighted step d=130 K=3, plain tier", (130, 3, 2001, 0.0), {"MLHIP_BIG_DIM": "0"}, "plain", False)]


@pytest.mark.parametrize("name,shape,env,tier,self_norm", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_weighted_step(ctx, monkeypatch, name, shape, env, tier, self_norm):
    X, w, pi0, mu0, S0, _ = case(*shape)
    ref, cpu = references(*shape)
    _setenv(monkeypatch, env)
    dt = _block(ctx, X, w)
    _assert_route(dt.em_route(len(pi0)), dict(WEIGHTED_ROUTE, estep=tier, self_norm=self_norm))
    assert dt.weight_sum == float(w.sum())
    ctx.timing_enable(True)
    ctx.timing_reset()
    ll, pi1, mu1, S1 = dt.em_step(pi0, mu0, S0)
    passes = ctx.timing_get("em_weights")[1]
    ctx.timing_enable(False)
    # the self-normalising form needs no pass of its own in the iteration; the others run the w lse pass and the w r pass
    assert passes == (0 if self_norm else 2), passes
    name += " [self-normalising]" if self_norm else ""
    dt.close()
    e_cpu = dict(_errors(cpu, ref), resp=None)
    _report_and_check(name, _errors((ll, None, pi1, mu1, _ridge_off(S1, False)), ref), e_cpu, _ratio(X, ref))


def test_weighted_diagonal_step(ctx):
    X, w, pi0, mu0, var0, _ = case(*DIAG_SHAPE, True)
    ref, cpu = references(*DIAG_SHAPE, True)
    dt = _block(ctx, X, w)
    _assert_route(dt.em_route(len(pi0), "diag"), dict(WEIGHTED_ROUTE, estep="matrix4", self_norm=True))
    ll, pi1, mu1, var1 = dt.em_step_diag(pi0, mu0, var0)
    dt.close()
    _report_and_check("weighted diagonal step d=16 K=8 (full-covariance kernels)", _errors((ll, None, pi1, mu1, _ridge_off(var1, True)), ref),
                      dict(_errors(cpu, ref), resp=None), _ratio(X, ref, True))


@pytest.mark.parametrize("factor", [1.0, 0.25])
def test_scaling_the_weights_changes_nothing_beyond_rounding(ctx, factor):
    shape = (16, 8, 4001, 2.0)
    X, w, pi0, mu0, S0, _ = case(*shape)
    ref, cpu = references(*shape)
    dt = _block(ctx, X, w * factor)
    assert dt.weight_sum == float(w.sum()) * factor
    ll, pi1, mu1, S1 = dt.em_step(pi0, mu0, S0)
    dt.close()
    _report_and_check(f"weights m * {factor}, d=16 K=8", _errors((ll, None, pi1, mu1, _ridge_off(S1, False)), ref),
                      dict(_errors(cpu, ref), resp=None), _ratio(X, ref))


# ---- pieces ------------------------------------------------------------------------------------------------------------------

def _limit(e_cpu):
    return 4 * max(e_cpu, FLOOR)


def test_weighted_expectation_log_likelihood(ctx):
    shape = (13, 5, 3001, 0.0)
    X, w, pi0, mu0, S0, _ = case(*shape)
    ref, cpu = references(*shape)
    dt = _block(ctx, X, w)
    ll = dt.em_expectation(pi0, mu0, S0)
    dt.close()
    e_gpu, e_cpu = abs(float((LD(ll) - ref[0]) / ref[0])), abs(float((LD(cpu[0]) - ref[0]) / ref[0]))
    print(f"HPERR weighted expectation d=13 | ll {e_gpu:.1e} / {e_cpu:.1e}", flush=True)
    assert e_gpu <= _limit(e_cpu)


@pytest.mark.parametrize("shape", [(6, 8, 3001, 2.0), (33, 4, 3001, 0.0)], ids=["d=6", "d=33"])
def test_weighted_sample_covariance(ctx, shape):
    X, w, _, _, _, Xr = case(*shape)
    mean_ref, cov_ref = hp.sample_covariance(Xr)
    dt = _block(ctx, X, w)
    mean, cov = dt.sample_covariance()
    dt.close()
    e_gpu = (hp.rel_err(mean, mean_ref), hp.rel_err(cov, cov_ref))
    e_cpu = (hp.rel_err(Xr.mean(axis=0), mean_ref), hp.rel_err(np.cov(Xr.T), cov_ref))
    print(f"HPERR weighted sample covariance d={shape[0]} | mean {e_gpu[0]:.1e} / {e_cpu[0]:.1e} | cov {e_gpu[1]:.1e} / {e_cpu[1]:.1e}", flush=True)
    assert e_gpu[0] <= _limit(e_cpu[0]) and e_gpu[1] <= _limit(e_cpu[1])


@pytest.mark.parametrize("source", ["labels", "responsibilities"])
def test_weighted_maximisation_from(ctx, oracle, source):
    shape = (16, 8, 4001, 2.0)
    X, w, pi0, mu0, S0, Xr = case(*shape)
    K, d = len(pi0), X.shape[1]
    rng = np.random.default_rng(5)
    if source == "labels":
        labels = np.argmin(((X[:, None, :] - mu0[None]) ** 2).sum(axis=2), axis=1).astype(np.uint32)
        R = np.zeros((len(X), K))
        R[np.arange(len(X)), labels] = 1.0
    else:
        R = rng.uniform(0.05, 1.0, (len(X), K))
        R /= R.sum(axis=1, keepdims=True)
    Rr = replicate(R, w)
    ref = hp.m_step(Xr, Rr)
    em = oracle.EM(K)
    em.set_responsibilities(Rr, d)
    em.maximisation_step(Xr)
    cpu = (em.mixing_probabilities, em.means, _ridge_off(em.covariances, False))
    dt = _block(ctx, X, w)
    keep = R.copy()
    pi1, mu1, S1 = dt.em_maximisation_from_labels(labels, K) if source == "labels" else dt.em_maximisation_from(R)
    dt.close()
    assert np.array_equal(R, keep)                                   # the caller's array is not changed
    full = lambda t: (LD(1), None) + tuple(t)                        # noqa: E731  (no log-likelihood in an M-step)
    ref5 = (LD(1), None) + tuple(ref)
    e_gpu, e_cpu = _errors(full((pi1, mu1, _ridge_off(S1, False))), ref5), _errors(full(cpu), ref5)
    _report_and_check(f"weighted M-step from {source}, d=16 K=8", e_gpu, e_cpu, _ratio(X, ref5))


def test_weighted_refinement_pass(ctx, oracle):
    """A far, tight component (hp_cases.refinement_problem above the guard): the second pass about the component's own mean
    uses the same weights."""
    X, pi0, mu0, S0 = refinement_problem(32, 2e4)
    w = weights(len(X))
    Xr = replicate(X, w)
    ref = hp.em_step(Xr, pi0, mu0, S0)
    from oracle.hp_cases import oracle_step
    cpu = oracle_step(oracle, Xr, pi0, mu0, S0)
    ratio = _ratio(X, ref)
    dt = _block(ctx, X, w)
    _assert_route(dt.em_route(2), dict(WEIGHTED_ROUTE, estep="matrix4", self_norm=True))
    ctx.timing_enable(True)
    ctx.timing_reset()
    ll, pi1, mu1, S1 = dt.em_step(pi0, mu0, S0)
    refined = ctx.timing_get("em_refine")[1]
    ctx.timing_enable(False)
    dt.close()
    assert refined == int((ratio > 1e4).sum()) and refined >= 1, (refined, ratio)
    _report_and_check(f"weighted refinement d=32 ratio {ratio.max():.4g} refine launches {refined}",
                      _errors((ll, None, pi1, mu1, _ridge_off(S1, False)), ref), dict(_errors(cpu, ref), resp=None), ratio,
                      refined=ratio > 1e4)


# ---- per-row results are not weighted ----------------------------------------------------------------------------------------

PER_ROW = [((6, 8, 3001, 2.0), {"MLHIP_FUSED": "0"}), ((16, 8, 4001, 2.0), {}), ((33, 4, 3001, 0.0), {}), ((130, 3, 2001, 0.0), {})]


@pytest.mark.parametrize("shape,env", PER_ROW, ids=[f"d={s[0]}" for s, _ in PER_ROW])
def test_per_row_results_are_unweighted(ctx, monkeypatch, shape, env):
    """Responsibilities and labels after a weighted step against those after the unweighted step with the same parameters on the
    DEFAULT route (d = 16, 33: self-normalising on both sides; d = 130: big-dim). At d = 6 the unweighted default is the fused kernel,
    which a weighted block never takes: there the unweighted side runs under MLHIP_FUSED=0 (mlhip.h says so). mlhip_em_score against
    the default route everywhere."""
    X, w, pi0, mu0, S0, _ = case(*shape)
    K = len(pi0)
    plain = _block(ctx, X)
    dens0, lab0 = plain.em_score(pi0, mu0, S0)
    _setenv(monkeypatch, env)
    plain.em_step(pi0, mu0, S0)
    resp0, labels0 = plain.em_responsibilities(K), plain.em_labels(K)
    plain.close()
    for name in env:
        monkeypatch.delenv(name)
    dt = _block(ctx, X, w)
    dt.em_step(pi0, mu0, S0)
    resp1, labels1 = dt.em_responsibilities(K), dt.em_labels(K)
    dens1, lab1 = dt.em_score(pi0, mu0, S0)
    dt.close()
    assert np.array_equal(resp0, resp1) and np.array_equal(labels0, labels1)
    assert np.array_equal(dens0, dens1) and np.array_equal(lab0, lab1)
    assert (w == 0).any() and np.all(np.isfinite(resp1[w == 0])) and np.allclose(resp1[w == 0].sum(axis=1), 1.0)


# ---- the loop ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("env", [{}, {"MLHIP_DEVICE_CLOSE": "0"}], ids=["device closing", "MLHIP_DEVICE_CLOSE=0"])
@pytest.mark.parametrize("shape", [(6, 8, 3001, 2.0), (16, 8, 4001, 2.0)], ids=["d=6", "d=16"])
def test_weighted_iterate_equals_steps(ctx, monkeypatch, shape, env):
    X, w, pi0, mu0, S0, _ = case(*shape)
    _setenv(monkeypatch, env)
    dt = _block(ctx, X, w)
    assert dt.em_route(len(pi0))["device_close"] == (not env)
    pi, mu, S, lls = pi0, mu0, S0, []
    for _ in range(5):
        ll, pi, mu, S = dt.em_step(pi, mu, S)
        lls.append(ll)
    steps, _, ll_b, pi_b, mu_b, S_b, hist = dt.em_iterate(pi0, mu0, S0, 5)
    dt.close()
    assert steps == 5
    # mlhip.h: "same results as calling mlhip_em_step in a loop, to the last bits of log()"
    assert np.max(np.abs(hist - np.array(lls)) / np.abs(lls)) <= 1e-13 and abs(ll_b - lls[-1]) <= 1e-13 * abs(lls[-1])
    assert hp.rel_err(pi_b, pi.astype(LD)) <= 1e-12 and hp.rel_err(mu_b, mu.astype(LD)) <= 1e-12 and hp.rel_err(S_b, S.astype(LD)) <= 1e-11


# ---- the whole fit through Python ----------------------------------------------------------------------------------------------

def test_weighted_fit_through_python(ctx, oracle):
    from ml_amd.cppyml import clustering
    shape = (6, 8, 3001, 2.0)
    X, w, pi0, mu0, S0, Xr = case(*shape)
    K, steps = len(pi0), 5

    def fitted(sample_weight, n_steps):
        em = clustering.EM(K)
        em.set_means_initialiser(clustering.FixedCentroids(mu0))
        em.set_absolute_tolerance(0.0)
        em.set_relative_tolerance(0.0)
        em.set_maximum_steps(n_steps)
        em.fit(X, sample_weight=sample_weight)
        return em

    # The log-likelihood history step by step (a fit of s steps reports the log-likelihood of its s-th E-step) against the
    # extended-precision chain on the replicated sample -- each step fed the previous one's parameters, + 1e-15 I as the library
    # adds it -- with the oracle's fit of the replicated sample from the same start as the yardstick: the step rule at EVERY step,
    # no looser bound for later ones; the growth per step is what the lines below report.
    _, cov0 = hp.sample_covariance(Xr)
    pi, mu, S = pi0, mu0, np.stack([cov0.astype(np.float64)] * K)
    ref_ll = []
    for _ in range(steps):
        ref = hp.em_step(Xr, pi, mu, S)
        ref_ll.append(ref[0])
        pi, mu, S = ref[2], ref[3], ref[4] + LD(1e-15) * np.eye(X.shape[1], dtype=LD)
    failures = []
    for s in range(2, steps + 1):
        em = fitted(w, s)
        orc = oracle.EM(K)
        orc.set_means_initialiser(oracle.FIXED, mu0)
        orc.set_absolute_tolerance(0.0)
        orc.set_relative_tolerance(0.0)
        orc.set_maximum_steps(s)
        orc.fit(Xr)
        assert em.steps_done == s
        e_gpu = abs(float((LD(em.log_likelihood) - ref_ll[s - 1]) / ref_ll[s - 1]))
        e_cpu = abs(float((LD(orc.log_likelihood) - ref_ll[s - 1]) / ref_ll[s - 1]))
        print(f"HPERR weighted fit d=6 K=8, log-likelihood of E-step {s} | {e_gpu:.1e} / {e_cpu:.1e}", flush=True)
        if not e_gpu <= 4 * max(e_cpu, FLOOR):
            failures.append((s, e_gpu, e_cpu))
    assert not failures, failures
    # the same object afterwards, unweighted: bit for bit a fresh unweighted fit
    em = fitted(w, steps)
    em.fit(X)
    fresh = fitted(None, steps)
    assert em.log_likelihood == fresh.log_likelihood and np.array_equal(em.means, fresh.means)
    assert all(np.array_equal(em.covariance(k), fresh.covariance(k)) for k in range(K))


# ---- clearing, rejection -------------------------------------------------------------------------------------------------------

def test_clearing_the_weights_restores_the_unweighted_step(ctx):
    X, w, pi0, mu0, S0, _ = case(16, 8, 4001, 2.0)
    never = _block(ctx, X)
    want_route, want = never.em_route(len(pi0)), never.em_step(pi0, mu0, S0)
    never.close()
    dt = _block(ctx, X, w)
    dt.em_step(pi0, mu0, S0)
    dt.set_weights(None)
    assert dt.em_route(len(pi0)) == want_route and dt.weight_sum == float(len(X))
    got = dt.em_step(pi0, mu0, S0)
    dt.close()
    assert got[0] == want[0] and all(np.array_equal(a, b) for a, b in zip(got[1:], want[1:]))


@pytest.mark.parametrize("bad", ["nan", "inf", "negative", "all zero"])
def test_bad_weights_are_refused_and_the_block_stays_unweighted(ctx, bad):
    X, w, pi0, mu0, S0, _ = case(6, 8, 3001, 2.0)
    never = _block(ctx, X)
    want = never.em_step(pi0, mu0, S0)
    never.close()
    v = w.copy()
    if bad == "all zero":
        v[:] = 0.0
    else:
        v[1234] = {"nan": np.nan, "inf": np.inf, "negative": -1.0}[bad]
    dt = _block(ctx, X, w)
    with pytest.raises(ValueError):
        dt.set_weights(v)
    assert dt.weight_sum == float(len(X))
    got = dt.em_step(pi0, mu0, S0)
    dt.close()
    assert got[0] == want[0] and all(np.array_equal(a, b) for a, b in zip(got[1:], want[1:]))


# ---- shards --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]], ids=["2 shards", "3 shards"])
def test_weighted_fit_on_a_device_group(ctx, devices):
    from ml_amd import _lib
    X, w, pi0, mu0, S0, _ = case(16, 8, 4001, 2.0)
    w = w.copy()
    w[: len(X) // len(devices) + 1] = 0.0                            # every row of shard 0 has weight 0
    one = _block(ctx, X, w)
    steps, _, ll, pi1, mu1, S1, hist = one.em_iterate(pi0, mu0, S0, 4)
    one.close()
    group = _lib.Context.group(len(devices), device_ids=devices)
    gd = _lib.Data(group, X)
    lo, cnt = gd.shard_rows(0)
    assert not w[lo:lo + cnt].any()
    gd.set_weights(w)
    assert abs(gd.weight_sum - float(w.sum())) <= 1e-12 * w.sum()
    steps_g, _, ll_g, pi_g, mu_g, S_g, hist_g = gd.em_iterate(pi0, mu0, S0, 4)
    bad = w.copy()
    bad[-1] = np.nan                                                  # in the LAST shard: every shard must refuse
    with pytest.raises(ValueError):
        gd.set_weights(bad)
    assert gd.weight_sum == float(len(X))
    gd.close()
    group.close()
    assert steps_g == steps == 4
    assert abs(ll_g - ll) <= 1e-12 * abs(ll) and np.max(np.abs(hist_g - hist)) <= 1e-12 * abs(ll)
    assert np.max(np.abs(mu_g - mu1)) <= 1e-11 * np.max(np.abs(mu1)) and np.max(np.abs(pi_g - pi1)) <= 1e-11
