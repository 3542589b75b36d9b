"""Every route held to its own results when the data change units (tests/units_cases.py states the principle, the scalings and the
allowance U; tests/test_units_cases.py checks the inputs on the CPU). Needs a GPU: `timeout -k 10 1800 pytest tests/test_gpu_units.py -m gpu -s`.

Each case runs once at unit scale and once per scaling, on fresh handles, asserts the route it is written for (and that the scaled run
takes the same one, with the same `em_refine` launch count), then compares:

* BIT for bit after dividing by the powers of two (`tobytes()`, no tolerance): Data.shift and sample_covariance, the M-step from given
  responsibilities or labels, K-means (labels, counts, distances, inertia, centroids, the loop's steps) and the seeding calls under the
  uniform scalings, silhouette values, drawn samples, the conditioning maps and the Cholesky factor;
* within the allowance U: per-row log-densities (U), responsibilities (2 U), the log-likelihood (U), labels (equal on every row whose
  two largest unit-scale log-weights are more than 2 U apart), and the new parameters of an EM step to the tolerances
  tests/test_gpu_random_sweep.py holds them to (1e-11 mixing weights and means, 1e-9 covariances) -- a step is also held to the
  extended-precision reference on the SCALED input under tests/hp_limits.py's rules, the fp64 whitening restatement's error as the
  yardstick (the oracle's linear-domain determinant leaves the fp64 range at these scales). NOT held to that reference, only to their
  own unit-scale run: the weighted step (the reference has no weighted full-covariance form), the two loops and the restarts (the
  loops' U comes from the parameters their LAST E-step is called with, taken from the CPU restatement's trajectory);
* mixed units where nothing is covariant (K-means under M60): against the reference on the scaled input, as test_gpu_hp_error.py does.

Each comparison prints one `UNITS` line: the case, the scaling, the largest deviation, U (0: bit for bit). No limit comes from what a
kernel gave."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import estep_screen_cases as sc
import units_cases as uc
from oracle import hp_cases
from oracle import hp_reference as hp
from hp_limits import FLOOR, FOLD_BOUND, _check_kmeans, _errors, _fsum_centroids, _report_and_check

pytestmark = pytest.mark.gpu

LD = np.longdouble
SWITCHES = ("MLHIP_FUSED", "MLHIP_MSTATS_SPARSE", "MLHIP_ESTEP_FOLD", "MLHIP_SELF_NORM", "MLHIP_BIG_DIM", "MLHIP_ESTEP", "MLHIP_DIAG_AB",
            "MLHIP_TIED", "MLHIP_KMEANS", "MLHIP_RESIDENT", "MLHIP_SCORE", "MLHIP_SCORE_ROWS", "MLHIP_SILHOUETTE", "MLHIP_SAMPLE_TABLE",
            "MLHIP_EM_RESTARTS", "MLHIP_ESTEP_SCREEN", "MLHIP_CONDITION", "MLHIP_IMPUTE", "MLHIP_DEVICE_CLOSE")


@pytest.fixture(scope="module")
def ctx():
    from ml_amd import _lib
    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def _data(ctx, X, ridge=None, w=None):
    from ml_amd import _lib
    dt = _lib.Data(ctx, np.ascontiguousarray(X, dtype=np.float64))
    if w is not None:
        dt.set_weights(w)
    if ridge is not None:
        dt.set_covariance_ridge(ridge)
    return dt


def _launches(ctx, name):
    return ctx.timing_get(name)[1]


def _setenv(monkeypatch, env):
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def _assert_route(route, want):
    got = {k: route[k] for k in want}
    assert got == want, (got, want)


def _relerr(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, np.max(np.abs(b))))


def _line(case, scaling, deviation, U=0.0):
    print(f"UNITS {case} | {scaling} | largest deviation {deviation:.2e} | U {U:.2e}", flush=True)


def _bits_deviation(got, want):
    """Largest |got - want| relative to the largest |want| (0 when the bits agree): what the UNITS line of a bit-for-bit case shows."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if uc.same_bits(got, want):
        return 0.0
    with np.errstate(invalid="ignore"):
        return float(np.nanmax(np.abs(got - want)) / max(1e-300, float(np.nanmax(np.abs(want)))))


def _assert_bits(case, scaling, pairs):
    """pairs: (what, unscaled result, unit-scale result). Prints the line, then asserts tobytes() equality of every pair."""
    worst = max(_bits_deviation(g, w) for _, g, w in pairs)
    _line(case, scaling, worst)
    for what, g, w in pairs:
        assert uc.same_bits(g, w), (case, scaling, what, _bits_deviation(g, w))


# ---- Data.shift and sample_covariance -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("d,n", uc.DATA_SHAPES)
def test_data_statistics(ctx, d, n, weighted):
    X1 = hp_cases.problem(d, 1, n, 1.5)[0]
    w = uc.row_weights(n) if weighted else None

    def run(X):
        dt = _data(ctx, X, w=w)
        route = dt.em_route(1)
        out = (dt.shift,) + dt.sample_covariance()
        dt.close()
        return route, out

    route1, (shift1, mean1, cov1) = run(X1)
    _assert_route(route1, {"estep": {6: "scalar_fed", 33: "matrix4", 136: "big_dim"}[d]})
    for scaling in uc.SCALINGS:
        f = uc.factors(scaling, d)
        route, (shift, mean, cov) = run(uc.points(X1, f))
        assert route == route1
        _assert_bits(f"Data.shift + sample_covariance d={d} {'weighted' if weighted else 'plain'}", scaling,
                     [("shift", shift / f, shift1), ("mean", mean / f, mean1), ("covariance", cov / f[:, None] / f[None, :], cov1)])


# ---- M-step from given responsibilities / labels --------------------------------------------------------------------------------------

@pytest.mark.parametrize("d,K,n,env", uc.MSTEP_CASES, ids=[f"d{c[0]}-K{c[1]}" + ("-plain" if c[3] else "") for c in uc.MSTEP_CASES])
def test_mstep_from_given_responsibilities(ctx, monkeypatch, d, K, n, env):
    _setenv(monkeypatch, env)
    X1 = hp_cases.problem(d, K, n, 1.0)[0]
    R = uc.responsibilities(n, K, 100 * d + K)
    labels = R.argmax(axis=1).astype(np.uint32)

    def run(X, ridge):
        dt = _data(ctx, X, ridge=ridge)
        route = dt.em_route(K)
        ctx.timing_enable(True)
        ctx.timing_reset()
        soft = dt.em_maximisation_from(R)
        hard = dt.em_maximisation_from_labels(labels, K)
        counts = {name: _launches(ctx, name) for name in ("em_mstats", "em_refine")}
        ctx.timing_enable(False)
        dt.close()
        return route, counts, soft, hard

    units = {r: run(X1, r) for r in (uc.DEFAULT_RIDGE, 0.0)}
    route1 = units[0.0][0]
    _assert_route(route1, {"estep": ("plain" if env else "big_dim") if d > 128 else "matrix4" if d >= 16 else "scalar_fed"})
    for scaling in uc.SCALINGS:
        f = uc.factors(scaling, d)
        _, counts1, soft1, hard1 = units[uc.unit_ridge(scaling)]
        route, counts, soft, hard = run(uc.points(X1, f), uc.ridge(scaling))
        assert route == route1 and counts == counts1, (route, counts, counts1)
        pairs = []
        for what, got, want in (("responsibilities", soft, soft1), ("labels", hard, hard1)):
            pairs += [(what + ": mixing", got[0], want[0]), (what + ": means", got[1] / f, want[1]),
                      (what + ": covariances", got[2] / f[:, None] / f[None, :], want[2])]
        _assert_bits(f"M-step from given responsibilities d={d} K={K}" + (" plain tier" if env else ""), scaling, pairs)


# ---- K-means, uniform scalings: bit for bit -------------------------------------------------------------------------------------------

def _km_run(ctx, X, C0, steps=3, w=None):
    """One step on a fresh handle (with labels and distances), then the loop with atol 0 on another one."""
    dt = _data(ctx, X, w=w)
    route = dt.kmeans_route(len(C0))
    ctx.timing_enable(True)
    ctx.timing_reset()
    inertia, changed, counts, C1 = dt.kmeans_step(C0, weighted=w is not None)
    launches = _launches(ctx, "kmeans_assign")
    ctx.timing_enable(False)
    labels, dists = dt.kmeans_labels(), dt.kmeans_distances()
    dt.close()
    dt = _data(ctx, X, w=w)
    loop = dt.kmeans_iterate(C0, steps, 0.0, weighted=w is not None)
    loop_labels = dt.kmeans_labels()
    dt.close()
    return {"route": route, "launches": launches, "inertia": inertia, "changed": changed, "counts": counts, "C1": C1, "labels": labels,
            "dists": dists, "loop": loop, "loop_labels": loop_labels}


def _km_compare(case, scaling, got, unit, f):
    f2 = float(f[0]) ** 2
    assert got["route"] == unit["route"] and got["launches"] == unit["launches"]
    assert np.array_equal(got["labels"], unit["labels"]) and got["changed"] == unit["changed"]
    assert np.array_equal(got["loop_labels"], unit["loop_labels"])
    steps, conv, inertia, counts, cur, old = got["loop"]
    steps1, conv1, inertia1, counts1, cur1, old1 = unit["loop"]
    assert (steps, conv) == (steps1, conv1)
    _assert_bits(case, scaling, [("counts", got["counts"], unit["counts"]), ("distances", got["dists"] / f2, unit["dists"]),
                                 ("inertia", got["inertia"] / f2, unit["inertia"]), ("centroids", got["C1"] / f, unit["C1"]),
                                 ("loop inertia", inertia / f2, inertia1), ("loop counts", counts, counts1),
                                 ("loop centroids", cur / f, cur1), ("loop old centroids", old / f, old1)])


@pytest.mark.parametrize("name,shape,env,route", uc.KM_CASES, ids=[c[0] for c in uc.KM_CASES])
def test_kmeans_is_covariant(ctx, monkeypatch, name, shape, env, route):
    _setenv(monkeypatch, env)
    X1, C1 = uc.km_problem(shape)
    unit = _km_run(ctx, X1, C1)
    _assert_route(unit["route"], route)
    assert unit["launches"] == 1
    for scaling in uc.UNIFORM:
        f = uc.factors(scaling, shape[0])
        _km_compare("K-means " + name, scaling, _km_run(ctx, uc.points(X1, f), uc.points(C1, f)), unit, f)


def test_kmeans_lattice_ties_resolve_the_same_way(ctx):
    X1, C1 = uc.lattice_problem()
    unit = _km_run(ctx, X1, C1)
    _assert_route(unit["route"], {"kernel": "matrix", "pad": False})
    for scaling in uc.UNIFORM:
        f = uc.factors(scaling, X1.shape[1])
        _km_compare("K-means integer lattice d=8 K=256", scaling, _km_run(ctx, uc.points(X1, f), uc.points(C1, f)), unit, f)


def test_resident_kmeans_loop_is_covariant(ctx):
    X1, C1 = uc.km_problem(uc.KM_RESIDENT_SHAPE)

    def run(X, C0):
        dt = _data(ctx, X)
        route = dt.kmeans_route(len(C0))
        ctx.timing_enable(True)
        ctx.timing_reset()
        loop = dt.kmeans_iterate(C0, 3, 0.0)
        launches = (_launches(ctx, "kmeans_resident"), _launches(ctx, "kmeans_assign"))
        ctx.timing_enable(False)
        labels, dists = dt.kmeans_labels(), dt.kmeans_distances()
        dt.close()
        return route, launches, loop, labels, dists

    route1, launches1, loop1, labels1, dists1 = run(X1, C1)
    _assert_route(route1, {"kernel": "direct", "pad": False, "resident": True})
    assert launches1 == (1, 0) and loop1[0] == 3
    for scaling in uc.UNIFORM:
        f = uc.factors(scaling, 2)
        f2 = float(f[0]) ** 2
        route, launches, loop, labels, dists = run(uc.points(X1, f), uc.points(C1, f))
        assert route == route1 and launches == launches1 and loop[:2] == loop1[:2] and np.array_equal(labels, labels1)
        _assert_bits("K-means resident loop d=2 K=5, 3 steps", scaling,
                     [("inertia", loop[2] / f2, loop1[2]), ("counts", loop[3], loop1[3]), ("centroids", loop[4] / f, loop1[4]),
                      ("old centroids", loop[5] / f, loop1[5]), ("distances", dists / f2, dists1)])


def test_weighted_kmeans_step_is_covariant(ctx):
    shape = uc.KM_WEIGHTED_SHAPE
    X1, C1 = uc.km_problem(shape)
    w = uc.row_weights(shape[2])
    unit = _km_run(ctx, X1, C1, w=w)
    _assert_route(unit["route"], {"kernel": "matrix", "pad": False})
    for scaling in uc.UNIFORM:
        f = uc.factors(scaling, shape[0])
        _km_compare("K-means weighted step d=8 K=9", scaling, _km_run(ctx, uc.points(X1, f), uc.points(C1, f), w=w), unit, f)


# ---- K-means, mixed units: against the reference on the scaled input ------------------------------------------------------------------

@pytest.mark.parametrize("name,shape,env,route", uc.KM_MIXED_CASES, ids=[c[0] for c in uc.KM_MIXED_CASES])
def test_kmeans_in_mixed_units_against_the_reference(ctx, oracle, monkeypatch, name, shape, env, route):
    """Columns whose maxima lie up to 2^120 apart: every column on its own fixed-point grid. Held exactly as test_gpu_hp_error.py holds
    its K-means cases: labels on every row outside the margin, distances and inertia at the rounding level, update sums == math.fsum."""
    d, K, n = shape
    X, C0 = uc.km_problem(shape, "M60")
    s = uc.exponents("M60", d)
    assert s.max() - s.min() == 120
    ref = hp.kmeans_step(X, C0)
    km = oracle.KMeans(K)
    km.set_centroids(C0, n)
    km.assignment_step(X)
    _setenv(monkeypatch, env)
    dt = _data(ctx, X)
    _assert_route(dt.kmeans_route(K), route)
    got = dt.kmeans_step(C0)
    labels, dists = dt.kmeans_labels(), dt.kmeans_distances()
    dt.close()
    _line("K-means in mixed units " + name, "M60", hp.rel_err(dists, ref[0]), 4 * FLOOR)
    _check_kmeans("K-means M60 " + name, X, C0, got, labels, dists, ref, km)


# ---- seeding, uniform scalings --------------------------------------------------------------------------------------------------------

def _kpp(dt, centroid, first, u):
    from ml_amd import _lib
    index, certain, fixed = C.c_uint64(), C.c_int(), C.c_uint64()
    centroid = np.ascontiguousarray(centroid, dtype=np.float64)
    _lib.check(_lib.lib.mlhip_kpp_draw(dt.ctx.handle, dt.handle, _lib.dptr(centroid), int(first), C.c_double(u), C.c_uint64(0),
                                       C.byref(index), C.byref(certain), None))
    weights = np.empty(dt.n)
    _lib.check(_lib.lib.mlhip_kpp_weights(dt.ctx.handle, dt.handle, _lib.dptr(weights)))
    _lib.check(_lib.lib.mlhip_kpp_draw_fixed_point(dt.ctx.handle, dt.handle, _lib.dptr(centroid), int(first), C.c_double(u), C.c_uint64(0),
                                                   C.byref(fixed)))
    return index.value, certain.value, weights, fixed.value


@pytest.mark.parametrize("shape", [(5, 7, 3001), (16, 10, 3001)], ids=["d5", "d16"])
def test_seeding_is_covariant(ctx, shape):
    d = shape[0]
    X1, C1 = uc.km_problem(shape)
    uniforms = np.random.default_rng(9).random(4)

    def run(X, C0):
        dt = _data(ctx, X)
        msd = dt.min_squared_distances(C0[:3])
        draws, row = [], 17
        for t, u in enumerate(uniforms):                   # every draw's centroid is the row the draw before picked
            index, certain, weights, fixed = _kpp(dt, X[row], t == 0, float(u))
            draws.append((index, certain, fixed))
            last = weights
            row = int(fixed)
        dt.close()
        return msd, draws, last

    msd1, draws1, w1 = run(X1, C1)
    assert all(c == 1 for _, c, _ in draws1)               # (the device settled every draw: the comparison below is the kernels')
    for scaling in uc.UNIFORM:
        f = uc.factors(scaling, d)
        f2 = float(f[0]) ** 2
        msd, draws, w = run(uc.points(X1, f), uc.points(C1, f))
        assert draws == draws1, (draws, draws1)
        _assert_bits(f"seeding: min_squared_distances, kpp_weights, both draws d={d}", scaling,
                     [("min_squared_distances", msd / f2, msd1), ("kpp_weights", w / f2, w1)])


# ---- silhouette, uniform scalings -----------------------------------------------------------------------------------------------------

SILHOUETTE_CASES = [(d, n, False) for d, n in uc.SILHOUETTE_SHAPES] + [(d, n, True) for d, n in uc.SILHOUETTE_SHAPES if d <= 32]


@pytest.mark.parametrize("d,n,plain", SILHOUETTE_CASES, ids=[f"d{c[0]}-" + ("plain tier forced" if c[2] else "own tier") for c in SILHOUETTE_CASES])
def test_silhouette_is_invariant(ctx, monkeypatch, d, n, plain):
    from ml_amd import _lib
    if plain:
        monkeypatch.setenv("MLHIP_SILHOUETTE", "plain")
    X1 = hp_cases.problem(d, 4, n, 2.0)[0]
    labels = np.random.default_rng(d).integers(0, 4, n)

    def run(X):
        dt = _data(ctx, X)
        route = _lib.silhouette_route(dt)
        a, b, s = _lib.silhouette(dt, labels, parts=True)
        dt.close()
        return route, a, b, s

    route1, a1, b1, s1 = run(X1)
    assert route1 == ("plain" if plain or d > 32 else "registers")
    for scaling in uc.UNIFORM:
        f = float(uc.factors(scaling, d)[0])
        route, a, b, s = run(X1 * f)
        assert route == route1
        _assert_bits(f"silhouette d={d} {route1}" + (" (forced)" if plain else ""), scaling, [("a", a / f, a1), ("b", b / f, b1), ("s", s, s1)])


# ---- sampling, conditioning, factors: all four scalings -------------------------------------------------------------------------------

SAMPLE_CASES = [("lds_table", (8, 5), {}), ("global_table", (8, 5), {"MLHIP_SAMPLE_TABLE": "global"}), ("plain", (72, 2), {})]


@pytest.mark.parametrize("route,shape,env", SAMPLE_CASES, ids=[c[0] for c in SAMPLE_CASES])
def test_samples_are_covariant(ctx, monkeypatch, route, shape, env):
    from ml_amd import _lib
    _setenv(monkeypatch, env)
    d, K = shape
    _, pi, mu, S = hp_cases.problem(d, K, 1001, 1.0)
    pi = np.random.default_rng(3).dirichlet(np.full(K, 4.0))
    assert _lib.em_sample_route(d, K) == route
    X1, labels1 = ctx.em_sample(pi, mu, S, 1001, seed=7)
    for scaling in uc.SCALINGS:
        f = uc.factors(scaling, d)
        X, labels = ctx.em_sample(pi, uc.points(mu, f), uc.covariances(S, f), 1001, seed=7)
        assert np.array_equal(labels, labels1)
        _assert_bits(f"em_sample {route} d={d} K={K}", scaling, [("rows", X / f, X1)])


def test_conditioning_pieces_and_factors_are_covariant():
    from ml_amd import _lib
    d, K, observed = 8, 16, [6, 1, 3, 4]
    missing = [j for j in range(d) if j not in observed]
    _, pi, mu, S = hp_cases.problem(d, K, 1001, 1.0)
    mu_o1, S_oo1, A1, mu_m1 = _lib.em_condition(mu, S, observed)
    L1 = np.stack([_lib.cholesky_lower(S[k]) for k in range(K)])
    for scaling in uc.SCALINGS:
        f = uc.factors(scaling, d)
        fo, fm = f[observed], f[missing]
        mu_o, S_oo, A, mu_m = _lib.em_condition(uc.points(mu, f), uc.covariances(S, f), observed)
        L = np.stack([_lib.cholesky_lower(Sk) for Sk in uc.covariances(S, f)])
        _assert_bits("em_condition + mlhip_cholesky_lower d=8 dO=4 K=16", scaling,
                     [("means_observed", mu_o / fo, mu_o1), ("covs_observed", S_oo / fo[:, None] / fo[None, :], S_oo1),
                      ("maps", A / fm[:, None] * fo[None, :], A1), ("means_missing", mu_m / fm, mu_m1), ("cholesky", L / f[:, None], L1)])


# ---- within the allowance: the references of one (shape, scaling), computed once ------------------------------------------------------

def _ridge_off(S, ridge, diagonal=False):
    S = np.asarray(S, dtype=LD)
    return S - LD(ridge) if diagonal else S - LD(ridge) * np.eye(S.shape[-1], dtype=LD)


@functools.lru_cache(maxsize=None)
def _unit_log_weights(shape):
    X, pi0, mu0, S0 = uc.em_problem(shape)
    q = uc.whitened_q(X, mu0, S0)
    old = hp.conditioning(X.astype(LD).mean(axis=0), mu0, covs=S0)
    return q, uc.log_constants(pi0, S0) - 0.5 * q, float(old["fold"].max())


@functools.lru_cache(maxsize=None)
def _allowance(shape, scaling):
    """(U, the rows a label may differ on, sum ln f) from the CPU restatement (q has the unit-scale bits: tests/test_units_cases.py)."""
    d = shape[0]
    q, lw1, _ = _unit_log_weights(shape)
    _, pi0, _, S0 = uc.em_problem(shape, scaling)
    coef = uc.log_constants(pi0, S0)
    ln_f = uc.sum_ln_f(scaling, d)
    U = uc.allowance(d, coef, ln_f, np.abs(coef - 0.5 * q).max())
    return U, uc.undecided_rows(lw1, U), ln_f


@functools.lru_cache(maxsize=None)
def _scaled_references(shape, scaling):
    """The extended-precision step on the scaled input, the fp64 whitening restatement's errors against it, the new parameters' ratios."""
    X, pi0, mu0, S0 = uc.em_problem(shape, scaling)
    ref = hp.em_step(X, pi0, mu0, S0)
    e_cpu = _errors(hp_cases.whitened_step_fp64(X, pi0, mu0, S0)[:5], ref)
    ratio = hp.conditioning(X.astype(LD).mean(axis=0), ref[3], covs=ref[4])["ratio"]
    return ref, e_cpu, ratio


def _em_run(ctx, X, pi0, mu0, S0, ridge, w=None):
    K = len(pi0)
    dt = _data(ctx, X, ridge=ridge, w=w)
    route = dt.em_route(K)
    ctx.timing_enable(True)
    ctx.timing_reset()
    ll, pi1, mu1, S1 = dt.em_step(pi0, mu0, S0)
    launched = {name: _launches(ctx, name) for name in ("em_fused", "em_estep", "em_mstats", "em_refine")}
    ctx.timing_enable(False)
    resp, labels = dt.em_responsibilities(K), dt.em_labels(K)
    dt.close()
    return {"route": route, "launched": launched, "ll": ll, "pi": pi1, "mu": mu1, "S": S1, "resp": resp, "labels": labels}


def _compare_with_unit(case, scaling, got, unit, f, U, undecided, ln_f, second_scale):
    """The unit-scale comparison of one step: route and launch counts equal; ll within U, responsibilities within 2 U, labels on the
    decided rows, the parameters to test_gpu_random_sweep.py's tolerances."""
    assert got["route"] == unit["route"] and got["launched"] == unit["launched"], (got["route"], got["launched"], unit["launched"])
    assert undecided.mean() <= 1e-3
    e_ll = abs((got["ll"] + ln_f) - unit["ll"])
    e_resp = float(np.abs(got["resp"] - unit["resp"]).max()) if got.get("resp") is not None else 0.0
    e_pi, e_mu = _relerr(got["pi"], unit["pi"]), _relerr(got["mu"] / f, unit["mu"])
    e_S = _relerr(got["S"] / second_scale, unit["S"])
    print(f"UNITS {case} | {scaling} | largest deviation {max(e_ll, e_resp / 2):.2e} | U {U:.2e} | ll {e_ll:.2e} resp {e_resp:.2e} mixing "
          f"{e_pi:.2e} means {e_mu:.2e} covs {e_S:.2e} | rows left out {int(undecided.sum())}", flush=True)
    assert e_ll <= U and e_resp <= 2 * U, (case, scaling, e_ll, e_resp, U)
    if got.get("labels") is not None:
        assert np.array_equal(got["labels"][~undecided], unit["labels"][~undecided])
    assert e_pi <= 1e-11 and e_mu <= 1e-11 and e_S <= 1e-9, (case, scaling, e_pi, e_mu, e_S)


@pytest.mark.parametrize("name,shape,env,route", uc.EM_CASES, ids=[c[0] for c in uc.EM_CASES])
def test_em_step_under_a_change_of_units(ctx, monkeypatch, name, shape, env, route):
    _setenv(monkeypatch, env)
    d = shape[0]
    X1, pi0, mu1, S1 = uc.em_problem(shape)
    units = {r: _em_run(ctx, X1, pi0, mu1, S1, r) for r in (uc.DEFAULT_RIDGE, 0.0)}
    taken = units[0.0]["route"]
    _assert_route(taken, route)
    fold = taken["estep"] == "matrix4" and taken["fold_allowed"] and not taken["fused"] and _unit_log_weights(shape)[2] <= 64
    for scaling in uc.SCALINGS:
        f = uc.factors(scaling, d)
        X, _, mu0, S0 = uc.em_problem(shape, scaling)
        got = _em_run(ctx, X, pi0, mu0, S0, uc.ridge(scaling))
        U, undecided, ln_f = _allowance(shape, scaling)
        _compare_with_unit("EM step " + name, scaling, got, units[uc.unit_ridge(scaling)], f, U, undecided, ln_f, f[:, None] * f[None, :])
        ref, e_cpu, ratio = _scaled_references(shape, scaling)
        e_gpu = _errors((got["ll"], got["resp"], got["pi"], got["mu"], _ridge_off(got["S"], uc.ridge(scaling))), ref)
        above = ratio > 1e4
        assert got["launched"]["em_refine"] == int(above.sum()), (name, scaling, got["launched"], ratio)
        _report_and_check(f"{name} [{scaling}]", e_gpu, e_cpu, ratio, FOLD_BOUND if fold else None, "FOLD", abs(float(ref[0])), refined=above)


@pytest.mark.parametrize("exact", [False, True], ids=["two-operation form", "MLHIP_DIAG_AB=0"])
@pytest.mark.parametrize("shape", uc.DIAG_SHAPES, ids=[f"d{s[0]}-K{s[1]}" for s in uc.DIAG_SHAPES])
def test_diagonal_step_under_a_change_of_units(ctx, monkeypatch, shape, exact):
    if exact:
        monkeypatch.setenv("MLHIP_DIAG_AB", "0")
    d, K = shape[0], shape[1]
    X1, pi0, mu1, v1 = uc.em_problem(shape, None, diagonal=True)

    def run(X, mu0, v0, ridge):
        dt = _data(ctx, X, ridge=ridge)
        route = dt.em_route(K, "diag")
        ctx.timing_enable(True)
        ctx.timing_reset()
        ll, pi, mu, var = dt.em_step_diag(pi0, mu0, v0)
        launched = {name: _launches(ctx, name) for name in ("em_diag", "em_refine")}
        ctx.timing_enable(False)
        full = dt.em_route(K)
        resp, labels = dt.em_responsibilities(K), dt.em_labels(K)       # (rebuilt on demand by the full-covariance E-step of the shape)
        dt.close()
        return {"route": route, "full": full, "launched": launched, "ll": ll, "pi": pi, "mu": mu, "S": var, "resp": resp, "labels": labels}

    units = {r: run(X1, mu1, v1, r) for r in (uc.DEFAULT_RIDGE, 0.0)}
    _assert_route(units[0.0]["route"], {"diag_kernel": True, "diag_exact": exact})
    assert units[0.0]["launched"]["em_diag"] >= 1
    q1 = np.stack([(((X1 - mu1[k]) ** 2) / v1[k]).sum(axis=1) for k in range(K)], axis=1)
    lw1 = (np.log(pi0) - 0.5 * np.log(v1).sum(axis=1)) - 0.5 * q1
    # the responsibilities come from the full-covariance E-step: its FOLD form (section 4: 1e-13) where the route allows it and every
    # |W (mu - shift)| entry, W = diag(1 / sigma), is <= 64 -- a scale-free quantity
    full = units[0.0]["full"]
    reach = float(np.abs((mu1 - X1.mean(axis=0)) / np.sqrt(v1)).max())
    fold = full["estep"] == "matrix4" and full["fold_allowed"] and reach <= 64
    for scaling in uc.SCALINGS:
        f = uc.factors(scaling, d)
        X, _, mu0, v0 = uc.em_problem(shape, scaling, diagonal=True)
        coef = np.log(pi0) - 0.5 * np.log(v0).sum(axis=1)
        ln_f = uc.sum_ln_f(scaling, d)
        U = uc.allowance(d, coef, ln_f, np.abs(coef - 0.5 * q1).max())
        got = run(X, mu0, v0, uc.ridge(scaling))
        case = f"diagonal step d={d} K={K} {'exact form' if exact else 'two-operation form'}"
        _compare_with_unit(case, scaling, got, units[uc.unit_ridge(scaling)], f, U, uc.undecided_rows(lw1, U), ln_f, f * f)
        ref = hp.em_step_diag(X, pi0, mu0, v0)
        e_cpu = _errors(uc.diag_step_fp64(X, pi0, mu0, v0), ref)
        ratio = hp.conditioning(X.astype(LD).mean(axis=0), ref[3], variances=ref[4])["ratio"]
        assert got["full"] == full and got["launched"]["em_refine"] == int((ratio > 1e4).sum()), (got["launched"], ratio)
        e_resp = hp.abs_err(got["resp"], ref[1])
        resp_limit = 4 * max(e_cpu["resp"], FLOOR, FOLD_BOUND if fold else 0.0)
        print(f"UNITS {case} [{scaling}] responsibilities against the reference {e_resp:.2e} / restatement {e_cpu['resp']:.2e} | limit "
              f"{resp_limit:.2e} (FOLD: {fold})", flush=True)
        assert e_resp <= resp_limit, (case, scaling, e_resp, resp_limit)
        e_cpu = dict(e_cpu, resp=None)
        b = np.abs((mu1 - X1.mean(axis=0)) / np.sqrt(v1))                  # section 4's model of the two-operation form (scale-free)
        model = None if exact else hp.EPS64 * float(b.sum(axis=1).max())
        _report_and_check(f"{case} [{scaling}]", _errors((got["ll"], None, got["pi"], got["mu"], _ridge_off(got["S"], uc.ridge(scaling), True)), ref),
                          e_cpu, ratio, model, "2^-53 sum abs b", abs(float(ref[0])), refined=ratio > 1e4)


@pytest.mark.parametrize("tied_route", ["kernel", "composed"])
def test_tied_step_under_a_change_of_units(ctx, monkeypatch, tied_route):
    monkeypatch.setenv("MLHIP_TIED", tied_route)
    d, K, n = uc.TIED_SHAPE
    X1, pi0, mu1, S1 = uc.tied_problem()

    def run(X, mu0, S0, ridge):
        dt = _data(ctx, X, ridge=ridge)
        route = dt.em_tied_route(K)
        ctx.timing_enable(True)
        ctx.timing_reset()
        ll, pi, mu, S = dt.em_step_tied(pi0, mu0, S0)
        launched = {"em_refine": _launches(ctx, "em_refine")}
        ctx.timing_enable(False)
        resp, labels = dt.em_responsibilities(K), dt.em_labels(K)
        dt.close()
        return {"route": route, "launched": launched, "ll": ll, "pi": pi, "mu": mu, "S": S, "resp": resp, "labels": labels}

    units = {r: run(X1, mu1, S1, r) for r in (uc.DEFAULT_RIDGE, 0.0)}
    assert units[0.0]["route"] == tied_route
    q1 = uc.whitened_q(X1, mu1, np.stack([S1] * K))
    lw1 = uc.log_constants(pi0, np.stack([S1] * K)) - 0.5 * q1
    for scaling in uc.SCALINGS:
        f = uc.factors(scaling, d)
        X, _, mu0, S0 = uc.tied_problem(scaling)
        coef = uc.log_constants(pi0, np.stack([S0] * K))
        ln_f = uc.sum_ln_f(scaling, d)
        U = uc.allowance(d, coef, ln_f, np.abs(coef - 0.5 * q1).max())
        got = run(X, mu0, S0, uc.ridge(scaling))
        case = f"tied step d={d} K={K} {tied_route}"
        _compare_with_unit(case, scaling, got, units[uc.unit_ridge(scaling)], f, U, uc.undecided_rows(lw1, U), ln_f, f[:, None] * f[None, :])
        ref = hp.em_step_tied(X, pi0, mu0, S0)
        stack = lambda step: step[:4] + (np.asarray(step[4])[None],)   # noqa: E731
        e_cpu = _errors(stack(uc.tied_step_fp64(X, pi0, mu0, S0)), stack(ref))
        tratio = hp.tied_conditioning(X, X.astype(LD).mean(axis=0), mu0, S0, ref[4])["tratio"]
        _report_and_check(f"{case} [{scaling}]", _errors(stack((got["ll"], got["resp"], got["pi"], got["mu"], _ridge_off(got["S"], uc.ridge(scaling)))),
                                                          stack(ref)), e_cpu, np.array([tratio]))


def test_weighted_step_under_a_change_of_units(ctx):
    shape = (16, 8, 4001, 2.0)
    d = shape[0]
    w = uc.row_weights(shape[2])
    X1, pi0, mu1, S1 = uc.em_problem(shape)
    units = {r: _em_run(ctx, X1, pi0, mu1, S1, r, w=w) for r in (uc.DEFAULT_RIDGE, 0.0)}
    _assert_route(units[0.0]["route"], {"estep": "matrix4", "fused": False, "sparse": False, "resident": False})
    for scaling in uc.SCALINGS:
        f = uc.factors(scaling, d)
        X, _, mu0, S0 = uc.em_problem(shape, scaling)
        U, undecided, ln_f = _allowance(shape, scaling)
        _compare_with_unit("weighted EM step d=16 K=8", scaling, _em_run(ctx, X, pi0, mu0, S0, uc.ridge(scaling), w=w),
                           units[uc.unit_ridge(scaling)], f, U, undecided, ln_f, f[:, None] * f[None, :])


LOOP_CASES = [("resident loop d=2 K=3, 4 iterations", (2, 3, 3001, 0.0), 4, {"fused": True, "fused_form": "valu", "resident": True, "device_close": True},
               {"em_resident": 1, "em_fused": 0}),
              ("em_iterate d=16 K=8, 6 iterations", (16, 8, 4001, 2.0), 6, {"estep": "matrix4", "fused": False, "device_close": True, "resident": False}, None)]


@pytest.mark.parametrize("name,shape,steps,route,launches", LOOP_CASES, ids=[c[0] for c in LOOP_CASES])
def test_em_loop_under_a_change_of_units(ctx, name, shape, steps, route, launches):
    d, K = shape[0], shape[1]
    X1, pi0, mu1, S1 = uc.em_problem(shape)

    def run(X, mu0, S0, ridge):
        dt = _data(ctx, X, ridge=ridge)
        taken = dt.em_route(K)
        ctx.timing_enable(True)
        ctx.timing_reset()
        done, _, ll, pi, mu, S, hist = dt.em_iterate(pi0, mu0, S0, steps, 0.0, 0.0)
        launched = {name: _launches(ctx, name) for name in ("em_resident", "em_fused", "em_refine")}
        ctx.timing_enable(False)
        resp, labels = dt.em_responsibilities(K), dt.em_labels(K)
        dt.close()
        assert done == steps == len(hist)
        return {"route": taken, "launched": launched, "ll": ll, "pi": pi, "mu": mu, "S": S, "resp": resp, "labels": labels}

    units = {r: run(X1, mu1, S1, r) for r in (uc.DEFAULT_RIDGE, 0.0)}
    _assert_route(units[0.0]["route"], route)
    if launches:
        assert {k: units[0.0]["launched"][k] for k in launches} == launches
    # The compared log-likelihood and responsibilities are the LAST E-step's: U is formed from the parameters that E-step is called
    # with, the CPU restatement's after steps - 1 iterations (ridge as the library adds it), not from the starting ones.
    last = {}
    for r in (uc.DEFAULT_RIDGE, 0.0):
        pi, mu, S = pi0, mu1, S1
        for _ in range(steps - 1):
            _, _, pi, mu, S, _ = hp_cases.whitened_step_fp64(X1, pi, mu, S)
            S = S + r * np.eye(d)
        q = uc.whitened_q(X1, mu, S)
        last[r] = (pi, S, q, uc.log_constants(pi, S) - 0.5 * q)
    for scaling in uc.SCALINGS:
        f = uc.factors(scaling, d)
        X, _, mu0, S0 = uc.em_problem(shape, scaling)
        pi_t, S_t, q_t, lw_t = last[uc.unit_ridge(scaling)]
        coef = uc.log_constants(pi_t, uc.covariances(S_t, f))
        ln_f = uc.sum_ln_f(scaling, d)
        U = uc.allowance(d, coef, ln_f, np.abs(coef - 0.5 * q_t).max())
        undecided = uc.undecided_rows(lw_t, U)
        _compare_with_unit("EM " + name, scaling, run(X, mu0, S0, uc.ridge(scaling)), units[uc.unit_ridge(scaling)], f, U, undecided, ln_f,
                           f[:, None] * f[None, :])


def test_restarts_pick_the_same_winner(ctx, monkeypatch):
    monkeypatch.setenv("MLHIP_EM_RESTARTS", "batch")
    shape, R, steps = (2, 3, 3001, 0.0), 4, 3
    d, K = shape[0], shape[1]
    X1, pi0, mu1, S1 = uc.em_problem(shape)
    rng = np.random.default_rng(31)
    starts = np.stack([mu1 + 0.5 * r * rng.standard_normal(mu1.shape) for r in range(R)])

    def run(X, f, ridge):
        dt = _data(ctx, X, ridge=ridge)
        assert dt.em_route(K)["fused_form"] == "valu" and dt.em_restarts_route(K, R)[0] == "batched"
        ctx.timing_enable(True)
        ctx.timing_reset()
        restarts, best = dt.em_iterate_restarts(np.stack([pi0] * R), uc.points(starts, f), np.stack([uc.covariances(S1, f)] * R), steps, 0.0, 0.0)
        launched = {name: _launches(ctx, name) for name in ("em_restarts_pass", "em_refine")}
        ctx.timing_enable(False)
        dt.close()
        return restarts, best, launched

    # a condition on the data, from the CPU restatement: after `steps` iterations the best start leads the runner-up by far more than
    # any U (at 5 iterations all four starts have reached the same optimum and agree to 5e-15: no winner to compare)
    final = []
    for r in range(R):
        pi, mu, S = pi0, starts[r], S1
        for _ in range(steps):
            ll, _, pi, mu, S, _ = hp_cases.whitened_step_fp64(X1, pi, mu, S)
        final.append(ll)
    winner = int(np.argmax(final))
    assert np.sort(final)[-1] - np.sort(final)[-2] > 1e-3
    ones = np.ones(d)
    units = {r: run(X1, ones, r) for r in (uc.DEFAULT_RIDGE, 0.0)}
    assert units[0.0][1] == winner == units[uc.DEFAULT_RIDGE][1] and units[0.0][2]["em_restarts_pass"] >= 1
    for scaling in uc.SCALINGS:
        f = uc.factors(scaling, d)
        U, _, ln_f = _allowance(shape, scaling)
        restarts, best, launched = run(uc.points(X1, f), f, uc.ridge(scaling))
        restarts1, best1, launched1 = units[uc.unit_ridge(scaling)]
        assert launched == launched1, (launched, launched1)
        e_ll = max(abs((a[2] + ln_f) - b[2]) for a, b in zip(restarts, restarts1))
        _line(f"em_iterate_restarts R={R} batched d=2 K=3", scaling, e_ll, U)
        assert best == best1 and [a[0] for a in restarts] == [b[0] for b in restarts1] and [a[1] for a in restarts] == [b[1] for b in restarts1]
        assert e_ll <= U
        assert _relerr(restarts[best][4] / f, restarts1[best][4]) <= 1e-11 and _relerr(restarts[best][5] / f[:, None] / f[None, :], restarts1[best][5]) <= 1e-9


# ---- per-row log-densities: mlhip_em_score ----------------------------------------------------------------------------------------------

SCORE_CASES = [("scalar_fed", (8, 5, 3001, 3.0), {}), ("matrix4", (33, 4, 3001, 0.0), {}), ("composed", (16, 8, 4001, 2.0), {"MLHIP_SCORE": "composed"})]


@pytest.mark.parametrize("route,shape,env", SCORE_CASES, ids=[c[0] for c in SCORE_CASES])
def test_scores_under_a_change_of_units(ctx, monkeypatch, route, shape, env):
    _setenv(monkeypatch, env)
    d, K = shape[0], shape[1]

    def run(X, pi0, mu0, S0):
        dt = _data(ctx, X)
        taken = dt.em_score_route(K)
        dens, labels = dt.em_score(pi0, mu0, S0)
        ll = dt.em_expectation(pi0, mu0, S0)
        resp = dt.em_responsibilities(K)
        dt.close()
        return taken, dens, labels, ll, resp

    taken1, dens1, labels1, ll1, resp1 = run(*uc.em_problem(shape))
    assert taken1 == route
    for scaling in uc.SCALINGS:
        U, undecided, ln_f = _allowance(shape, scaling)
        taken, dens, labels, ll, resp = run(*uc.em_problem(shape, scaling))
        e_dens, e_ll, e_resp = float(np.abs((dens + ln_f) - dens1).max()), abs((ll + ln_f) - ll1), float(np.abs(resp - resp1).max())
        _line(f"em_score {route} + em_expectation d={d} K={K}", scaling, max(e_dens, e_ll, e_resp / 2), U)
        assert taken == taken1 and undecided.mean() <= 1e-3
        assert e_dens <= U and e_ll <= U and e_resp <= 2 * U, (e_dens, e_ll, e_resp, U)
        assert np.array_equal(labels[~undecided], labels1[~undecided])


# ---- the screened E-step ----------------------------------------------------------------------------------------------------------------

def test_screened_estep_under_a_change_of_units(ctx):
    """Three passes at d = 32, K = 64, N = 3000. Uniform scalings and M16: the same route counts as at unit scale. M60: the diagonal of
    W = L^-1 carries the columns' units, its ratio passes kMaxDiagRatio (device/em_screen_bound.hpp) and no pass is screened --
    correct, and recorded in DESIGN.md section 3.3p; only the bits and the route fields are asserted, the counts printed."""
    d, K, n = uc.SCREEN_SHAPE
    X1, p = sc.mixture(d, K, n, 5)
    passes = sc.three_passes(p)
    try:
        trail1 = sc.both(ctx, X1, passes)
        assert sc.routes(trail1) == sc.THREE
        dt = _data(ctx, X1[:64])
        route1 = dt.em_route(K)
        dt.close()
        _assert_route(route1, {"estep": "matrix4", "fused": False})
        for scaling in uc.SCALINGS:
            f = uc.factors(scaling, d)
            scaled = [(q[0], uc.points(q[1], f), uc.covariances(q[2], f)) for q in passes]
            trail = sc.both(ctx, uc.points(X1, f), scaled)               # (asserts screened == dense, bit for bit, at this scaling)
            dt = _data(ctx, uc.points(X1[:64], f))
            assert dt.em_route(K) == route1
            dt.close()
            print(f"UNITS screened E-step d={d} K={K} | {scaling} | largest deviation 0.00e+00 | U 0.00e+00 | (screened, dense, no_information) "
                  f"after each pass {sc.routes(trail)}", flush=True)
            if scaling != "M60":
                assert sc.routes(trail) == sc.routes(trail1) == sc.THREE
    finally:
        sc.set_screen(None)


# ---- conditioning: em_conditional_means and em_impute ------------------------------------------------------------------------------------

def test_conditional_means_and_impute_under_a_change_of_units(ctx):
    """d = 8, dO = 4, K = 16: values / f_M against the longdouble restatement of the UNIT-scale case under test_gpu_condition.py's rule,
    4 max(err_f64, FLOOR) + max_i sum_k dr |m_ik| / max |y|, with the responsibilities' 2 U as dr."""
    import condition_reference as ref
    from ml_amd import _lib
    key = (2, 8, 16, (6, 1, 3, 4), 321)
    c = ref.case(*key)
    d, K, observed = 8, 16, list(key[3])
    missing = ref.missing_of(d, observed)
    ld = c["ld"]
    err_f64 = ref.error(c["f64"]["y"], ld["y"])
    mu_o1, S_oo1, _, _ = _lib.em_condition(c["means"], c["covs"], observed)
    q1 = uc.whitened_q(c["X_observed"], mu_o1, S_oo1)
    for scaling in uc.SCALINGS:
        f = uc.factors(scaling, d)
        fo, fm = f[observed], f[missing]
        mu, S = uc.points(c["means"], f), uc.covariances(c["covs"], f)
        mu_o, S_oo, A, mu_m = _lib.em_condition(mu, S, observed)
        coef = uc.log_constants(c["mixing"], S_oo)
        ln_f = math.log(2.0) * int(uc.exponents(scaling, d)[observed].sum())
        U = uc.allowance(len(observed), coef, ln_f, np.abs(coef - 0.5 * q1).max())
        limit = 4 * max(err_f64, FLOOR) + float((2 * LD(U) * np.abs(ld["m"]).sum(axis=1)).max() / np.abs(ld["y"]).max())
        dt = _data(ctx, uc.points(c["X_observed"], fo))
        assert dt.em_condition_route(K, len(missing)) == "registers"
        y = dt.em_conditional_means(c["mixing"], mu_o, S_oo, A, mu_m)
        dt.close()
        holes = uc.points(c["X"], f)
        holes[:, missing] = np.nan
        assert _lib.em_impute_route(d, K) == "kernel"
        filled = _lib.em_impute(ctx, c["mixing"], mu, S, holes)
        assert uc.same_bits(filled[:, observed], holes[:, observed])
        e_y, e_fill = ref.error(y / fm, ld["y"]), ref.error(filled[:, missing] / fm, ld["y"])
        _line("em_conditional_means / em_impute d=8 dO=4 K=16", scaling, max(e_y, e_fill), limit)
        assert e_y <= limit and e_fill <= limit, (e_y, e_fill, limit)


# ---- the magnitudes found by reading ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d,K,kernel", [(2, 3, "direct"), (4, 20, "matrix")])
def test_kmeans_on_columns_whose_maximum_is_2_to_minus_1000(ctx, oracle, d, K, kernel):
    """Finite columns with max |x_j| = 2^-1000: the fixed-point scale 2^(94 - e_j) = 2^1093 is no double, so it is applied as two
    powers of two (runtime/kmeans.cpp). Every squared distance underflows to 0 in fp64, in the reference's loop too, so the first
    centroid wins every row; its new centroid is the exact sum of all rows, rounded once, over the count."""
    n = 1001
    rng = np.random.default_rng(1000 + d)
    X = rng.uniform(-1.0, 1.0, (n, d))
    X[rng.integers(0, n, d), np.arange(d)] = 1.0
    X = np.ascontiguousarray(np.ldexp(X, -1000))
    assert np.isfinite(X).all() and (np.abs(X).max(axis=0) == 2.0 ** -1000).all()
    C0 = X[rng.choice(n, K, replace=False)].copy()
    km = oracle.KMeans(K)
    km.set_centroids(C0, n)
    km.assignment_step(X)
    assert not np.asarray(km.labels).any() and km.inertia == 0.0
    dt = _data(ctx, X)
    _assert_route(dt.kmeans_route(K), {"kernel": kernel, "pad": False})
    inertia, changed, counts, C1 = dt.kmeans_step(C0)
    labels, dists = dt.kmeans_labels(), dt.kmeans_distances()
    dt.close()
    exact = _fsum_centroids(X, labels, K)
    _line(f"K-means, column maxima 2^-1000, {kernel} d={d} K={K}", "2^-1000", _bits_deviation(C1, exact))
    assert np.array_equal(labels, np.asarray(km.labels)) and inertia == 0.0 and not dists.any() and changed == n
    assert np.array_equal(counts, np.bincount(labels, minlength=K).astype(float))
    assert np.isfinite(C1).all() and uc.same_bits(C1, exact)
    dt = _data(ctx, X)                                         # the loop (d = 2: the resident kernel, which converts the sums itself)
    steps, conv, inertia, counts, cur, _ = dt.kmeans_iterate(C0, 2, 0.0)
    dt.close()
    assert (steps, conv, inertia) == (2, True, 0.0) and uc.same_bits(cur, exact)


def test_kmeans_padding_row_never_wins(ctx, oracle):
    """d = 4, K = 15 (one padding row in the matrix-core kernel's table), rows at 0, centroids of the size of 2^505: every score
    x . c - |c|^2 / 2 lies below the padding row's -2^1020 while every direct-form distance is finite. The exact phase calls a winner
    with index >= K ambiguous, so the full scan decides (device/kmeans_mfma.hip). Held to the extended-precision reference; the fp64
    inertia overflows, in the reference's own loop as well."""
    d, K, n = 4, 15, 70
    m = np.array([40, 38, 36, 34, 32, 30, 26, 28, 29, 31, 33, 35, 37, 39, 27], dtype=np.float64)
    C0 = np.ascontiguousarray(np.ldexp(np.outer(m, [1.0, -1.0, 1.0, 1.0]), 505))
    X = np.zeros((n, d))
    assert ((C0 * C0).sum(axis=1) / 2 > 2.0 ** 1020).all() and np.isfinite((C0 * C0).sum(axis=1)).all()
    dist, label, margin, _, ref_counts, _ = hp.kmeans_step(X, C0)
    assert (label == 6).all() and (margin > 64 * hp.EPS64 * dist).all()
    km = oracle.KMeans(K)
    km.set_centroids(C0, n)
    km.assignment_step(X)
    dt = _data(ctx, X)
    _assert_route(dt.kmeans_route(K), {"kernel": "matrix", "pad": False})
    inertia, _, counts, C1 = dt.kmeans_step(C0)
    labels, dists = dt.kmeans_labels(), dt.kmeans_distances()
    dt.close()
    e_dist = hp.rel_err(dists, dist)
    _line("K-means, a padding row holds the best score, d=4 K=15", "2^505", e_dist, 4 * FLOOR)
    assert np.array_equal(labels, label) and np.array_equal(labels, np.asarray(km.labels))
    assert e_dist <= 4 * FLOOR and np.array_equal(counts, ref_counts.astype(float))
    assert inertia == km.inertia == np.inf
    assert not C1.any()                                        # (the mean of rows at 0; an empty cluster's is the origin)
