"""The extended-precision reference (oracle/hp_reference.py) pinned against 50-digit arithmetic, the CPU oracle measured
against the reference at d = 2 ... 256 (its first independent pin above d = 32), and the comparison helper itself. CPU only.

Oracle bound: every output of one E + M step within  C_ORACLE * sqrt(N_k) * 2^-53 * kappa_k  of the
reference in section 4's norms (max-norm relative; per component for means and covariances with N_k = N pi_k and kappa_k =
|L_k|_inf |L_k^-1|_inf of the component's input covariance; N and the largest kappa for the log-likelihood, the mixing weights
and the responsibilities). C_ORACLE is 4 x the largest constant the oracle needed over CASES / DIAG_CASES in one CPU run
(the per-case figures are in DESIGN.md section 5 and oracle/README.md); `python tests/test_hp_reference.py` prints them."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import hp_reference as hp   # noqa: E402  (raises where long double is not extended precision: a failure, not a skip)
from oracle import hp_cases   # noqa: E402
from oracle.hp_cases import KMEANS_SHAPES, edge_problem, oracle_step, problem, refinement_problem   # noqa: E402

LD = np.longdouble
MP_LIMIT = hp.EPS64 / 64
C_ORACLE = 4 * 7.0        # measured: the largest constant over all cases is 6.99 (diagonal d = 7, K = 40: a component of ~15 samples,
                          # where sqrt(N_k) 2^-53 is close to the few roundings any route makes); DESIGN.md section 5


# ---- the reference against mpmath at 50 digits ---------------------------------------------------------------------------

def _mp_problem(d, K, n, seed, diagonal=False):
    rng = np.random.default_rng(seed)
    means = 1.5 * rng.standard_normal((K, d))
    comp = rng.integers(0, K, n)
    X = means[comp] + rng.standard_normal((n, d)) + 0.25
    mu0 = means + 0.3 * rng.standard_normal((K, d))
    pi0 = rng.uniform(0.5, 1.5, K)
    pi0 /= pi0.sum()
    if diagonal:
        S0 = rng.uniform(0.7, 1.6, (K, d))
    else:
        A = rng.standard_normal((K, d, d))
        S0 = np.stack([a @ a.T / d + np.eye(d) for a in A])
    return X, pi0, mu0, S0


def _mp_em_step(X, pi0, mu0, S0, diagonal):
    import mpmath as mp
    mp.mp.dps = 50
    n, d = X.shape
    K = len(pi0)
    x = [[mp.mpf(float(v)) for v in row] for row in X]
    lw = [[None] * K for _ in range(n)]
    for k in range(K):
        mu = [mp.mpf(float(v)) for v in mu0[k]]
        if diagonal:
            var = [mp.mpf(float(v)) for v in S0[k]]
            half_log_det = sum(mp.log(v) for v in var) / 2
        else:
            L = mp.cholesky(mp.matrix([[mp.mpf(float(v)) for v in row] for row in S0[k]]))
            half_log_det = sum(mp.log(L[j, j]) for j in range(d))
        for i in range(n):
            c = [x[i][j] - mu[j] for j in range(d)]
            if diagonal:
                q = sum(c[j] * c[j] / var[j] for j in range(d))
            else:
                y = []
                for j in range(d):
                    y.append((c[j] - sum(L[j, l] * y[l] for l in range(j))) / L[j, j])
                q = sum(v * v for v in y)
            lw[i][k] = mp.log(mp.mpf(float(pi0[k]))) - half_log_det - q / 2 - d * mp.log(2 * mp.pi) / 2
    resp = [[None] * K for _ in range(n)]
    ll = mp.mpf(0)
    for i in range(n):
        m = max(lw[i])
        total = sum(mp.exp(v - m) for v in lw[i])
        ll += m + mp.log(total)
        for k in range(K):
            resp[i][k] = mp.exp(lw[i][k] - m) / total
    s0 = [sum(resp[i][k] for i in range(n)) for k in range(K)]
    means = [[sum(resp[i][k] * x[i][j] for i in range(n)) / s0[k] for j in range(d)] for k in range(K)]
    if diagonal:
        second = [[sum(resp[i][k] * (x[i][j] - means[k][j]) ** 2 for i in range(n)) / s0[k] for j in range(d)] for k in range(K)]
    else:
        second = [[[sum(resp[i][k] * (x[i][a] - means[k][a]) * (x[i][b] - means[k][b]) for i in range(n)) / s0[k]
                    for b in range(d)] for a in range(d)] for k in range(K)]
    return ll / n, resp, [v / n for v in s0], means, second


def _mp_rel_err(got, ref):
    """max |got - ref| / max |ref| with the difference taken at 50 digits (a long double converts to mpmath exactly)."""
    import mpmath as mp
    got = np.asarray(got, dtype=LD).ravel()
    flat = ref
    while isinstance(flat, list) and flat and isinstance(flat[0], list):
        flat = [v for row in flat for v in row]
    if not isinstance(flat, list):
        flat = [flat]
    assert got.size == len(flat)
    as_mp = [mp.mpf(int(m * LD(2) ** 64)) * mp.mpf(2) ** (int(e) - 64) for m, e in (np.frexp(v) for v in got)]
    return float(max(abs(a - b) for a, b in zip(as_mp, flat)) / max(abs(b) for b in flat))


@pytest.mark.parametrize("d,K,n,seed,diagonal", [(2, 3, 60, 1, False), (3, 2, 47, 2, False), (6, 3, 60, 3, False), (5, 1, 33, 4, False),
                                                 (4, 3, 60, 5, True), (6, 2, 51, 6, True)])
def test_em_reference_against_50_digits(d, K, n, seed, diagonal):
    X, pi0, mu0, S0 = _mp_problem(d, K, n, seed, diagonal)
    got = (hp.em_step_diag if diagonal else hp.em_step)(X, pi0, mu0, S0)
    want = _mp_em_step(X, pi0, mu0, S0, diagonal)
    for name, g, w in zip(("log-likelihood", "responsibilities", "mixing", "means", "covariances"), got, want):
        err = _mp_rel_err(g, w)
        print(f"d={d} K={K} n={n} {name}: {err:.2e} (limit {MP_LIMIT:.2e})")
        assert err <= MP_LIMIT, name


def _mp_em_step_tied(X, pi0, mu0, S0, w):
    """em_step_tied at 50 digits: one factor, the covariance about the new means, a component of zero mass left out of it."""
    import mpmath as mp
    mp.mp.dps = 50
    n, d = X.shape
    K = len(pi0)
    x = [[mp.mpf(float(v)) for v in row] for row in X]
    wt = [mp.mpf(float(v)) for v in w]
    L = mp.cholesky(mp.matrix([[mp.mpf(float(v)) for v in row] for row in S0]))
    half_log_det = sum(mp.log(L[j, j]) for j in range(d))
    resp = [[None] * K for _ in range(n)]
    ll = mp.mpf(0)
    for i in range(n):
        lw = []
        for k in range(K):
            c = [x[i][j] - mp.mpf(float(mu0[k, j])) for j in range(d)]
            y = []
            for j in range(d):
                y.append((c[j] - sum(L[j, l] * y[l] for l in range(j))) / L[j, j])
            log_pi = mp.log(mp.mpf(float(pi0[k]))) if pi0[k] > 0 else mp.mpf("-inf")
            lw.append(log_pi - half_log_det - sum(v * v for v in y) / 2 - d * mp.log(2 * mp.pi) / 2)
        m = max(lw)
        e = [mp.exp(v - m) if v != mp.mpf("-inf") else mp.mpf(0) for v in lw]
        ll += wt[i] * (m + mp.log(sum(e)))
        resp[i] = [v / sum(e) for v in e]
    total = sum(wt)
    s0 = [sum(wt[i] * resp[i][k] for i in range(n)) for k in range(K)]
    live = [k for k in range(K) if s0[k] > 0]
    means = {k: [sum(wt[i] * resp[i][k] * x[i][j] for i in range(n)) / s0[k] for j in range(d)] for k in live}
    cov = [[sum(wt[i] * resp[i][k] * (x[i][a] - means[k][a]) * (x[i][b] - means[k][b]) for k in live for i in range(n)) / total
            for b in range(d)] for a in range(d)]
    return ll / total, resp, [v / total for v in s0], means, cov


@pytest.mark.parametrize("d,K,n,seed,weighted,zero", [(2, 3, 60, 31, False, None), (5, 2, 47, 32, False, None), (3, 3, 53, 33, True, None),
                                                      (4, 3, 60, 34, False, 1)])
def test_tied_reference_against_50_digits(d, K, n, seed, weighted, zero):
    X, pi0, mu0, S = _mp_problem(d, K, n, seed)
    S0 = S[0]
    w = np.random.default_rng(seed).integers(0, 4, n).astype(np.float64) if weighted else None
    if zero is not None:
        pi0[zero] = 0.0
        pi0 /= pi0.sum()
    got = hp.em_step_tied(X, pi0, mu0, S0, w)
    ll, resp, mixing, means, cov = _mp_em_step_tied(X, pi0, mu0, S0, np.ones(n) if w is None else w)
    live = sorted(means)
    assert live == [k for k in range(K) if k != zero]
    if zero is not None:                                   # the empty component: no mass, no mean, nothing in the covariance
        assert got[2][zero] == 0 and not got[1][:, zero].any() and np.isnan(got[3][zero].astype(np.float64)).all()
    for name, g, want in (("log-likelihood", got[0], ll), ("responsibilities", got[1], resp), ("mixing", got[2], mixing),
                          ("means", got[3][live], [means[k] for k in live]), ("covariance", got[4], cov)):
        err = _mp_rel_err(g, want)
        print(f"tied d={d} K={K} n={n} weighted={weighted} zero={zero} {name}: {err:.2e} (limit {MP_LIMIT:.2e})")
        assert err <= MP_LIMIT, name


@pytest.mark.parametrize("d,K,n,seed", [(2, 3, 60, 11), (5, 2, 41, 12), (6, 3, 57, 13)])
def test_kmeans_reference_against_50_digits(d, K, n, seed):
    import mpmath as mp
    mp.mp.dps = 50
    X, _, C0, _ = _mp_problem(d, K, n, seed)
    dist, label, margin, inertia, counts, new = hp.kmeans_step(X, C0)
    x = [[mp.mpf(float(v)) for v in row] for row in X]
    c = [[mp.mpf(float(v)) for v in row] for row in C0]
    D2 = [[sum((x[i][j] - c[k][j]) ** 2 for j in range(d)) for k in range(K)] for i in range(n)]
    want_label = [min(range(K), key=lambda k: D2[i][k]) for i in range(n)]
    assert list(label) == want_label
    want_dist = [D2[i][want_label[i]] for i in range(n)]
    want_margin = [min(D2[i][k] for k in range(K) if k != want_label[i]) - want_dist[i] for i in range(n)]
    assert _mp_rel_err(dist, want_dist) <= MP_LIMIT
    assert _mp_rel_err(margin, want_margin) <= MP_LIMIT
    assert _mp_rel_err(inertia, sum(want_dist)) <= MP_LIMIT
    assert list(counts) == [want_label.count(k) for k in range(K)] and min(counts) > 0
    want_new = [[sum(x[i][j] for i in range(n) if want_label[i] == k) / int(counts[k]) for j in range(d)] for k in range(K)]
    assert _mp_rel_err(new, want_new) <= MP_LIMIT
    assert _mp_rel_err(hp.min_squared_distances(X, C0), want_dist) <= MP_LIMIT
    # an empty cluster's centroid is the origin
    far = np.vstack([C0, np.full((1, d), 1e3)])
    out = hp.kmeans_step(X, far)
    assert out[4][K] == 0 and not out[5][K].any()


def test_moments_reference_against_50_digits():
    import mpmath as mp
    mp.mp.dps = 50
    X, _, _, _ = _mp_problem(5, 2, 50, 21)
    y = np.random.default_rng(22).standard_normal(50)
    x = [[mp.mpf(float(v)) for v in row] for row in X]
    mean = [sum(r[j] for r in x) / 50 for j in range(5)]
    cov = [[sum((r[a] - mean[a]) * (r[b] - mean[b]) for r in x) / 49 for b in range(5)] for a in range(5)]
    got_mean, got_cov = hp.sample_covariance(X)
    assert _mp_rel_err(got_mean, mean) <= MP_LIMIT and _mp_rel_err(got_cov, cov) <= MP_LIMIT
    xxt, xy = hp.xxt_xy(X, y)
    assert _mp_rel_err(xxt, [[sum(r[a] * r[b] for r in x) for b in range(5)] for a in range(5)]) <= MP_LIMIT
    assert _mp_rel_err(xy, [sum(r[a] * mp.mpf(float(v)) for r, v in zip(x, y)) for a in range(5)]) <= MP_LIMIT


def test_conditioning_quantities():
    shift = np.array([1.0, -2.0])
    means = np.array([[4.0, -2.0], [1.0, 6.0]])
    covs = np.stack([np.diag([0.25, 4.0]), np.diag([1.0, 16.0])])
    c = hp.conditioning(shift, means, covs=covs)
    assert np.allclose(c["ratio"], [36.0, 4.0]) and np.allclose(c["fold"], [6.0, 2.0]) and np.allclose(c["b2"], [36.0, 4.0])
    assert np.allclose(c["kappa"], [4.0, 4.0])
    v = hp.conditioning(shift, means, variances=np.array([[0.25, 4.0], [1.0, 16.0]]))
    assert np.allclose(v["ratio"], [36.0, 4.0]) and np.allclose(v["b2"], [36.0, 4.0]) and np.allclose(v["kappa"], [4.0, 4.0])


# ---- the oracle against the reference ------------------------------------------------------------------------------------

# (d, K, N, offset of the data from the origin); N never a multiple of 64
CASES = [(2, 3, 3001, 0.0), (3, 4, 3001, 5.0), (13, 5, 3001, 0.0), (16, 8, 4001, 0.0), (32, 16, 6001, 0.0), (33, 4, 3001, 0.0),
         (64, 4, 3001, 3.0), (72, 2, 2501, 0.0), (128, 3, 2001, 0.0), (256, 2, 1501, 0.0), (8, 5, 3001, 40.0)]
DIAG_CASES = [(4, 3, 3001, 0.0), (7, 40, 4001, 0.0), (16, 16, 4001, 2.0), (32, 8, 3001, 0.0)]


def step_errors(got, ref, kappa, n):
    """Per output: (error in section 4's norm, the unit sqrt(N_k) 2^-53 kappa_k it is bounded in), the worst component."""
    n_k = n * np.asarray(ref[2], dtype=np.float64)
    whole = np.sqrt(n) * hp.EPS64 * kappa.max()
    out = {"ll": (abs(float((LD(got[0]) - ref[0]) / ref[0])), whole),
           "resp": (hp.abs_err(got[1], ref[1]), whole),
           "mixing": (hp.rel_err(got[2], ref[2]), whole)}
    for name, i in (("means", 3), ("covs", 4)):
        per = [(hp.rel_err(got[i][k], ref[i][k]), np.sqrt(n_k[k]) * hp.EPS64 * kappa[k]) for k in range(len(n_k))]
        out[name] = max(per, key=lambda eu: eu[0] / eu[1])
    return out


def _oracle_case(d, K, n, offset, diagonal):
    from oracle import oracle_ctypes as orc
    X, pi0, mu0, S0 = problem(d, K, n, offset, diagonal)
    ref = (hp.em_step_diag if diagonal else hp.em_step)(X, pi0, mu0, S0)
    got = oracle_step(orc, X, pi0, mu0, S0, diagonal)
    cond = hp.conditioning(X.mean(axis=0), mu0, **({"variances": S0} if diagonal else {"covs": S0}))
    return step_errors(got, ref, cond["kappa"], n)


@pytest.mark.parametrize("d,K,n,offset", CASES)
def test_oracle_step_within_its_bound_of_the_reference(d, K, n, offset):
    for name, (err, unit) in _oracle_case(d, K, n, offset, False).items():
        print(f"d={d} K={K} N={n} offset={offset} {name}: err {err:.2e} = {err / unit:.3f} units of {unit:.2e}")
        assert err <= C_ORACLE * unit, name


@pytest.mark.parametrize("d,K,n,offset", DIAG_CASES)
def test_oracle_diagonal_step_within_its_bound_of_the_reference(d, K, n, offset):
    for name, (err, unit) in _oracle_case(d, K, n, offset, True).items():
        print(f"diag d={d} K={K} N={n} offset={offset} {name}: err {err:.2e} = {err / unit:.3f} units of {unit:.2e}")
        assert err <= C_ORACLE * unit, name


def test_oracle_kmeans_step_against_the_reference():
    from oracle import oracle_ctypes as orc
    for d, K, n in KMEANS_SHAPES:
        X, _, C0, _ = problem(d, K, n, 2.0)
        dist, label, margin, inertia, counts, new = hp.kmeans_step(X, C0)
        km = orc.KMeans(K)
        km.set_centroids(C0, n)
        km.assignment_step(X)
        safe = margin > 64 * hp.EPS64 * dist
        print(f"K-means d={d} K={K} N={n}: {int((~safe).sum())} rows within 64 * 2^-53 * dist of a tie")
        assert safe.mean() >= 0.999 and np.array_equal(km.labels[safe], label[safe])
        assert abs(float((LD(km.inertia) - inertia) / inertia)) <= np.sqrt(n) * hp.EPS64
        km.update_step(X)
        if safe.all():                                    # (the same labels, so the same sums: N_k terms each, kappa = 1)
            assert hp.rel_err(km.centroids, new) <= C_ORACLE * np.sqrt(counts.max()) * hp.EPS64

@pytest.mark.parametrize("d,diagonal,reach", [(16, False, 0.9 * 64), (32, False, 0.9 * 64), (16, False, 1.1 * 64), (32, False, 1.1 * 64),
                                              (16, True, 64 * 0.9 ** 0.5), (16, True, 64 * 1.1 ** 0.5)])
def test_edge_problems_sit_at_their_guard_with_overlapping_components(d, diagonal, reach):
    """The guard sweeps of tests/test_gpu_hp_error.py mean something only if the guarded quantity is where it is meant to be AND
    the outputs depend on the density form: hundreds of rows with responsibilities strictly inside (0, 1)."""
    X, pi0, mu0, S0 = edge_problem(d, reach, diagonal)
    cond = hp.conditioning(X.astype(LD).mean(axis=0), mu0, **({"variances": S0} if diagonal else {"covs": S0}))
    achieved = np.sqrt(cond["b2"].max()) if diagonal else cond["fold"].max()
    assert abs(achieved / reach - 1) < 1e-6, (achieved, reach)
    resp = (hp.em_step_diag if diagonal else hp.em_step)(X, pi0, mu0, S0)[1].astype(np.float64)
    assert (((resp > 1e-3) & (resp < 1 - 1e-3)).any(axis=1)).sum() >= 500


def test_refinement_problems_reach_their_ratio():
    for d in (4, 32):
        for target in (5e3, 9e3, 1.1e4):
            X, pi0, mu0, S0 = refinement_problem(d, target)
            ref = hp.em_step(X, pi0, mu0, S0)
            ratio = hp.conditioning(X.astype(LD).mean(axis=0), ref[3], covs=ref[4])["ratio"]
            assert abs(ratio.max() / target - 1) < 0.02, (d, target, ratio)


# ---- the tied-covariance cases of tests/test_gpu_tied_hp.py: what each one needs of its data --------------------------------

def test_tied_conditioning_quantities():
    X = np.array([[3.0, 0.0], [-3.0, 0.0], [0.0, 4.0], [0.0, -4.0]])
    means = np.array([[2.0, 0.0], [0.0, -8.0]])
    resp = np.array([[1.0, 0.0], [1e-7, 1.0], [0.5, 0.5], [0.0, 1.0]])
    c = hp.tied_conditioning(X, np.zeros(2), means, np.diag([1.0, 4.0]), np.diag([0.5, 2.0]), resp=resp)
    # T / N = diag(4.5, 8); m = (2, 0), (0, -4); y = (3, 0), (-3, 0), (0, 2), (0, -2)
    assert np.isclose(c["tratio"], 9.0) and np.isclose(c["reach"], 4.0)
    # pairs with r >= 1e-6: (0, 0): 1 * 5 = 5; (2, 0): 2 * 2 + 2 * 2 = 8; (1, 1): 3 * 3 + 4 * 4 = 25; (2, 1): 6 * 6 = 36; (3, 1): 2 * 6 = 12
    assert np.isclose(c["whiten"], 36.0)


@pytest.mark.parametrize("d,K", hp_cases.TIED_CODE_OBJECT_CASES)
def test_tied_code_object_cases_have_comparable_labels(d, K):
    """Labels are compared on the rows whose two largest reference responsibilities differ by more than 1e-9: at least 99.9 % of
    the rows must qualify, and on them the oracle's labels and responsibilities are the reference's."""
    from oracle import oracle_ctypes as orc
    X, pi0, mu0, S0 = hp_cases.tied_problem(d, K, hp_cases.TIED_N, 2.0, 2.5)
    ref = hp.em_step_tied(X, pi0, mu0, S0)
    top = np.sort(ref[1], axis=1)
    clear = (top[:, -1] - top[:, -2]) > 1e-9
    assert clear.mean() >= 0.999
    cpu = hp_cases.oracle_tied_step(orc, X, pi0, mu0, S0)
    assert np.array_equal(cpu[1].argmax(axis=1)[clear], ref[1].argmax(axis=1)[clear])
    assert hp.abs_err(cpu[1], ref[1]) <= 1e-12
    assert np.all(ref[2] > 0)


def test_tied_sweep_and_reach_cases_and_the_whitening_constant():
    """The conditioning sweep spans tratio 10 ... 1e5 and sends components of the composed route above the refinement guard; the
    reach cases sit below / above / far above 64 with >= 500 rows inside (1e-3, 1 - 1e-3); and C_WHITEN is the fp64 restatement's
    largest log-responsibility error in units of 2^-53 * whiten over all of them, rounded up."""
    worst, tratios = 0.0, []
    for offset, sep in hp_cases.TIED_SWEEP_CASES:
        X, pi0, mu0, S0 = hp_cases.tied_problem(8, 5, 3001, offset, sep)
        ref = hp.em_step_tied(X, pi0, mu0, S0)
        shift = X.astype(LD).mean(axis=0)
        tratios.append(hp.tied_conditioning(X, shift, mu0, S0, ref[4])["tratio"])
        ratio = hp.conditioning(shift, ref[3], covs=hp.m_step(X, ref[1])[2])["ratio"]
        ratio_w, whiten = hp_cases.tied_whitening_ratio(X, pi0, mu0, S0)
        print(f"tied sweep offset={offset} sep={sep}: tratio {tratios[-1]:.4g}, composed ratio max {ratio.max():.4g}, "
              f"{int((ratio > 1e4).sum())} above 1e4, whiten {whiten:.4g}, restatement {ratio_w:.3f} x 2^-53 whiten")
        assert (ratio.max() > 1e4) == (sep >= 300)
        worst = max(worst, ratio_w)
    assert 10 < tratios[0] < 20 and 1e3 < tratios[1] < 2e3 and tratios[2] > 1e5 and abs(tratios[3] / tratios[1] - 1) < 1e-9
    for reach in hp_cases.TIED_REACHES:
        X, pi0, mu0, S0 = hp_cases.tied_reach_problem(reach)
        ref = hp.em_step_tied(X, pi0, mu0, S0)
        cond = hp.tied_conditioning(X, X.astype(LD).mean(axis=0), mu0, S0, ref[4], resp=ref[1])
        soft = int(((ref[1] > 1e-3) & (ref[1] < 1 - 1e-3)).any(axis=1).sum())
        ratio_w, whiten = hp_cases.tied_whitening_ratio(X, pi0, mu0, S0)
        print(f"tied reach {reach}: achieved {cond['reach']:.4g}, {soft} soft rows, whiten {whiten:.4g}, restatement {ratio_w:.3f} x 2^-53 whiten")
        assert soft >= 500 and abs(cond["reach"] / reach - 1) < 0.05 and (cond["reach"] > 64) == (reach > 64)
        worst = max(worst, ratio_w)
    assert hp_cases.C_WHITEN - 1 < worst <= hp_cases.C_WHITEN, worst


def test_tied_edge_problems_hold_what_they_are_built_for():
    X, pi0, mu0, S0 = hp_cases.tied_edge_problem("zero_weight")
    ref = hp.em_step_tied(X, pi0, mu0, S0)
    assert pi0[2] == 0 and abs(pi0.sum() - 1) < 1e-15 and not ref[1][:, 2].any() and np.isfinite(float(ref[0]))
    X, pi0, mu0, S0 = hp_cases.tied_edge_problem("empty")
    ref = hp.em_step_tied(X, pi0, mu0, S0)
    L = np.linalg.cholesky(S0)
    assert np.linalg.norm(np.linalg.solve(L, (X - mu0[4]).T), axis=0).min() > 9.9e3
    assert not ref[1][:, 4].any() and ref[2][4] == 0 and np.all(ref[2][:4] > 0)            # exactly 0, in long double too
    assert np.isnan(ref[3][4].astype(np.float64)).all() and np.isfinite(ref[4].astype(np.float64)).all()
    X, pi0, mu0, S0 = hp_cases.tied_edge_problem("tail")
    dist = np.stack([np.linalg.norm(np.linalg.solve(L, (X - m).T), axis=0) for m in mu0], axis=1).min(axis=1)
    far = np.sort(dist)[-20:]
    assert np.all(np.abs(far - 40) < 1e-6) and np.sort(dist)[-21] < 10
    ref = hp.em_step_tied(X, pi0, mu0, S0)
    assert np.isfinite(float(ref[0])) and hp.abs_err(ref[1].sum(axis=1), np.ones(len(X))) < 1e-18


def test_tied_fp64_restatement_and_many_tile_shapes():
    """The fp64 yardstick of the longest many-tiles case agrees with the reference at a small size far inside
    tests/test_gpu_tied.py's tolerances, and on a 256-CU card every many-tiles shape gives a wave a third tile."""
    X, pi0, mu0, S0 = hp_cases.tied_problem(32, 40, 1501, 2.0, 2.5)
    ref = hp.em_step_tied(X, pi0, mu0, S0)
    got = hp_cases.tied_step_fp64(X, pi0, mu0, S0)
    assert abs(float((LD(got[0]) - ref[0]) / ref[0])) < 1e-14 and hp.abs_err(got[1], ref[1]) < 1e-13
    assert hp.rel_err(got[2], ref[2]) < 1e-13 and hp.rel_err(got[3], ref[3]) < 1e-13
    assert hp.rel_err(got[4] - 1e-15 * np.eye(32), ref[4]) < 1e-12
    for d, K, rows in ((3, 2, 262181), (21, 5, 131109), (32, 40, 65573)):
        grid = hp_cases.tied_grid(d, K, 2 ** 31, 256)
        n = hp_cases.tied_many_tiles_rows(d, K, 256)
        assert n == rows and (n + 63) // 64 > 2 * 4 * grid == 2 * 4 * hp_cases.tied_grid(d, K, n, 256)


# ---- the inputs of tests/test_gpu_hp_edges.py: what each kind needs of its data -----------------------------------------------

EDGE_CASES = ([(s, False) for s in hp_cases.EDGE_SHAPES + hp_cases.EDGE_LOOP_SHAPES] + [(s, True) for s in hp_cases.EDGE_DIAG_SHAPES])
EDGE_IDS = [f"d={s[0]}-K={s[1]}{'-diag' if dg else ''}" for s, dg in EDGE_CASES]


@pytest.mark.parametrize("shape,diagonal", EDGE_CASES, ids=EDGE_IDS)
@pytest.mark.parametrize("kind", hp_cases.MASSLESS_KINDS)
def test_massless_kinds_give_the_documented_pattern(kind, shape, diagonal):
    """Reference and oracle agree on the massless component -- responsibilities exactly 0 (in long double too), pi_k = 0, mu_k and
    Sigma_k / var_k NaN throughout, everything else finite --, the oracle's live part keeps its bound, and a `hole` sits at reach
    0 with the other components inside the guard of the fast density form."""
    from oracle import oracle_ctypes as orc
    d, K, n, _ = shape
    X, pi0, mu0, S0, k = hp_cases.massless_problem(kind, *shape, diagonal)
    live = np.array([j for j in range(K) if j != k])
    ref = (hp.em_step_diag if diagonal else hp.em_step)(X, pi0, mu0, S0)
    with np.errstate(all="ignore"):
        cpu = oracle_step(orc, X, pi0, mu0, S0, diagonal)
    assert not ref[1][:, k].any() and not np.asarray(cpu[1])[:, k].any()
    assert hp_cases.massless_pattern(ref, k) and hp_cases.massless_pattern(cpu, k)
    key = "variances" if diagonal else "covs"
    cond = hp.conditioning(X.astype(LD).mean(axis=0), mu0, **{key: S0})
    part = lambda s: (s[0], s[1], np.asarray(s[2])[live], np.asarray(s[3])[live], np.asarray(s[4])[live])   # noqa: E731
    for name, (err, unit) in step_errors(part(cpu), part(ref), cond["kappa"][live], n).items():
        print(f"{kind} d={d} K={K} diag={diagonal} {name}: err {err:.2e} = {err / unit:.3f} units of {unit:.2e}")
        assert err <= C_ORACLE * unit, name
    if kind == "far":
        assert cond["b2"][k] > 64.0 ** 2 and (diagonal or cond["fold"][k] > 64)
    if kind == "hole":
        reach = cond["b2"] if diagonal else cond["fold"]
        assert reach[k] <= 1e-9 and reach[live].max() <= (64.0 ** 2 if diagonal else 64.0)
        whiten = np.sqrt(S0[k].min()) if diagonal else np.sqrt(S0[k][0, 0])
        assert np.linalg.norm(X - X.mean(axis=0), axis=1).min() / whiten >= hp_cases.HOLE_UNITS * (1 - 1e-12)


@pytest.mark.parametrize("shape,diagonal", [c for c in EDGE_CASES if c[0] not in hp_cases.EDGE_LOOP_SHAPES],
                         ids=[i for c, i in zip(EDGE_CASES, EDGE_IDS) if c[0] not in hp_cases.EDGE_LOOP_SHAPES])
def test_tail_rows_are_decided_by_their_own_component(shape, diagonal):
    """Each moved row: won by the component it was moved behind, at a log-weight in (-900, -750) -- below the underflow of a
    linear-domain density, so the oracle's log-likelihood is not finite --, the runner-up at least TAIL_GAP = 8 below: an error
    delta in that row's log-weights moves a responsibility by at most e^-8 delta. The window is hp_cases.tail_window(d), the one
    the generator selects by: at d = 136 the density's constant -d/2 log 2 pi = -125 alone puts the same 40 whitened units at
    -943, and the window is (-950, -750) there. With K above the number of rows
    (diagonal K = 40) only the rows that meet this are moved, at least 8 of them."""
    from oracle import oracle_ctypes as orc
    d, K, n, _ = shape
    X, pi0, mu0, S0, rows, comps = hp_cases.tail_problem(*shape, diagonal, only_clear=K > hp_cases.TAIL_ROWS)
    assert len(rows) == hp_cases.TAIL_ROWS or (K > hp_cases.TAIL_ROWS and len(rows) >= 8)
    assert np.array_equal(comps, np.arange(hp_cases.TAIL_ROWS)[:len(comps)] % K) or K > hp_cases.TAIL_ROWS
    top, gap, winner = hp_cases.tail_row_margins(X[rows], pi0, mu0, S0, diagonal)
    print(f"tail d={d} K={K} diag={diagonal}: {len(rows)} rows, log-weight {top.min():.1f} .. {top.max():.1f}, smallest gap {gap.min():.3g}")
    assert hp_cases.tail_window(d) == ((-950.0, -750.0) if d == 136 else (-900.0, -750.0))
    assert all(hp_cases.tail_row_is_clear(k, t, g, w, d) for k, t, g, w in zip(comps, top, gap, winner))
    assert np.array_equal(winner, comps) and gap.min() >= hp_cases.TAIL_GAP
    L = hp_cases._factors(S0, diagonal)
    for row, k in zip(rows, comps):
        assert abs(np.linalg.norm(np.linalg.solve(L[k], X[row] - mu0[k])) - 40) < 1e-9
    with np.errstate(all="ignore"):
        assert not np.isfinite(oracle_step(orc, X, pi0, mu0, S0, diagonal)[0])
    ref = (hp.em_step_diag if diagonal else hp.em_step)(X, pi0, mu0, S0)
    assert np.isfinite(float(ref[0])) and hp.abs_err(ref[1].sum(axis=1), np.ones(n)) < 1e-18
    assert np.array_equal(ref[1][rows].argmax(axis=1), comps)


@pytest.mark.parametrize("shape", hp_cases.EDGE_WEIGHTED_SHAPES, ids=[f"d={s[0]}" for s in hp_cases.EDGE_WEIGHTED_SHAPES])
def test_zero_weight_rows_leave_a_live_component_without_weighted_mass(shape):
    from test_weights_cases import replicate, weights
    d, K, n, _ = shape
    X, w, pi0, mu0, S0, rows = hp_cases.zero_weight_rows_problem(*shape, weights(n))
    assert len(rows) == hp_cases.ZERO_ROWS and not w[rows].any() and np.array_equal(np.delete(w, rows), np.delete(weights(n), rows))
    block = hp.em_step(X, pi0, mu0, S0)
    assert np.all(block[1][rows, K - 1] == 1) and block[2][K - 1] > 0            # alive on the block ...
    ref = hp.em_step(replicate(X, w), pi0, mu0, S0)
    assert not ref[1][:, K - 1].any() and hp_cases.massless_pattern(ref, K - 1)   # ... exactly massless on the weighted sample


@pytest.mark.parametrize("d,first", hp_cases.MASSLESS_REFINEMENT_CASES)
def test_massless_refinement_problem_has_one_live_component_above_the_guard(d, first):
    from oracle import oracle_ctypes as orc
    X, pi0, mu0, S0, k = hp_cases.massless_refinement_problem(d, 1.1e4, first)
    assert pi0[k] == 0 and abs(pi0.sum() - 1) < 1e-15
    ref = hp.em_step(X, pi0, mu0, S0)
    with np.errstate(all="ignore"):
        assert hp_cases.massless_pattern(ref, k) and hp_cases.massless_pattern(oracle_step(orc, X, pi0, mu0, S0), k)
    live = [j for j in range(3) if j != k]
    ratio = hp.conditioning(X.astype(LD).mean(axis=0), ref[3][live], covs=ref[4][live])["ratio"]
    assert (ratio > 1e4).tolist() == [False, True] and abs(ratio[1] / 1.1e4 - 1) < 0.02, ratio


@pytest.mark.parametrize("kind,shape,diagonal", [("zero_weight_last", (16, 8, 4001, 2.0), False), ("zero_weight_first", (72, 2, 2501, 0.0), False),
                                                 ("zero_weight_last", (16, 8, 4001, 0.5), True), ("zero_weight_first", (8, 5, 3001, 3.0), False),
                                                 ("zero_weight_last", (2, 3, 3001, 0.0), False)])
def test_a_second_step_after_a_component_died_is_nan_throughout(kind, shape, diagonal):
    """What the loop cases of tests/test_gpu_hp_edges.py expect of two iterations: the oracle's second E-step meets log 0 + NaN in
    every row."""
    from oracle import oracle_ctypes as orc
    X, pi0, mu0, S0, k = hp_cases.massless_problem(kind, *shape, diagonal)
    em = orc.EM(len(pi0))
    if diagonal:
        em.set_covariance_type("diag")
    em.set_parameters(mu0, np.stack([np.diag(v) for v in S0]) if diagonal else S0, pi0)
    with np.errstate(all="ignore"):
        em.expectation_step(X)
        first = em.log_likelihood
        em.maximisation_step(X)
        em.expectation_step(X)
        second = em.log_likelihood
        em.maximisation_step(X)
    assert np.isfinite(first) and np.isnan(second)
    assert np.isnan(em.mixing_probabilities).all() and np.isnan(em.means).all() and np.isnan(em.covariances).all()


def test_edge_checkers_reject_fabricated_results():
    """The checkers of tests/test_gpu_hp_edges.py (tests/hp_limits.py) on results made up from the reference: the reference rounded
    to fp64 passes; the empty component's mean 0 instead of NaN, a NaN in a live component and a log-likelihood that lost one
    tail row's term do not."""
    from hp_limits import check_massless, check_tail, edge_references
    shape = (2, 3, 3001, 0.0)
    X, pi0, mu0, S0, k = hp_cases.massless_problem("zero_weight_last", *shape)
    refs = edge_references(X, pi0, mu0, S0, k, False)
    ref = refs["ref"]
    fp64 = lambda: [float(ref[0])] + [np.array(a, dtype=np.float64) for a in ref[1:]]   # noqa: E731
    labels = np.asarray(ref[1], dtype=np.float64).argmax(axis=1)
    check_massless("the reference in fp64", tuple(fp64()), labels, refs, 0)
    wrong = fp64()
    wrong[3][k] = 0.0
    with pytest.raises(AssertionError):
        check_massless("mean 0 for the empty component", tuple(wrong), labels, refs, 0)
    wrong = fp64()
    wrong[3][0, 1] = np.nan
    with pytest.raises(AssertionError):
        check_massless("NaN in a live component", tuple(wrong), labels, refs, 0)
    wrong = fp64()
    wrong[4][1, 0, 1] = np.nan
    with pytest.raises(AssertionError):
        check_massless("NaN in a live covariance", tuple(wrong), labels, refs, 0)
    wrong = fp64()
    wrong[1][5, k] = 1e-300
    with pytest.raises(AssertionError):
        check_massless("a responsibility of the empty component not exactly 0", tuple(wrong), labels, refs, 0)
    X, pi0, mu0, S0, rows, comps = hp_cases.tail_problem(*shape)
    refs = edge_references(X, pi0, mu0, S0, None, False)
    ref = refs["ref"]
    labels = np.asarray(ref[1], dtype=np.float64).argmax(axis=1)
    check_tail("the reference in fp64", tuple(fp64()), labels, refs, rows, comps, 0)
    lse = hp._normalise(hp.log_weights(X[rows[:1]], pi0, mu0, S0))[1]
    wrong = fp64()
    wrong[0] = float(ref[0] - lse[0] / len(X))
    with pytest.raises(AssertionError):
        check_tail("one tail row's term dropped", tuple(wrong), labels, refs, rows, comps, 0)
    wrong = fp64()
    wrong[0] = -np.inf
    with pytest.raises(AssertionError):
        check_tail("a log-sum-exp lost", tuple(wrong), labels, refs, rows, comps, 0)
    other = labels.copy()
    other[rows[0]] = (comps[0] + 1) % 3
    with pytest.raises(AssertionError):
        check_tail("a moved row with another label", tuple(fp64()), other, refs, rows, comps, 0)


# ---- ill-conditioned covariances: the inputs of tests/test_gpu_hp_ill.py, the whitening model's constants, the limit rule -------

ILL_CASES = [(shape, cond) for shape in hp_cases.ILL_SHAPES for cond in hp_cases.ILL_CONDS]
ILL_IDS = [f"d={s[0]}-K={s[1]}-cond={c:g}" for s, c in ILL_CASES]


@functools.lru_cache(maxsize=None)
def _ill_case(shape, cond):
    """The case's references (hp_limits.ill_references) and what the fp64 restatement needs on it: `needed`, the constant per output
    of one step, the per-row log-density (`lse`) and the second E-step's log-likelihood on its own new parameters (`ll2`)."""
    import hp_limits
    d, K, n = shape
    c = hp_limits.ill_references(d, K, n, cond)
    X, white = c["X"], c["white"]
    needed = hp_limits.ill_needed(c["e_white"], c["ref"], c["old"]["kappa"], c["new"]["ratio"], n)
    whole = np.sqrt(n) * hp.EPS64 * c["old"]["kappa"].max()
    e_lse = hp.abs_err(white[5], c["lse"])
    needed["lse"] = float(e_lse / whole) if e_lse > 4 * hp_limits.FLOOR else 0.0
    pi1, mu1, S1 = white[2], white[3], white[4] + 1e-15 * np.eye(d)             # (what the library hands to its next E-step)
    ref2 = hp._normalise(hp.log_weights(X, pi1, mu1, S1))[1].sum() / n
    e_ll2 = abs(float((LD(hp_cases.whitened_log_likelihood_fp64(X, pi1, mu1, S1)[0]) - ref2) / ref2))
    kappa1 = hp.conditioning(X.astype(LD).mean(axis=0), mu1, covs=S1)["kappa"]
    needed["ll2"] = float(e_ll2 / (np.sqrt(n) * hp.EPS64 * kappa1.max())) if e_ll2 > 4 * hp_limits.FLOOR else 0.0
    return dict(c, needed=needed, kappa1=kappa1)


def _ill_line(shape, cond, c):
    o = _ill_oracle_needed(c, shape[2])
    return (f"ill {shape} cond {cond:g} seed {hp_cases.ill_seed(*shape, cond)}: kappa {c['old']['kappa'].max():.3g}, max abs W(mu-s) "
            f"{c['old']['fold'].max():.4g}, new ratio {c['new']['ratio'].max():.3g} | units needed, whitening fp64 (oracle): "
            + ", ".join(f"{k} {v:.4f}" + (f" ({o[k]:.2f})" if k in o else "") for k, v in c["needed"].items()))


def _ill_oracle_needed(c, n):
    import hp_limits
    return hp_limits.ill_needed(c["e_oracle"], c["ref"], c["old"]["kappa"], c["new"]["ratio"], n)


@pytest.mark.parametrize("shape,cond", ILL_CASES, ids=ILL_IDS)
def test_ill_problems_hold_what_they_are_built_for_and_the_restatement_keeps_its_constants(shape, cond):
    """What tests/test_gpu_hp_ill.py needs of each input -- kappa ~ sqrt(cond), hundreds of rows with responsibilities strictly
    inside (0, 1), new covariances that factor and stay far below the refinement guard, max |W (mu - shift)| 5 % clear of the FOLD
    guard, at most 0.1 % of the rows too close for a label --, and what pins C_ILL: the fp64 restatement of the whitening form
    within C_ILL / 4 units on every output."""
    import hp_limits
    d, K, n = shape
    c = _ill_case(shape, cond)
    print(_ill_line(shape, cond, c))
    kappa = c["old"]["kappa"].max()
    assert np.sqrt(cond) / 2 <= kappa <= 40 * np.sqrt(cond), kappa
    resp = c["ref"][1].astype(np.float64)
    assert ((resp > 1e-3) & (resp < 1 - 1e-3)).any(axis=1).sum() >= 500
    for k in range(K):
        hp.cholesky(c["ref"][4][k])                                              # (raises where a new covariance does not factor)
    assert c["new"]["ratio"].max() < 1e3, c["new"]["ratio"]
    assert abs(c["old"]["fold"].max() / 64 - 1) > 0.05, c["old"]["fold"]
    assert hp_limits.ill_decided_rows(c["lw"], hp_limits.ill_row_limit(n, c["old"]["kappa"])).mean() >= 0.999
    for key, value in c["needed"].items():
        assert value <= hp_cases.C_ILL[key] / 4, (key, value)
    hp_limits.check_ill("the restatement", c["e_white"], c["ref"], c["old"]["kappa"], c["new"]["ratio"], n, False, c["e_white"], c["e_oracle"])


def test_ill_constants_are_the_restatement_s_and_the_limit_rejects_the_explicit_inverse_form():
    """C_ILL is 4 x the restatement's largest need, rounded up by no more than a third; and the limit has the teeth the oracle-relative
    rule lacks: with the oracle's step (explicit inverse covariance, error ~ cond * eps) in a kernel's place the responsibilities
    exceed it at cond = 1e8 on at least half of the shapes with d >= 6."""
    import hp_limits
    worst = {key: max(_ill_case(s, c)["needed"][key] for s, c in ILL_CASES) for key in hp_cases.C_ILL}
    print("largest constants the restatement needs:", ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    for key, value in worst.items():
        assert 0.75 * hp_cases.C_ILL[key] / 4 <= value <= hp_cases.C_ILL[key] / 4, (key, value)
    shapes = [s for s in hp_cases.ILL_SHAPES if s[0] >= 6]
    rejected = []
    for shape in shapes:
        c = _ill_case(shape, 1e8)
        limits = hp_limits.ill_limits(c["ref"], c["old"]["kappa"], c["new"]["ratio"], shape[2], False)
        if c["e_oracle"]["resp"] > limits["resp"]:
            rejected.append(shape)
    print(f"the oracle's responsibilities exceed the limit on {len(rejected)} of {len(shapes)} shapes: {rejected}")
    assert 2 * len(rejected) >= len(shapes)
    with pytest.raises(AssertionError):
        c = _ill_case(rejected[0], 1e8)
        hp_limits.check_ill("the oracle in a kernel's place", c["e_oracle"], c["ref"], c["old"]["kappa"], c["new"]["ratio"], rejected[0][2], False)


# ---- the comparison helper ------------------------------------------------------------------------------------------------

def test_comparison_helper_tells_a_lost_digit_from_rounding_noise():
    rng = np.random.default_rng(5)
    ref = (rng.standard_normal((7, 9)) + 3).astype(LD) * (1 + LD(2) ** -60)
    limit = 8 * hp.EPS64
    noisy = (ref * (1 + hp.EPS64 * rng.uniform(-1, 1, ref.shape))).astype(np.float64)
    assert not hp.over_limit(noisy, ref, limit)
    assert not hp.over_limit(ref.astype(np.float64), ref, limit)
    wrong = ref.astype(np.float64)
    worst = np.unravel_index(np.abs(ref).argmax(), ref.shape)
    wrong[worst] *= 1 + 1e-12
    assert hp.over_limit(wrong, ref, limit)
    for entry in [(0, 0), (6, 8), (3, 4)]:
        wrong = ref.astype(np.float64)
        wrong[entry] += 1e-12 * float(np.abs(ref).max())          # (the norm is relative to the largest entry)
        assert hp.over_limit(wrong, ref, limit), entry
    broken = ref.astype(np.float64)
    broken[2, 2] = np.nan
    assert hp.over_limit(broken, ref, limit) and hp.over_limit(ref[:, :8].astype(np.float64), ref, limit)
    assert hp.over_limit(np.array([1e-12]), np.array([0.0], LD), 1e-13, absolute=True)
    assert not hp.over_limit(np.array([1e-14]), np.array([0.0], LD), 1e-13, absolute=True)


if __name__ == "__main__":
    import time
    for diagonal, cases in ((False, CASES), (True, DIAG_CASES)):
        for case in cases:
            t = time.time()
            res = _oracle_case(*case, diagonal)
            print(("diag " if diagonal else "full ") + str(case), "%.1fs" % (time.time() - t),
                  " ".join(f"{k} {e:.1e} ({e / u:.3f})" for k, (e, u) in res.items()), flush=True)
    for shape, cond in ILL_CASES:
        print(_ill_line(shape, cond, _ill_case(shape, cond)), flush=True)
    print("C_ILL / 4:", {k: v / 4 for k, v in hp_cases.C_ILL.items()}, "largest needed:",
          {k: round(max(_ill_case(s, c)["needed"][k] for s, c in ILL_CASES), 4) for k in hp_cases.C_ILL})
