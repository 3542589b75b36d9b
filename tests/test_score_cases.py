"""The held-out scoring cases of tests/test_gpu_score.py and what makes them fair cases, checked on the CPU: a mixture problem of
oracle/hp_cases.py, the parameters = the oracle's one EM step on the first half of the rows (ridge included), the scored block =
the second half. For every case
  * no row is near a tie: the two largest log-responsibilities of any row are further apart than any rounding error (the
    extended-precision values; the smallest gap of all cases is 4.2e-3, the bound here 1e-6: a tie would need the log-weights'
    ~1e-13 errors to be ten million times larger),
  * the oracle's labels are the extended-precision argmax on every row,
  * the reference's linear-domain density is a normal number on every row (log-density above -700; exp underflows at -745),
so the GPU tests compare EVERY row with the oracle and exclude none."""
import numpy as np
import pytest

from oracle import hp_cases, hp_reference as hp

# (d, K, N, offset): N not a multiple of 64, off-centre data, every tier of the scoring pass
SHAPES = [(2, 3, 3001, 5.0), (3, 4, 3001, 5.0), (4, 3, 3001, 3.0), (6, 4, 3001, 3.0), (8, 5, 3001, 3.0), (12, 5, 3001, 4.0),
          (16, 8, 4001, 2.0), (32, 16, 4001, 1.0), (33, 4, 3001, 0.0), (72, 2, 2501, 0.0), (128, 3, 2001, 0.0), (192, 2, 1501, 0.0)]
MIN_GAP = 1e-6


def held_out(orc, d, K, n, offset):
    """(scored block Y, mixing, means K x d, covariances K x d x d)."""
    X, pi0, mu0, S0 = hp_cases.problem(d, K, n, offset)
    half = n // 2
    em = orc.EM(K)
    em.set_parameters(mu0, S0, pi0)
    em.expectation_step(np.ascontiguousarray(X[:half]))
    em.maximisation_step(np.ascontiguousarray(X[:half]))
    return np.ascontiguousarray(X[half:]), em.mixing_probabilities.copy(), em.means.copy(), em.covariances.copy()


def oracle_labels(orc, Y, pi, mu, S, diagonal=False):
    """(labels, responsibilities) of the oracle's expectation_step + calculate_labels."""
    em = orc.EM(len(pi))
    if diagonal:
        em.set_covariance_type("diag")
    em.set_parameters(mu, S, pi)
    em.expectation_step(Y)
    em.calculate_labels()
    return np.asarray(em.labels).astype(np.uint32), em.responsibilities


def oracle_density_rows(orc, Y, pi, mu, S, rows, diagonal=False):
    """The oracle's log-density of single rows: expectation_step on the one-row block returns it as its log_likelihood."""
    em = orc.EM(len(pi))
    if diagonal:
        em.set_covariance_type("diag")
    em.set_parameters(mu, S, pi)
    out = np.empty(len(rows))
    for j, i in enumerate(rows):
        em.expectation_step(np.ascontiguousarray(Y[i:i + 1]))
        out[j] = em.log_likelihood
    return out


def sample_rows(n):
    """256 rows (all of them when there are fewer), the first and the last 64 among them."""
    if n <= 256:
        return np.arange(n)
    middle = np.linspace(64, n - 65, 128).astype(np.int64)
    return np.unique(np.concatenate([np.arange(64), middle, np.arange(n - 64, n)]))


def density_error(values, hp_values):
    """max_i |v_i - hp_i| / max(1, |hp_i|)."""
    ref = np.asarray(hp_values, dtype=hp.LD)
    return float((np.abs(np.asarray(values, dtype=hp.LD) - ref) / np.maximum(1, np.abs(ref))).max())


@pytest.mark.parametrize("d,K,n,offset", SHAPES)
def test_held_out_cases_have_no_near_ties_and_finite_densities(oracle, d, K, n, offset):
    Y, pi, mu, S = held_out(oracle, d, K, n, offset)
    lw = hp.log_weights(Y, pi, mu, S)                        # K x N, long double
    order = np.sort(lw, axis=0)
    gap = float((order[-1] - order[-2]).min())
    assert gap > MIN_GAP, gap
    labels, _ = oracle_labels(oracle, Y, pi, mu, S)
    assert np.array_equal(labels, lw.argmax(axis=0).astype(np.uint32))
    _, lse = hp._normalise(lw)
    assert np.all(np.isfinite(lse.astype(np.float64))) and float(lse.min()) > -700.0, float(lse.min())
    # the oracle's side of the density rule, for the record (2e-16 .. 5e-15 over these shapes)
    rows = sample_rows(len(Y))
    err_cpu = density_error(oracle_density_rows(oracle, Y, pi, mu, S, rows), lse[rows])
    print("score case d=%d K=%d: min gap %.3g, log-density %.1f .. %.1f, err_cpu %.3g" % (d, K, gap, float(lse.min()), float(lse.max()), err_cpu))
    assert err_cpu < 1e-13
