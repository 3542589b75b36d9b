"""The conditioning calls share one chunked pass (ml_amd/csrc/runtime/em_condition.cpp): the marginal mixture's E-step per chunk, the
call's own kernel behind it, the log-density from the E-step's log-sum-exp. What that sharing promises, stated once across all of
them: on the same block the mean that mlhip_em_conditional_variances (both forms), mlhip_em_conditional_cdfs and
mlhip_em_conditional_quantiles return has the bits of mlhip_em_conditional_means, every log_density has the bits of every other, and a
2-shard device group gives the bits of the single context.

One model of K = 3 components, (dO, dM) = (3, 2) on the register tier and (33, 2) on the plain tier, under MLHIP_CONDITION_ROWS=64.
The switch is rounded UP to whole sample tiles of 256 rows (route.cpp), so a chunk holds 256 rows: n = 130 is one chunk, and n = 514
is the three chunks with a last one of 2 rows (a shard of the group then holds 257 rows: two chunks, the last of 1 row). The
launches per call are counted, so the chunks are what this says. Device against device, bit for bit: no reference and no tolerance.
The per-call tests hold each call to its definition."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SWITCHES = ("MLHIP_CONDITION", "MLHIP_CONDITION_ROWS", "MLHIP_CONDITION_SKIP", "MLHIP_CONDITION_GROUP", "MLHIP_SCORE", "MLHIP_SCORE_ROWS")
K, ROWS, TILE = 3, 64, 256                                      # (TILE: kSampleTile, ml_amd/csrc/device/layout.hpp)
SIZES = (130, 514)
N = max(SIZES)
SHAPES = {"registers": (3, 2), "plain": (33, 2)}
PROBABILITIES = (0.05, 0.5, 0.999)


@pytest.fixture(scope="module")
def ctx():
    from ml_amd import _lib
    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _condition_rows_of_64(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("MLHIP_CONDITION_ROWS", str(ROWS))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


_CASES = {}


def case(tier):
    """The model conditioned by the library's own host helpers (held by the host tests), the block of N rows and the CDF's values; once
    a tier."""
    from ml_amd import _lib
    if tier not in _CASES:
        dO, dM = SHAPES[tier]
        d = dO + dM
        rng = np.random.default_rng(7 + d)
        means = 2.0 * rng.standard_normal((K, d))
        roots = rng.standard_normal((K, d, d)) / np.sqrt(d)
        covs = roots @ roots.transpose(0, 2, 1) + 0.5 * np.eye(d)
        mixing = np.array([0.5, 0.3, 0.2])
        observed = np.arange(dO, dtype=np.uint32)
        labels = rng.integers(0, K, N)
        X = means[labels] + np.einsum("nij,nj->ni", np.linalg.cholesky(covs)[labels], rng.standard_normal((N, d)))
        conditioned = _lib.em_condition(means, covs, observed)
        C_m, _ = _lib.em_condition_covariances(covs, observed)
        _CASES[tier] = dict(mixing=mixing, conditioned=conditioned, C_m=C_m, scales=_lib.em_condition_scales(C_m),
                            X=np.ascontiguousarray(X[:, :dO]), values=np.ascontiguousarray(X[:, dO:]))
    return _CASES[tier]


def every_call(context, tier, n, count_launches=False):
    """name -> (mean, log_density) of every call on one handle of `context` over the block's first n rows, 'means' first; the routes
    are the tier's."""
    from ml_amd import _lib
    c = case(tier)
    dM = SHAPES[tier][1]
    mixing, cond, C_m, scales = c["mixing"], c["conditioned"], c["C_m"], c["scales"]
    X, values = np.ascontiguousarray(c["X"][:n]), np.ascontiguousarray(c["values"][:n])
    data = _lib.Data(context, X)
    try:
        assert data.em_condition_route(K, dM) == tier
        assert _lib.em_condition_variance_route(data, K, dM, False) == tier and _lib.em_condition_variance_route(data, K, dM, True) == tier
        assert _lib.em_condition_quantile_route(data, K, dM, False) == tier and _lib.em_condition_quantile_route(data, K, dM, True) == tier
        if count_launches:
            context.timing_enable(True)
            context.timing_reset()
        out = {"means": data.em_conditional_means(mixing, *cond, log_density=True)}
        out["variances"] = _lib.em_conditional_variances(data, mixing, *cond, C_m, means=True, log_density=True)[1:]
        out["variances_full"] = _lib.em_conditional_variances(data, mixing, *cond, C_m, full=True, means=True, log_density=True)[1:]
        out["cdfs"] = _lib.em_conditional_cdfs(data, mixing, *cond, *scales, values, means=True, log_density=True)[1:]
        out["quantiles"] = _lib.em_conditional_quantiles(data, mixing, *cond, *scales, PROBABILITIES, means=True, log_density=True)[1:]
        if count_launches:
            chunks = -(-n // (-(-ROWS // TILE) * TILE))
            for name in ("em_condition", "em_condition_variance", "em_condition_cdf", "em_condition_quantile"):
                launches = context.timing_get(name)[1]
                assert launches == (2 * chunks if name == "em_condition_variance" else chunks), (name, launches)
            assert context.timing_get("em_estep")[1] == 5 * chunks
    finally:
        if count_launches:
            context.timing_enable(False)
        data.close()
    for y, dens in out.values():
        assert y.shape == (n, dM) and dens.shape == (n,) and np.isfinite(y).all() and np.isfinite(dens).all()
    return out


_SINGLE = {}


def single(ctx, tier, n):
    if (tier, n) not in _SINGLE:
        _SINGLE[tier, n] = every_call(ctx, tier, n, count_launches=True)
    return _SINGLE[tier, n]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("tier", sorted(SHAPES))
def test_every_call_returns_the_mean_and_the_log_density_of_conditional_means(ctx, tier, n):
    out = single(ctx, tier, n)
    y, dens = out["means"]
    for name, (y_call, dens_call) in out.items():
        assert np.array_equal(bits(y_call), bits(y)), name
        assert np.array_equal(bits(dens_call), bits(dens)), name


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("tier", sorted(SHAPES))
def test_a_two_shard_group_gives_the_same_bits_in_every_call(ctx, tier, n):
    from ml_amd import _lib
    y, dens = single(ctx, tier, n)["means"]
    group = _lib.Context.group(2, device_ids=[0, 0])
    try:
        grouped = every_call(group, tier, n)
    finally:
        group.close()
    for name, (y_call, dens_call) in grouped.items():
        assert np.array_equal(bits(y_call), bits(y)), name
        assert np.array_equal(bits(dens_call), bits(dens)), name
