"""mlhip_em_impute, everything that needs no GPU: the argument errors of the three surfaces before any device work, the exported
symbols, the plan and route diagnostics (the route at d = 32 / 33 and under the switch; a launch count that does not grow with the
number of patterns), and the model surface without a device. CPU only."""
import numpy as np
import pytest

import impute_reference as imp


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in ("MLHIP_IMPUTE", "MLHIP_IMPUTE_ROWS", "MLHIP_IMPUTE_PATTERNS", "MLHIP_IMPUTE_GRID"):
        monkeypatch.delenv(name, raising=False)


def test_new_symbols_are_exported():
    from ml_amd import _lib
    from ml_amd.cppyml import clustering
    for name in ("mlhip_em_impute", "mlhip_em_impute_plan", "mlhip_em_impute_route", "mlhip_em_impute_condition", "mlpp_em_impute"):
        assert hasattr(_lib.lib, name), name
    for fn in (_lib.em_impute, _lib.em_impute_plan, _lib.em_impute_route, _lib.em_impute_condition, clustering.EM.impute):
        assert callable(fn)
    assert "`EM.impute`" in clustering.__doc__


def test_entry_points_check_their_arguments_without_a_device():
    from ml_amd import _lib
    C, lib, P, U = _lib.C, _lib.lib, _lib.dptr, _lib.u32ptr
    INVALID = _lib.E_INVALID_ARGUMENT
    a = np.zeros(16)
    obs = np.array([0], dtype=np.uint32)
    n4 = C.c_uint64(4)
    stand_in = C.create_string_buffer(8)
    fake = C.c_void_p(C.addressof(stand_in))                     # (only compared with NULL before the error is found)
    assert lib.mlhip_em_impute(None, 2, 2, 0, P(a), P(a), P(a), P(a), n4, P(a), None, None) == INVALID
    assert b"" != lib.mlhip_last_error()
    for bad in (dict(mixing=None), dict(means=None), dict(covs=None), dict(x=None), dict(out=None), dict(K=0), dict(d=0), dict(d=4097),
                dict(ctype=3), dict(ctype=-1), dict(n=C.c_uint64(2 ** 32))):
        g = dict(d=2, K=2, ctype=0, mixing=P(a), means=P(a), covs=P(a), x=P(a), n=n4, out=P(a))
        g.update(bad)
        assert lib.mlhip_em_impute(fake, g["d"], g["K"], g["ctype"], g["mixing"], g["means"], g["covs"], g["x"], g["n"], g["out"], None, None) == INVALID, bad
    k, launches, p = C.c_int(), C.c_uint64(), C.c_uint32()
    assert lib.mlhip_em_impute_route(2, 2, None, C.c_uint64(0), None, None) == INVALID
    assert lib.mlhip_em_impute_route(0, 2, None, C.c_uint64(0), C.byref(k), None) == INVALID
    assert lib.mlhip_em_impute_route(2, 2, None, n4, C.byref(k), C.byref(launches)) == INVALID
    assert lib.mlhip_em_impute_plan(P(a), n4, 2, None, None, None, None) == INVALID
    assert lib.mlhip_em_impute_plan(None, n4, 2, C.byref(p), None, None, None) == INVALID
    assert lib.mlhip_em_impute_plan(P(a), n4, 0, C.byref(p), None, None, None) == INVALID
    assert lib.mlhip_em_impute_plan(None, C.c_uint64(0), 2, C.byref(p), None, None, None) == _lib.OK and p.value == 0
    assert lib.mlhip_em_impute_condition(None, 2, 2, 0, P(a), P(a), P(a), U(obs), 1, P(a), P(a), P(a), P(a), P(a)) == INVALID
    assert lib.mlpp_em_impute(None, P(a), n4, 2, P(a), None, None) == INVALID
    for bad in (np.zeros((4, 2), dtype=np.float32), np.asfortranarray(np.zeros((4, 2))), np.zeros(4), [[0.0, 1.0]]):
        with pytest.raises(TypeError):
            _lib.em_impute(None, np.ones(1), np.zeros((1, 2)), np.eye(2)[None], bad)
        with pytest.raises(TypeError):
            _lib.em_impute_plan(bad)
    with pytest.raises(ValueError):
        _lib.em_impute(None, np.ones(1), np.zeros((1, 2)), np.eye(2)[None], np.zeros((4, 3)))


def test_plan_groups_the_rows_by_pattern():
    from ml_amd import _lib
    X = np.random.default_rng(1).standard_normal((300, 5))
    G = imp.bernoulli_gaps(X, 0.3, 2, complete=[0, 7], empty=[1, 9])
    order, bounds, n_observed = _lib.em_impute_plan(G)
    want = imp.groups(G)
    assert len(n_observed) == len(want) and sorted(order.tolist()) == list(range(300))
    for p, (observed, rows_of) in enumerate(want):
        assert np.array_equal(order[bounds[p]:bounds[p + 1]], rows_of) and n_observed[p] == len(observed)
    assert n_observed[0] == 0 and n_observed[-1] == 5
    # NaNs of another sign and payload mark the same gap
    H = G.copy()
    H.view(np.uint64)[np.isnan(G)] = np.uint64(0xfff8000000000123)
    assert all(np.array_equal(a, b) for a, b in zip(_lib.em_impute_plan(H), (order, bounds, n_observed)))
    for d in (33, 70):                                          # more than one mask word: the same rules
        W = imp.bernoulli_gaps(np.random.default_rng(d).standard_normal((65, d)), 0.05, 3, complete=[0], empty=[1])
        order, bounds, n_observed = _lib.em_impute_plan(W)
        seen = [tuple(np.isnan(W[i])) for i in order]
        starts = [i for i in range(65) if i == 0 or seen[i] != seen[i - 1]]
        assert starts == bounds[:-1].tolist() and len(set(seen)) == len(n_observed)


def test_route_by_dimension_and_switch(monkeypatch):
    from ml_amd import _lib
    assert _lib.em_impute_route(32, 3) == "kernel" and _lib.em_impute_route(2, 64) == "kernel" and _lib.em_impute_route(16, 1000) == "kernel"
    assert _lib.em_impute_route(33, 3) == "composed" and _lib.em_impute_route(4096, 3) == "composed"
    assert _lib.em_impute_route(1, 3) == "composed"            # (one coordinate: a row is complete or empty)
    monkeypatch.setenv("MLHIP_IMPUTE", "composed")
    assert _lib.em_impute_route(32, 3) == "composed"
    monkeypatch.setenv("MLHIP_IMPUTE", "kernel")
    assert _lib.em_impute_route(32, 3) == "kernel" and _lib.em_impute_route(33, 3) == "composed"   # (forced only where it exists)
    with pytest.raises(ValueError):
        _lib.em_impute_route(4097, 3)


def _block(n_patterns, rows_each, d=13):
    """n_patterns distinct patterns of one to four missing coordinates at d = 13 (1 092 exist): dO 9 .. 12 and dM 1 .. 4, one padding class."""
    rng = np.random.default_rng(n_patterns)
    masks = set()
    while len(masks) < n_patterns:
        m = np.zeros(d, dtype=bool)
        m[rng.choice(d, size=rng.integers(1, 5), replace=False)] = True
        masks.add(tuple(m))
    missing = np.repeat(np.array(sorted(masks), dtype=bool), rows_each, axis=0)
    return imp.with_gaps(rng.standard_normal(missing.shape), missing)


def test_kernel_launches_do_not_grow_with_the_patterns(monkeypatch):
    """3 and 300 patterns that use the same padding class (dO 9 .. 12 -> 16, dM 1 .. 4 -> 4 at d = 13): the kernel route makes the same
    number of launches -- one records launch and one evaluation launch --, the composed route two per pattern."""
    from ml_amd import _lib
    few, many = _block(3, 5), _block(300, 5)
    assert len(_lib.em_impute_plan(few)[2]) == 3 and len(_lib.em_impute_plan(many)[2]) == 300
    assert _lib.em_impute_route(13, 3, few) == ("kernel", 2) and _lib.em_impute_route(13, 3, many) == ("kernel", 2)
    monkeypatch.setenv("MLHIP_IMPUTE_PATTERNS", "100")          # the pattern chunk: one records and one evaluation launch per chunk
    assert _lib.em_impute_route(13, 3, many) == ("kernel", 6)
    monkeypatch.delenv("MLHIP_IMPUTE_PATTERNS")
    monkeypatch.setenv("MLHIP_IMPUTE", "composed")
    assert _lib.em_impute_route(13, 3, few) == ("composed", 6) and _lib.em_impute_route(13, 3, many) == ("composed", 600)


def test_impute_raises_before_device_work_and_needs_a_device():
    from ml_amd import _lib
    from ml_amd.cppyml import clustering
    fresh = clustering.EM(2)
    with pytest.raises(ValueError):                               # before a fit
        fresh.impute(np.zeros((10, 3)))
    em = clustering.EM(2)
    assert em.fit(np.array([[0.0, 1.0, 2.0], [3.0, 5.0, 4.0]]))  # N == K: the exact fit needs no device
    Y = np.zeros((10, 3))
    Y[::2, 1] = np.nan
    for bad in (Y.astype(np.float32), np.asfortranarray(Y), Y[:, 0], Y.tolist()):
        with pytest.raises(TypeError):
            em.impute(bad)
    for bad in (np.zeros((10, 2)), np.zeros((10, 4))):
        with pytest.raises(ValueError):
            em.impute(bad)
    if _lib.device_count() > 0:
        return                                                   # (the rest is what happens WITHOUT a GPU; tests/test_gpu_impute.py has the other side)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        em.impute(Y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        em.impute(np.zeros((0, 3)), return_log_density=True, return_responsibilities=True)
    with pytest.raises(_lib.NoDeviceError):
        _lib.Context()
