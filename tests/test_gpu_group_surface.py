"""The entry points that reach a device group only through the facade elsewhere in the suite, called on a group directly and held to a
single context on the same block: mlhip_xxt_xy, mlhip_random_partition_means, mlhip_kpp_draw + mlhip_kpp_weights,
mlhip_min_squared_distances, mlhip_timing_get; mlhip_em_step with outputs that alias its inputs; a row range of responsibilities
that starts in one shard and ends in the next; and argument errors, which a group must report as a single context does and survive.
Two shapes: N = 1000, d = 5 over three shards (334 / 333 / 333 rows) and N = 5, d = 2 over eight (five shards of one row, three
empty). All shards sit on GPU 0."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 3


def relerr(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, np.max(np.abs(b)))


@pytest.fixture(scope="module", params=[(1000, 5, 3), (5, 2, 8)], ids=["1000x5-3shards", "5x2-8shards"])
def pair(request):
    """(group's block, single context's block, X, a parameter set) -- one upload per shape for the whole module."""
    from ml_amd import _lib
    n, d, shards = request.param
    rng = np.random.default_rng(1000 * n + d)
    X = np.ascontiguousarray(rng.standard_normal((n, d)) + 3.0 * rng.integers(0, K, (n, 1)))
    X.setflags(write=False)
    params = (np.full(K, 1.0 / K), X[:K] + 0.1, np.broadcast_to(np.cov(X.T) + np.eye(d), (K, d, d)).copy())
    group, single = _lib.Context.group(shards, device_ids=[0] * shards), _lib.Context()
    g, s = _lib.Data(group, X), _lib.Data(single, X)
    rows = [g.shard_rows(i)[1] for i in range(shards)]
    assert rows == ([334, 333, 333] if shards == 3 else [1, 1, 1, 1, 1, 0, 0, 0])
    yield g, s, X, params
    g.close(); s.close(); group.close(); single.close()


def _xxt_xy(data, y):
    from ml_amd import _lib
    xxt, xy = np.empty((data.d, data.d)), np.empty(data.d)
    _lib.check(_lib.lib.mlhip_xxt_xy(data.ctx.handle, data.handle, _lib.dptr(y), _lib.dptr(xxt), _lib.dptr(xy)))
    return xxt, xy


def test_xxt_xy(pair):
    g, s, X, _ = pair
    y = np.random.default_rng(2).standard_normal(g.n)
    (xxt_g, xy_g), (xxt_s, xy_s) = _xxt_xy(g, y), _xxt_xy(s, y)
    # (the bounds test_gpu_group.py holds sample_covariance to: 1e-12 for its vector, 1e-11 for its matrix)
    assert relerr(xy_g, xy_s) < 1e-12 and relerr(xxt_g, xxt_s) < 1e-11


def _random_partition_means(data, draws):
    from ml_amd import _lib
    order = np.argsort(draws, kind="stable").astype(np.uint32)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(draws, minlength=K))]).astype(np.uint32)
    means, sizes = np.zeros((K, data.d)), np.zeros(K)
    _lib.check(_lib.lib.mlhip_random_partition_means(data.ctx.handle, data.handle, K, _lib.u32ptr(order), _lib.u32ptr(offsets),
                                                     _lib.dptr(means), _lib.dptr(sizes)))
    return means, sizes


def test_random_partition_means_is_bit_identical(pair):
    g, s, X, _ = pair
    draws = np.random.default_rng(3).integers(0, K, g.n)
    (m_g, n_g), (m_s, n_s) = _random_partition_means(g, draws), _random_partition_means(s, draws)
    assert np.array_equal(n_s, np.bincount(draws, minlength=K))
    assert np.array_equal(m_g, m_s) and np.array_equal(n_g, n_s)      # the shards continue each other's chains in row order


def _kpp_draw(data, centroid, first, u):
    from ml_amd import _lib
    index, certain = C.c_uint64(), C.c_int()
    _lib.check(_lib.lib.mlhip_kpp_draw(data.ctx.handle, data.handle, _lib.dptr(centroid), int(first), C.c_double(u), C.c_uint64(0),
                                       C.byref(index), C.byref(certain), None))
    weights = np.empty(data.n)
    _lib.check(_lib.lib.mlhip_kpp_weights(data.ctx.handle, data.handle, _lib.dptr(weights)))
    return index.value, certain.value, weights


def test_kpp_draw_and_weights(pair):
    g, s, X, _ = pair
    for first, row, u in ((1, 0, 0.37), (0, g.n - 1, 0.81)):
        centroid = X[row].copy()
        (i_g, c_g, w_g), (i_s, c_s, w_s) = _kpp_draw(g, centroid, first, u), _kpp_draw(s, centroid, first, u)
        assert (i_g, c_g) == (i_s, c_s)
        assert np.array_equal(w_g, w_s)


def test_min_squared_distances_are_bit_identical(pair):
    g, s, X, _ = pair
    C0 = X[:2].copy()
    assert np.array_equal(g.min_squared_distances(C0), s.min_squared_distances(C0))


def test_timing_get_after_a_timed_em_step(pair):
    g, s, X, (pi, mu, S) = pair
    g.ctx.timing_reset()
    g.ctx.timing_enable(True)
    g.em_step(pi, mu, S)
    g.ctx.timing_enable(False)
    assert g.ctx.timing_get("allreduce")[1] > 0                      # the shards' statistics met
    assert g.ctx.timing_get("em_estep")[1] + g.ctx.timing_get("em_fused")[1] > 0
    assert g.ctx.timing_get("no such kernel") == (0.0, 0)


def _em_step_in_place(data, pi, mu, S):
    from ml_amd import _lib
    pi, mu, S, ll = pi.copy(), mu.copy(), S.copy(), C.c_double()
    _lib.check(_lib.lib.mlhip_em_step(data.ctx.handle, data.handle, K, _lib.dptr(pi), _lib.dptr(mu), _lib.dptr(S), C.byref(ll),
                                      _lib.dptr(pi), _lib.dptr(mu), _lib.dptr(S)))
    return ll.value, pi, mu, S


def test_em_step_with_outputs_aliasing_inputs(pair):
    g, s, X, (pi, mu, S) = pair
    apart, in_place, ref = g.em_step(pi, mu, S), _em_step_in_place(g, pi, mu, S), _em_step_in_place(s, pi, mu, S)
    for a, b in zip(apart, in_place):
        assert np.array_equal(a, b)                                   # shard 0 wrote the caller's arrays; nobody read them after
    assert abs(in_place[0] - ref[0]) <= 1e-12 * abs(ref[0])
    assert relerr(in_place[1], ref[1]) < 1e-11 and relerr(in_place[2], ref[2]) < 1e-11 and relerr(in_place[3], ref[3]) < 1e-10


def test_responsibilities_of_a_row_range_across_two_shards(pair):
    g, s, X, (pi, mu, S) = pair
    g.em_step(pi, mu, S); s.em_step(pi, mu, S)
    first_of_shard_1 = g.shard_rows(1)[0]
    lo, cnt = first_of_shard_1 - 1, 2                                 # the last row of shard 0 and the first of shard 1
    R_g = g.em_responsibilities(K)
    assert np.array_equal(g.em_responsibilities_rows(K, lo, cnt), R_g[lo:lo + cnt])
    assert np.max(np.abs(g.em_responsibilities_rows(K, lo, cnt) - s.em_responsibilities_rows(K, lo, cnt))) < 1e-12


def _invalid_calls():
    """name -> call(data, other, pi, mu, S) -> status; `other` is the block of the OTHER kind of context."""
    from ml_amd import _lib
    lib, dptr = _lib.lib, _lib.dptr

    def em_step(data, other, pi, mu, S, K=K, handle=None, out=True):
        ll, o = C.c_double(), (np.empty_like(pi), np.empty_like(mu), np.empty_like(S))
        return lib.mlhip_em_step(data.ctx.handle, handle or data.handle, K, dptr(pi), dptr(mu), dptr(S), C.byref(ll),
                                 dptr(o[0]) if out else None, dptr(o[1]), dptr(o[2]))

    def maximisation_from(data, other, pi, mu, S):
        R = np.asfortranarray(np.full((data.n, K), 1.0 / K))
        o = (np.empty_like(pi), np.empty_like(mu), np.empty_like(S))
        return lib.mlhip_em_maximisation_from(data.ctx.handle, data.handle, K, dptr(R), C.c_int64(data.n - 1), dptr(o[0]), dptr(o[1]), dptr(o[2]))

    def responsibilities_rows(data, other, pi, mu, S):
        out = np.empty((2, K), order="F")
        return lib.mlhip_em_responsibilities_rows(data.ctx.handle, data.handle, K, C.c_uint64(data.n - 1), C.c_uint64(2), dptr(out), C.c_int64(2))

    def em_iterate(data, other, pi, mu, S, max_steps=3, atol=0.0):
        pi, mu, S = pi.copy(), mu.copy(), S.copy()
        steps, conv, ll = C.c_uint32(), C.c_int(), C.c_double()
        return lib.mlhip_em_iterate(data.ctx.handle, data.handle, K, 0, dptr(pi), dptr(mu), dptr(S), C.c_uint32(max_steps), C.c_double(atol),
                                    C.c_double(0.0), C.byref(steps), C.byref(conv), C.byref(ll), None)

    return {
        "null output": lambda *a: em_step(*a, out=False),
        "K = 0": lambda *a: em_step(*a, K=0),
        "handle of the other context": lambda data, other, *p: em_step(data, other, *p, handle=other.handle),
        "ldr too small": maximisation_from,
        "row range past the end": responsibilities_rows,
        "max_steps = 0": lambda *a: em_iterate(*a, max_steps=0),
        "negative tolerance": lambda *a: em_iterate(*a, atol=-1.0),
    }


def _raised(status):
    from ml_amd import _lib
    with pytest.raises(Exception) as e:
        _lib.check(status)
    return e.type


@pytest.mark.parametrize("what", ["null output", "K = 0", "handle of the other context", "ldr too small", "row range past the end",
                                  "max_steps = 0", "negative tolerance"])
def test_an_invalid_call_fails_alike_and_the_group_goes_on(pair, what):
    g, s, X, (pi, mu, S) = pair
    call = _invalid_calls()[what]
    status_g = call(g, s, pi, mu, S)
    raised_g = _raised(status_g)
    status_s = call(s, g, pi, mu, S)
    assert status_g == status_s and raised_g is _raised(status_s) and raised_g is ValueError
    a, b = g.em_step(pi, mu, S), s.em_step(pi, mu, S)
    assert abs(a[0] - b[0]) <= 1e-12 * abs(b[0]) and relerr(a[2], b[2]) < 1e-11
