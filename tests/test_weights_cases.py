"""Cases shared by the row-weight tests (tests/test_gpu_weights.py runs them on the GPU): shapes from oracle.hp_cases.problem on
every kernel tier (d = 2 ... 130, ragged N), frequency weights from a seeded generator in {0, 1, 2, 3}, and the REPLICATED sample
-- row i repeated w_i times -- on which the unweighted extended-precision reference and the CPU oracle give what a weighted step
must give. The tests below run on the CPU and check that each case can be tested at all: enough rows of weight 0, every component
with positive mass in the reference's step, and the oracle's step on the replicated sample inside the bound
tests/test_hp_reference.py holds it to."""
import functools

import numpy as np
import pytest

from oracle import hp_reference as hp
from oracle.hp_cases import oracle_step, problem
from test_hp_reference import C_ORACLE, step_errors

# (d, K, N, offset) and the E-step tier the shape runs on
SHAPES = [((2, 3, 3001, 0.0), "scalar_fed"), ((6, 8, 3001, 2.0), "scalar_fed"), ((13, 5, 3001, 0.0), "matrix4"),
          ((16, 8, 4001, 2.0), "matrix4"), ((32, 16, 6001, 0.0), "matrix4"), ((33, 4, 3001, 0.0), "matrix4"),
          ((64, 4, 3001, 3.0), "matrix4"), ((130, 3, 2001, 0.0), "big_dim")]
DIAG_SHAPE = (16, 8, 4001, 0.5)


def weights(n, seed=2024):
    """Integer frequency weights in {0, 1, 2, 3} as float64 (dyadic when divided by 4: the scaling cases lose nothing)."""
    return np.random.default_rng(seed).integers(0, 4, n).astype(np.float64)


def replicate(X, w, *more):
    """Row i of X (and of every array in `more`) repeated w_i times."""
    counts = w.astype(np.int64)
    out = tuple(np.ascontiguousarray(np.repeat(a, counts, axis=0)) for a in (X,) + more)
    return out[0] if not more else out


@functools.lru_cache(maxsize=None)
def case(d, K, n, offset, diagonal=False):
    """(X, w, pi0, mu0, S0, the replicated sample)."""
    X, pi0, mu0, S0 = problem(d, K, n, offset, diagonal)
    w = weights(n)
    return X, w, pi0, mu0, S0, replicate(X, w)


@functools.lru_cache(maxsize=None)
def references(d, K, n, offset, diagonal=False):
    """The extended-precision step and the CPU oracle's step, both on the replicated sample."""
    from oracle import oracle_ctypes as orc
    X, w, pi0, mu0, S0, Xr = case(d, K, n, offset, diagonal)
    ref = (hp.em_step_diag if diagonal else hp.em_step)(Xr, pi0, mu0, S0)
    cpu = oracle_step(orc, Xr, pi0, mu0, S0, diagonal)
    return ref, cpu


ALL = [(s, False) for s, _ in SHAPES] + [(DIAG_SHAPE, True)]


@pytest.mark.parametrize("shape,diagonal", ALL, ids=[f"d={s[0]}{'-diag' if dg else ''}" for s, dg in ALL])
def test_case_can_be_tested(shape, diagonal):
    X, w, pi0, mu0, S0, Xr = case(*shape, diagonal)
    assert np.all(np.isin(w, (0.0, 1.0, 2.0, 3.0))) and len(w) == len(X)
    assert (w == 0).mean() >= 0.10                                   # rows a weighted pass must leave out
    assert len(Xr) == int(w.sum()) and len(X) % 64 != 0              # the block the kernels see has a ragged last tile
    ref, cpu = references(*shape, diagonal)
    assert np.all(np.asarray(ref[2], dtype=np.float64) > 0)          # every component keeps positive mass
    cond = hp.conditioning(Xr.mean(axis=0), mu0, **({"variances": S0} if diagonal else {"covs": S0}))
    for name, (err, unit) in step_errors(cpu, ref, cond["kappa"], len(Xr)).items():
        print(f"replicated d={shape[0]} K={shape[1]} N={len(Xr)} {name}: err {err:.2e} = {err / unit:.3f} units of {unit:.2e}")
        assert err <= C_ORACLE * unit, name


def test_scaling_weights_are_exact():
    w = weights(4001)
    assert np.array_equal((w / 4) * 4, w) and float((w / 4).sum()) * 4 == float(w.sum())
