"""Device time of one tied-covariance EM iteration on the tied kernel (device/em_tied.hip) against the same iteration on the
full-covariance path with the covariance replicated K times (mlhip_em_step: what a user had before the tied mode), in ONE process:
per step the kernels' HIP-event times (mlhip_timing_*) are summed, and the MEDIAN over the repeated steps after a warm-up is kept.

The tool pins the kernel route for (a): it sets MLHIP_TIED=kernel in its own environment before the first library call (the routing
reads the switch at every call), so that shapes the default routing sends to the composed path are timed on the kernel too -- that
comparison is what decides the default. The full path is timed twice: (b) repeated steps from one fixed start, and (b') along a
fit, every step starting from the previous step's result, where the self-normalising statistics pass may switch to its sparse
kernel once the responsibilities have sharpened (what `python bench.py` measures). A shape keeps the kernel route only while (a) is
below BOTH. Writes profiles/tied_timing.txt, the routing consequence included.

    python tools/tied_timing.py [--repeats 15] [--warmup 3] [--out profiles/tied_timing.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(10_000_000, 32, 64), (1_000_000, 16, 16), (10_000_000, 4, 3)]
FULL_KERNELS = ("em_estep", "em_mstats", "em_fused", "em_refine", "em_weights")


def sample(n, d, K, seed):
    rng = np.random.default_rng(seed)
    means = 2.5 * rng.standard_normal((K, d))
    A = rng.standard_normal((d, d))
    Sigma = A @ A.T / d + 0.5 * np.eye(d)
    L = np.linalg.cholesky(Sigma)
    X = np.empty((n, d))
    for lo in range(0, n, 1_000_000):                     # in slabs: no second N x d temporary
        hi = min(n, lo + 1_000_000)
        X[lo:hi] = means[rng.integers(0, K, hi - lo)] + rng.standard_normal((hi - lo, d)) @ L.T
    return X, np.full(K, 1.0 / K), means + 0.2 * rng.standard_normal((K, d)), Sigma + 0.1 * np.eye(d)


def timed_steps(ctx, step, kernels, warmup, repeats):
    """Median over `repeats` calls of step() of (sum of the named kernels' device ms, wall ms of the whole call)."""
    for _ in range(warmup):
        step()
    dev, wall = [], []
    for _ in range(repeats):
        ctx.timing_reset()
        t0 = time.perf_counter()
        step()
        wall.append(1e3 * (time.perf_counter() - t0))
        total = 0.0
        for name in kernels:
            ms, launches = ctx.timing_get(name)
            total += ms * launches
        dev.append(total)
    return statistics.median(dev), statistics.median(wall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tied_timing.txt"))
    args = ap.parse_args()
    os.environ["MLHIP_TIED"] = "kernel"                    # (a) is the kernel at every shape: see the docstring
    from ml_amd import _lib
    ctx = _lib.Context()
    lines = ["# tools/tied_timing.py: one tied EM iteration, median of %d steps after %d warm-up steps, one process, MLHIP_TIED=kernel" % (args.repeats, args.warmup),
             "# (a)  tied kernel: em_tied",
             "# (b)  mlhip_em_step with the covariance replicated K times, every step from the same start: " + " + ".join(FULL_KERNELS),
             "# (b') the same along a fit (every step from the previous step's result; the statistics pass may turn sparse)",
             "# device ms = HIP-event time of the kernels of one step; wall ms = the whole call (records, closing, read-back)",
             "# %10s %4s %4s %10s %10s %10s %8s %9s %9s %9s %9s  %s" % ("N", "d", "K", "(a) dev", "(b) dev", "(b') dev", "min/(a)", "(a) wall", "(b) wall",
                                                                  "(b') wall", "full route", "default route")]
    composed = []
    for n, d, K in SHAPES:
        X, pi0, mu0, S0 = sample(n, d, K, 1000 + d)
        dt = _lib.Data(ctx, X)
        del X
        assert dt.em_tied_route(K) == "kernel"
        route = dt.em_route(K)
        full_route = "fused/" + route["fused_form"] if route["fused"] else route["estep"] + ("+self_norm" if route["self_norm"] else "")
        full = np.ascontiguousarray(np.stack([S0] * K))
        ctx.timing_enable(True)
        a_dev, a_wall = timed_steps(ctx, lambda: dt.em_step_tied(pi0, mu0, S0), ("em_tied",), args.warmup, args.repeats)
        b_dev, b_wall = timed_steps(ctx, lambda: dt.em_step(pi0, mu0, full), FULL_KERNELS, args.warmup, args.repeats)
        state = [pi0, mu0, full]

        def fit_step():
            _, state[0], state[1], state[2] = dt.em_step(state[0], state[1], state[2])

        c_dev, c_wall = timed_steps(ctx, fit_step, FULL_KERNELS, args.warmup, args.repeats)
        ctx.timing_enable(False)
        dt.close()
        keeps = a_dev < min(b_dev, c_dev)
        if not keeps:
            composed.append((n, d, K, full_route))
        lines.append("  %10d %4d %4d %10.4f %10.4f %10.4f %8.2f %9.3f %9.3f %9.3f %9s  %s" %
                     (n, d, K, a_dev, b_dev, c_dev, min(b_dev, c_dev) / a_dev, a_wall, b_wall, c_wall, full_route,
                      "kernel" if keeps else "composed: (a) < (b) fails"))
        print(lines[-1], flush=True)
    ctx.close()
    lines.append("# Routing that follows (runtime/route.cpp mode_route): a shape where (a) < (b) fails takes the composed route by default;")
    lines.append("# MLHIP_TIED=kernel still selects the kernel there.")
    for n, d, K, full_route in composed:
        lines.append("#   N=%d d=%d K=%d: composed (its full-covariance step is %s)" % (n, d, K, full_route))
    if not composed:
        lines.append("#   none of the shapes above")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
