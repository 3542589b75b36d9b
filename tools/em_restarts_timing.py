"""Wall time of R restarts of a short EM fit: ONE batched call (mlhip_em_iterate_restarts under MLHIP_EM_RESTARTS=batch: the restarts
share the three launches of an iteration, device/em_restarts.hip) against R calls of mlhip_em_iterate on the same handle from the
same starts -- the solo path under its default routing (the one-launch resident loop where it applies), which the restarts feature
does not touch. 50 iterations per restart, tolerances 0, so both sides run the same iterations; the results are compared bit for bit
before anything is timed.

Both sides are host-clock times around calls that end in a stream synchronisation (the arrays come back to the host), in ONE process:
after a warm-up of both, the two are timed alternately `--repeats` times; the table gives the median and the (min .. max) spread of
each and the ratio of the medians. The automatic route (runtime/route.cpp restarts_route) takes the batch from the smallest R at
which it is faster at EVERY shape here, and at every larger R measured. Writes profiles/em_restarts_timing.txt, the routing
consequence included.

    python tools/em_restarts_timing.py [--repeats 11] [--warmup 2] [--out profiles/em_restarts_timing.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1_000, 2, 3), (10_000, 2, 3), (65_536, 2, 3), (10_000, 4, 3)]
RESTARTS = [2, 4, 8, 16, 32]
ITERATIONS = 50


def problem(n, d, K, R, seed):
    rng = np.random.default_rng(seed)
    means = 3.0 * rng.standard_normal((K, d))
    X = np.ascontiguousarray(means[rng.integers(0, K, n)] + rng.standard_normal((n, d)))
    mu0 = np.stack([means + (0.2 + 0.1 * r) * rng.standard_normal((K, d)) for r in range(R)])
    return X, mu0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "em_restarts_timing.txt"))
    args = ap.parse_args()
    os.environ["MLHIP_EM_RESTARTS"] = "batch"              # the batched call is the batch at every R: that comparison decides the default
    from ml_amd import _lib
    ctx = _lib.Context()
    lines = ["# tools/em_restarts_timing.py: R restarts of %d EM iterations (tolerances 0), wall ms of the whole call(s), median (min .. max) of %d"
             % (ITERATIONS, args.repeats),
             "# alternated repeats after %d warm-up rounds, one process, MLHIP_EM_RESTARTS=batch" % args.warmup,
             "# batched:    one mlhip_em_iterate_restarts (em_restarts_pass + em_restarts_reduce + em_restarts_close per iteration)",
             "# sequential: R x mlhip_em_iterate on the same handle, default routing (solo loop: see the column)",
             "# %8s %3s %3s %3s %28s %28s %9s %9s  %s" % ("N", "d", "K", "R", "batched ms", "sequential ms", "seq/batch", "us/it/R", "solo loop")]
    faster = {R: True for R in RESTARTS}
    for n, d, K in SHAPES:
        X, mu_all = problem(n, d, K, max(RESTARTS), 7 * d + K)
        dt = _lib.Data(ctx, X)
        _, cov = dt.sample_covariance()
        assert dt.em_restarts_route(K, 2)[0] == "batched"
        ctx.timing_enable(True)                           # which loop the solo call is at this shape: read off its launch counters
        ctx.timing_reset()
        dt.em_iterate(np.full(K, 1.0 / K), mu_all[0], np.stack([cov] * K), 3, 0.0, 0.0)
        solo_loop = "resident" if ctx.timing_get("em_resident")[1] else "three launches"
        ctx.timing_enable(False)
        for R in RESTARTS:
            pi0, mu0, S0 = np.full((R, K), 1.0 / K), mu_all[:R], np.stack([np.stack([cov] * K)] * R)

            def batched():
                return dt.em_iterate_restarts(pi0, mu0, S0, ITERATIONS, 0.0, 0.0)[0]

            def sequential():
                return [dt.em_iterate(pi0[r], mu0[r], S0[r], ITERATIONS, 0.0, 0.0) for r in range(R)]

            for got, ref in zip(batched(), sequential()):   # the same numbers, before anything is timed
                assert got[0] == ref[0] == ITERATIONS and got[2] == ref[2] and np.array_equal(got[6], ref[6])
                assert all(np.array_equal(a, b) for a, b in zip(got[3:6], ref[3:6]))
            for _ in range(args.warmup):
                batched()
                sequential()
            tb, ts = [], []
            for _ in range(args.repeats):
                for f, acc in ((batched, tb), (sequential, ts)):
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    f()
                    acc.append(1e3 * (time.perf_counter() - t0))
            mb, ms = statistics.median(tb), statistics.median(ts)
            faster[R] = faster[R] and mb < ms
            lines.append("  %8d %3d %3d %3d %9.3f (%7.3f .. %7.3f) %9.3f (%7.3f .. %7.3f) %9.2f %9.2f  %s" %
                         (n, d, K, R, mb, min(tb), max(tb), ms, min(ts), max(ts), ms / mb, 1e3 * mb / (ITERATIONS * R), solo_loop))
            print(lines[-1], flush=True)
        dt.close()
    ctx.close()
    # the smallest R from which the batch wins at every shape, at that R and every larger one measured
    batch_from = None
    for R in reversed(RESTARTS):
        if not faster[R]:
            break
        batch_from = R
    lines.append("# Routing that follows (runtime/route.cpp restarts_route, MLHIP_RESTARTS_BATCH_FROM in include/mlhip.h):")
    if batch_from is None:
        lines.append("#   the batch is faster at no measured R for every shape: the automatic route stays sequential, MLHIP_EM_RESTARTS=batch selects the batch")
    else:
        lines.append("#   the batch is faster at every shape from R = %d on (R = %s measured): the automatic route takes it from there"
                     % (batch_from, ", ".join(str(r) for r in RESTARTS)))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
