#!/usr/bin/env python3
"""Where the sparse statistics kernel stops paying: mixtures of decreasing separation at d = 32, K = 64, N = 2.5M, so that the
nonzero responsibilities per sample go from ~2 up to 64. For each mixture one forced-sparse and one forced-dense statistics pass
(MLHIP_MSTATS_SPARSE=1 / 0), timed by the library's own `em_mstats` timer (Context.timing_get), and the nonzero count of the
pass from the responsibilities themselves. Prints nonzeros per sample against both times; the crossover is where the threshold
kSparseMaxPairs (runtime/pass_history.hpp) belongs, just below.
    usage: python tools/mstats_sparse_sweep.py [--n 2500000] [--repeats 3] > profiles/mstats_sparse3_sweep.txt"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2_500_000)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--components", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--spreads", type=float, nargs="*", default=[6.0, 3.0, 2.0, 1.5, 1.2, 1.0, 0.8, 0.6, 0.4, 0.2, 0.05])
    args = ap.parse_args()
    from ml_amd import _lib

    d, K, n = args.dim, args.components, args.n
    ctx = _lib.Context()
    ctx.timing_enable(True)
    print(f"# N={n} d={d} K={K}: em_mstats timer, best of {args.repeats} passes after one warm-up pass, milliseconds")
    print("spread\tnonzeros_per_sample\tsparse_ms\tdense_ms")
    for spread in args.spreads:
        rng = np.random.default_rng(int(spread * 1000) + 1)
        means = spread * rng.standard_normal((K, d))
        X = np.ascontiguousarray(means[rng.integers(0, K, n)] + rng.standard_normal((n, d)))
        pi0, S0 = np.full(K, 1.0 / K), np.stack([np.eye(d)] * K)
        times = {}
        for m in ("1", "0"):
            os.environ["MLHIP_MSTATS_SPARSE"] = m
            data = _lib.Data(ctx, X)
            route = data.em_route(K)
            if not (route["self_norm"] and route["sparse"] is (m == "1")):
                raise SystemExit(f"the self-normalising statistics route is not taken at d={d}, K={K}: {route}")
            data.em_step(pi0, means, S0)
            best = float("inf")
            for _ in range(args.repeats):
                ctx.timing_reset()
                data.em_step(pi0, means, S0)
                ms, cnt = ctx.timing_get("em_mstats")
                best = min(best, ms / max(cnt, 1))
            times[m] = best
            if m == "0":
                # the count the kernels take: responsibilities that do not underflow, in float64 from the same parameters
                sub = X[: min(n, 20_000)]
                lw = -0.5 * ((sub * sub).sum(1)[:, None] - 2.0 * sub @ means.T + (means * means).sum(1)[None, :])
                nzs = float(np.mean(np.sum(lw - lw.max(axis=1, keepdims=True) > -745.13, axis=1)))
            data.close()
        print(f"{spread:g}\t{nzs:.2f}\t{times['1']:.3f}\t{times['0']:.3f}", flush=True)
    os.environ.pop("MLHIP_MSTATS_SPARSE", None)
    ctx.close()


if __name__ == "__main__":
    main()
