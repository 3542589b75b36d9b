"""Times mlhip_em_conditional_variances (Var[x_M | x_O] for a resident block) in one process on one GPU, piece by piece, beside
mlhip_em_conditional_means and one draw of mlhip_em_conditional_samples on the same block, measured in the same run.

    python tools/condition_variance_timing.py [--shapes 10000000x32x16x64xdiag,1000000x32x16x64xfull,10000000x4x2x3xdiag,10000000x4x2x3xfull]
                                              [--reps 5] [--threads 16] [--out FILE]

A shape is N x d x observed x K x form, form = diag (N x dM variances) or full (N x dM x dM covariances; at d = 32 its output is 2 KiB
per row, so the default shape takes N = 1M there). Per shape, after one warm-up, the median (and the smallest and largest) of `reps`
repetitions of
  estep     the HIP-event time of the marginal mixture's E-step kernels over all chunks of the call (their sum),
  variance  the same for the variance kernel (one launch per chunk);
  mean      the conditioning kernel of mlhip_em_conditional_means on the same block (its own call);
  draw      the drawing kernel of ONE draw of mlhip_em_conditional_samples on the same block: what one term of a Monte-Carlo
            variance costs, whose error after q draws is 1 / sqrt(q) of the variance's own spread;
  run       the share of the K components a wave of 64 rows runs: components with a nonzero responsibility in some row of the
            wave / K, from the E-step's responsibilities on the first rows of the block;
  TF/s      the flop the waves do -- per row and component run: the chain twice (2 x 2 dM dO), y (2 dM), u (dM) and the accumulators
            (4 dM, or 2 dM (dM + 1) in the full form) -- over `variance`, next to the fp64 vector peak of 78.6;
  GB/s      the kernel's HBM bytes -- 8 (K + 1) per row read by each of the two passes, 8 dO read and 8 dM or 8 dM^2 written per row
            -- over `variance`;
  call      wall time of the whole call: records, chunks, and the download into pageable memory.
Every line is appended to --out as soon as it is measured."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TFLOPS = 78.6              # fp64 vector peak, DESIGN.md section 2
RUN_ROWS = 64 * 4096            # rows the share of components run is taken from


def spread(values):
    return "%.3f (%.3f-%.3f)" % (statistics.median(values), min(values), max(values))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10000000x32x16x64xdiag,1000000x32x16x64xfull,10000000x4x2x3xdiag,10000000x4x2x3xfull")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ml_amd import _lib, synth

    def emit(line):
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    ctx = _lib.Context(0)
    emit("# median (smallest-largest) of %d repetitions after one warm-up; kernels by HIP events (summed over the call's launches), call: wall clock (ms)"
         % args.reps)
    emit("%9s %3s %3s %3s %3s %-5s %-9s %6s %-21s %-24s %-21s %-24s %6s %6s %7s %9s"
         % ("N", "d", "dO", "dM", "K", "form", "kernel", "chunks", "estep", "variance", "mean", "draw", "run", "TF/s", "GB/s", "call"))
    for shape in args.shapes.split(","):
        n, d, dO, K, form = shape.split("x")
        n, d, dO, K = int(n), int(d), int(dO), int(K)
        full = form == "full"
        dM = d - dO
        observed = list(range(dO))
        mix = synth.Mixture(d, K, seed=11)
        pi, mu, S = mix.weights, mix.means, mix.covs
        X, _ = mix.sample(n, threads=args.threads)
        X_o = np.ascontiguousarray(X[:, :dO])
        del X
        cond = _lib.em_condition(mu, S, observed)
        C_m, G = _lib.em_condition_covariances(S, observed)
        head = _lib.Data(ctx, X_o[:RUN_ROWS])
        head.em_expectation(pi, cond[0], cond[1])
        R = head.em_responsibilities(K)
        head.close()
        waves = R[: len(R) // 64 * 64].reshape(-1, 64, K)
        run = float((waves != 0).any(axis=1).sum(axis=1).mean()) / K
        del R, waves
        data = _lib.Data(ctx, X_o)
        kernel = _lib.em_condition_variance_route(data, K, dM, full)
        ctx.timing_enable(True)
        times = {"estep": [], "variance": [], "mean": [], "draw": [], "call": []}
        chunks = 1
        for rep in range(args.reps + 1):
            ctx.timing_reset()
            t0 = time.perf_counter()
            out = _lib.em_conditional_variances(data, pi, *cond, C_m, full=full)
            t1 = time.perf_counter()
            del out
            e_ms, e_n = ctx.timing_get("em_estep")
            v_ms, v_n = ctx.timing_get("em_condition_variance")
            chunks = max(1, v_n)
            ctx.timing_reset()
            y = data.em_conditional_means(pi, *cond)
            del y
            c_ms, c_n = ctx.timing_get("em_condition")
            ctx.timing_reset()
            x = data.em_conditional_samples(pi, *cond, G, n_draws=1, seed=1)
            del x
            s_ms, s_n = ctx.timing_get("em_condition_sample")
            if rep:
                times["estep"].append(e_ms * e_n)
                times["variance"].append(v_ms * v_n)
                times["mean"].append(c_ms * c_n)
                times["draw"].append(s_ms * s_n)
                times["call"].append(1e3 * (t1 - t0))
        v = statistics.median(times["variance"])
        width = dM * dM if full else dM
        flop = run * K * (dM * (4.0 * dO + 3.0) + (2.0 * dM * (dM + 1) if full else 4.0 * dM))
        tflops = flop * n / (v * 1e-3) / 1e12
        gbs = 8.0 * (2.0 * (K + 1) + dO + width) * n / (v * 1e-3) / 1e9
        emit("%9d %3d %3d %3d %3d %-5s %-9s %6d %-21s %-24s %-21s %-24s %6.3f %6.2f %7.0f %9.1f"
             % (n, d, dO, dM, K, form, kernel, chunks, spread(times["estep"]), spread(times["variance"]), spread(times["mean"]),
                spread(times["draw"]), run, tflops, gbs, statistics.median(times["call"])))
        ctx.timing_enable(False)
        data.close()
        del X_o
    ctx.close()


if __name__ == "__main__":
    main()
