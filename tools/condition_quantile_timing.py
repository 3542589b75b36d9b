"""Times mlhip_em_conditional_cdfs and mlhip_em_conditional_quantiles (the per-coordinate predictive CDF and its inverse for a resident
block) in one process on one GPU, piece by piece, beside mlhip_em_conditional_means and one draw of mlhip_em_conditional_samples on
the same block, measured in the same run.

    python tools/condition_quantile_timing.py [--shapes 10000000x32x16x64,10000000x4x2x3] [--reps 5] [--threads 16] [--out FILE]

A shape is N x d x observed x K. Per shape, after one warm-up, the median (and the smallest and largest) of `reps` repetitions of
  estep     the HIP-event time of the marginal mixture's E-step kernels over all chunks of the CDF call (their sum),
  cdf       the same for the CDF kernel (one launch per chunk), at values drawn from the model itself;
  q1        the quantile kernel at P = 1 (p = 0.5), summed over the call's launches;
  q3        the quantile kernel at P = 3 (p = 0.05, 0.5, 0.95);
  mean      the conditioning kernel of mlhip_em_conditional_means on the same block (its own call);
  draw      the drawing kernel of ONE draw of mlhip_em_conditional_samples on the same block: what one term of a Monte-Carlo
            quantile costs, whose error after q draws falls as 1 / sqrt(q);
  trips     the mean trips per output of the q3 call and, behind the slash, the mean over waves of the LARGEST trip count among a
            wave's 64 rows x dM coordinates -- what the lock-step search runs -- from the first rows of the block;
  run       the share of the K components a wave of 64 rows runs (components with a nonzero responsibility in some row of the wave / K);
  TF/s      the flop of the CDF kernel -- per row and component run: the chain (2 dM dO) and per coordinate the subtraction, the
            product, normal_cdf (1 division counted as 1, 26 + 14 + 2 fused multiply-adds counted as 2, 12 other operations) and the
            accumulation: 2 dM dO + 100 dM -- over `cdf`, next to the fp64 vector peak of 78.6;
  GB/s      the CDF kernel's HBM bytes -- 8 (K + 1) + 8 dO + 16 dM per row -- over `cdf`;
  call      wall time of the whole CDF call: records, chunks, the upload of the values and the download into pageable memory.
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
RUN_ROWS = 64 * 4096            # rows the share of components run and the trip counts are taken from
P1 = (0.5,)
P3 = (0.05, 0.5, 0.95)


def spread(values):
    return "%.3f (%.3f-%.3f)" % (statistics.median(values), min(values), max(values))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10000000x32x16x64,10000000x4x2x3")
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
    emit("%9s %3s %3s %3s %3s %-19s %6s %-21s %-24s %-24s %-27s %-21s %-24s %-11s %6s %6s %7s %9s"
         % ("N", "d", "dO", "dM", "K", "kernels", "chunks", "estep", "cdf", "q1", "q3", "mean", "draw", "trips", "run", "TF/s", "GB/s", "call"))
    for shape in args.shapes.split(","):
        n, d, dO, K = (int(x) for x in shape.split("x"))
        dM = d - dO
        observed = list(range(dO))
        mix = synth.Mixture(d, K, seed=11)
        pi, mu, S = mix.weights, mix.means, mix.covs
        X, _ = mix.sample(n, threads=args.threads)
        X_o = np.ascontiguousarray(X[:, :dO])
        values = np.ascontiguousarray(X[:, dO:])
        del X
        cond = _lib.em_condition(mu, S, observed)
        C_m, G = _lib.em_condition_covariances(S, observed)
        scales = _lib.em_condition_scales(C_m)
        head = _lib.Data(ctx, X_o[:RUN_ROWS])
        head.em_expectation(pi, cond[0], cond[1])
        R = head.em_responsibilities(K)
        waves = R[: len(R) // 64 * 64].reshape(-1, 64, K)
        run = float((waves != 0).any(axis=1).sum(axis=1).mean()) / K
        del R, waves
        _, trips = _lib.em_conditional_quantiles(head, pi, *cond, *scales, P3, iterations=True)
        head.close()
        per_wave = trips[:, : trips.shape[1] // 64 * 64].reshape(len(P3), -1, 64 * dM).max(axis=2)
        trip_text = "%.2f/%.2f" % (trips.mean(), per_wave.mean())
        del trips
        data = _lib.Data(ctx, X_o)
        kernels = _lib.em_condition_quantile_route(data, K, dM, False) + "/" + _lib.em_condition_quantile_route(data, K, dM, True)
        ctx.timing_enable(True)
        times = {"estep": [], "cdf": [], "q1": [], "q3": [], "mean": [], "draw": [], "call": []}
        chunks = 1
        for rep in range(args.reps + 1):
            ctx.timing_reset()
            t0 = time.perf_counter()
            out = _lib.em_conditional_cdfs(data, pi, *cond, *scales, values)
            t1 = time.perf_counter()
            del out
            e_ms, e_n = ctx.timing_get("em_estep")
            f_ms, f_n = ctx.timing_get("em_condition_cdf")
            chunks = max(1, f_n)
            measured = {}
            for name, probabilities in (("q1", P1), ("q3", P3)):
                ctx.timing_reset()
                out = _lib.em_conditional_quantiles(data, pi, *cond, *scales, probabilities)
                del out
                q_ms, q_n = ctx.timing_get("em_condition_quantile")
                measured[name] = q_ms * q_n
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
                times["cdf"].append(f_ms * f_n)
                times["q1"].append(measured["q1"])
                times["q3"].append(measured["q3"])
                times["mean"].append(c_ms * c_n)
                times["draw"].append(s_ms * s_n)
                times["call"].append(1e3 * (t1 - t0))
        f = statistics.median(times["cdf"])
        flop = run * K * dM * (2.0 * dO + 100.0)
        tflops = flop * n / (f * 1e-3) / 1e12
        gbs = 8.0 * ((K + 1) + dO + 2.0 * dM) * n / (f * 1e-3) / 1e9
        emit("%9d %3d %3d %3d %3d %-19s %6d %-21s %-24s %-24s %-27s %-21s %-24s %-11s %6.3f %6.2f %7.0f %9.1f"
             % (n, d, dO, dM, K, kernels, chunks, spread(times["estep"]), spread(times["cdf"]), spread(times["q1"]), spread(times["q3"]),
                spread(times["mean"]), spread(times["draw"]), trip_text, run, tflops, gbs, statistics.median(times["call"])))
        ctx.timing_enable(False)
        data.close()
        del X_o, values
    ctx.close()


if __name__ == "__main__":
    main()
