"""Times mlhip_em_conditional_samples (draws from p(x_M | x_O) for a resident block) in one process on one GPU, piece by piece, beside
mlhip_em_conditional_means on the same block and the float64 numpy restatement of the same definition
(tests/condition_sample_reference.py) on CPU threads.

    python tools/condition_sample_timing.py [--shapes 10000000x32x16x64xfull,1000000x16x8x16xfull,10000000x4x2x3xfull,10000000x32x16x64xdiag]
                                            [--draws 1,8] [--reps 3] [--threads 16] [--numpy-rows 50000] [--out FILE]

A shape is N x d x observed x K x mode as in tools/condition_timing.py. Per shape and number of draws, after one warm-up, the medians
of `reps` repetitions of
  estep    the HIP-event time of the marginal mixture's E-step kernels over all chunks of the call (their sum),
  draw     the same for the drawing kernel (all launches of the call), and draw/1 = draw / n_draws;
  mean     the conditioning kernel of mlhip_em_conditional_means on the same block (its own call);
  run      the share of the K components a wave of 64 rows runs: distinct labels per wave / K, from draw 0's labels;
  TF/s     2 (run K) dM (dO + (dM + 1) / 2) flop per row and draw over `draw`, next to the fp64 vector peak of 78.6 -- the work
           the waves do, not the 2 dM (dO + (dM + 1) / 2) a row needs;
  GB/s     the kernel's HBM bytes -- 8 (K + 1) per row read twice by every launch behind a chunk, 8 dO read and 8 dM written per row
           and draw -- over `draw`;
  call     wall time of the whole call: records, chunks, and the download of n_draws x N x dM doubles into pageable memory;
  numpy    the float64 restatement on `threads` threads over --numpy-rows rows, scaled to N rows.
Every line is appended to --out as soon as it is measured."""
import argparse
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_TFLOPS = 78.6              # fp64 vector peak, DESIGN.md section 2


def numpy_ms(ref, pi, mu, S, observed, X_o, draws, threads):
    parts = np.array_split(np.arange(len(X_o)), threads)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(lambda rows: ref.sample(pi, mu, S, observed, X_o[rows], n_draws=draws, first_row=int(rows[0]))[0], parts))
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10000000x32x16x64xfull,1000000x16x8x16xfull,10000000x4x2x3xfull,10000000x32x16x64xdiag")
    ap.add_argument("--draws", default="1,8")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--numpy-rows", type=int, default=50000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import condition_sample_reference as ref
    from ml_amd import _lib, synth

    def emit(line):
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    ctx = _lib.Context(0)
    emit("# medians of %d repetitions after one warm-up; kernels by HIP events (summed over the call's launches), the rest wall clock (ms);" % args.reps)
    emit("# numpy: the float64 restatement on %d threads over %d rows, scaled to N" % (args.threads, args.numpy_rows))
    emit("%9s %3s %3s %3s %3s %-5s %-9s %5s %8s %8s %8s %8s %8s %6s %6s %7s %9s %10s"
         % ("N", "d", "dO", "dM", "K", "mode", "kernel", "draws", "launches", "estep", "draw", "draw/1", "mean", "run", "TF/s", "GB/s", "call", "numpy"))
    for shape in args.shapes.split(","):
        n, d, dO, K, mode = shape.split("x")
        n, d, dO, K = int(n), int(d), int(dO), int(K)
        dM = d - dO
        observed = list(range(dO))
        mix = synth.Mixture(d, K, seed=11)
        pi, mu, S = mix.weights, mix.means, mix.covs
        X, _ = mix.sample(n, threads=args.threads)
        X_o = np.ascontiguousarray(X[:, :dO])
        del X
        if mode == "diag":
            variances = np.ascontiguousarray(np.stack([np.diag(S[k]) for k in range(K)]))
            cond = _lib.em_condition(mu, variances, observed, diagonal=True)
            _, G = _lib.em_condition_covariances(variances, observed, diagonal=True)
            S_np = np.stack([np.diag(v) for v in variances])
        else:
            cond = _lib.em_condition(mu, S, observed)
            _, G = _lib.em_condition_covariances(S, observed)
            S_np = S
        data = _lib.Data(ctx, X_o)
        kernel = data.em_conditional_sample_route(K, dM)
        ctx.timing_enable(True)
        mean_ms = []
        for rep in range(args.reps + 1):
            ctx.timing_reset()
            y = data.em_conditional_means(pi, *cond)
            del y
            c_ms, c_n = ctx.timing_get("em_condition")
            if rep:
                mean_ms.append(c_ms * c_n)
        for draws in (int(q) for q in args.draws.split(",")):
            times = {"estep": [], "draw": [], "call": []}
            launches, chunks, run = 0, 1, 0.0
            for rep in range(args.reps + 1):
                ctx.timing_reset()
                t0 = time.perf_counter()
                out = data.em_conditional_samples(pi, *cond, G, n_draws=draws, seed=1, labels=not rep)
                t1 = time.perf_counter()
                if not rep:
                    labels = out[1][0]
                    tiles = labels[: len(labels) // 64 * 64].reshape(-1, 64)[:: max(1, len(labels) // 64 // 20000)]
                    ordered = np.sort(tiles, axis=1)
                    run = float((1 + (np.diff(ordered, axis=1) != 0).sum(axis=1)).mean()) / K
                del out
                e_ms, e_n = ctx.timing_get("em_estep")
                s_ms, s_n = ctx.timing_get("em_condition_sample")
                launches, chunks = s_n, max(1, e_n)
                if rep:
                    times["estep"].append(e_ms * e_n)
                    times["draw"].append(s_ms * s_n)
                    times["call"].append(1e3 * (t1 - t0))
            e, s, call = (statistics.median(times[k]) for k in ("estep", "draw", "call"))
            rows = min(n, args.numpy_rows)
            t_np = numpy_ms(ref, pi, mu, S_np, observed, X_o[:rows], draws, args.threads) * n / rows
            tflops = 2.0 * run * K * dM * (dO + (dM + 1) / 2.0) * n * draws / (s * 1e-3) / 1e12
            gbs = 8.0 * (2.0 * (K + 1) * launches / chunks + (dO + dM) * draws) * n / (s * 1e-3) / 1e9
            emit("%9d %3d %3d %3d %3d %-5s %-9s %5d %8d %8.3f %8.3f %8.3f %8.3f %6.3f %6.2f %7.0f %9.1f %10.0f"
                 % (n, d, dO, dM, K, mode, kernel, draws, launches, e, s, s / draws, statistics.median(mean_ms), run, tflops, gbs, call, t_np))
        ctx.timing_enable(False)
        data.close()
        del X_o
    ctx.close()


if __name__ == "__main__":
    main()
