"""Times mlhip_em_conditional_means (E[x_M | x_O] of a resident block) in one process on one GPU, piece by piece, beside the float64
numpy restatement of the same definition (tests/condition_reference.py) on CPU threads.

    python tools/condition_timing.py [--shapes 10000000x32x16x64xfull,1000000x16x8x16xfull,10000000x4x2x3xfull,10000000x32x16x64xdiag]
                                     [--reps 3] [--threads 16] [--numpy-rows 200000] [--out profiles/condition_timing.txt]

A shape is N x d x observed x K x mode; the first `observed` coordinates are the observed ones. mode `diag`: the model's variances go in
as diagonal input, so every map is +0.0 (the kernel does the same work: it does not look at the maps). Per shape, after one warm-up, the
medians of `reps` repetitions of
  estep    the HIP-event time of the marginal mixture's E-step kernels over all chunks of the call (their sum),
  cond     the same for the conditioning kernel, with the skip and (cond/all) without it (MLHIP_CONDITION_SKIP=0);
  active   the share of the N K responsibilities that are not exactly 0 (from a sample of rows): K_active / K per row;
  TF/s     2 K_active dM dO flop per row over `cond`, next to the fp64 vector peak of 78.6;
  GB/s     the kernel's HBM bytes -- 8 (dO + K + 1) read and 8 dM written per row -- over `cond`;
  call     wall time of the whole call: records, chunks, and the download of N x dM doubles into pageable memory;
  rest     call - estep - cond: mostly the download;
  numpy    the float64 restatement on `threads` threads over --numpy-rows rows, scaled to N rows (its rate does not depend on N).
Wrap the same command in `rocprofv3 --kernel-trace --stats --` for the profiler's view of the same kernels."""
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


def numpy_ms(ref, pi, mu, S, observed, X_o, threads):
    parts = np.array_split(np.arange(len(X_o)), threads)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(lambda rows: ref.conditional_mean(pi, mu, S, observed, X_o[rows])["y"], parts))
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10000000x32x16x64xfull,1000000x16x8x16xfull,10000000x4x2x3xfull,10000000x32x16x64xdiag")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--numpy-rows", type=int, default=200000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import condition_reference as ref
    from ml_amd import _lib, synth
    ctx = _lib.Context(0)
    lines = ["# medians of %d repetitions after one warm-up; kernels by HIP events (summed over the call's chunks), the rest wall clock (ms);"
             % args.reps,
             "# numpy: the float64 restatement on %d threads over %d rows, scaled to N" % (args.threads, args.numpy_rows),
             "%9s %3s %3s %3s %3s %-5s %-9s %7s %8s %8s %9s %7s %6s %7s %8s %8s %10s"
             % ("N", "d", "dO", "dM", "K", "mode", "kernel", "chunks", "estep", "cond", "cond/all", "active", "TF/s", "GB/s", "call", "rest", "numpy")]
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
            S_np = np.stack([np.diag(v) for v in variances])
        else:
            cond = _lib.em_condition(mu, S, observed)
            S_np = S
        data = _lib.Data(ctx, X_o)
        kernel = data.em_condition_route(K, dM)
        sample = _lib.Data(ctx, np.ascontiguousarray(X_o[:: max(1, n // 100000)]))
        sample.em_expectation(pi, cond[0], cond[1])
        active = float(np.count_nonzero(sample.em_responsibilities(K))) / (sample.n * K)
        sample.close()
        times = {"estep": [], "cond": [], "all": [], "call": []}
        chunks = 0
        ctx.timing_enable(True)
        for rep in range(args.reps + 1):
            for skip in ("1", "0"):
                os.environ["MLHIP_CONDITION_SKIP"] = skip
                ctx.timing_reset()
                t0 = time.perf_counter()
                y = data.em_conditional_means(pi, *cond)
                t1 = time.perf_counter()
                del y
                e_ms, e_n = ctx.timing_get("em_estep")
                c_ms, c_n = ctx.timing_get("em_condition")
                chunks = c_n
                if rep and skip == "1":
                    times["estep"].append(e_ms * e_n)
                    times["cond"].append(c_ms * c_n)
                    times["call"].append(1e3 * (t1 - t0))
                elif rep:
                    times["all"].append(c_ms * c_n)
        os.environ.pop("MLHIP_CONDITION_SKIP", None)
        ctx.timing_enable(False)
        data.close()
        e, c, a, call = (statistics.median(times[k]) for k in ("estep", "cond", "all", "call"))
        rows = min(n, args.numpy_rows)
        t_np = numpy_ms(ref, pi, mu, S_np, observed, X_o[:rows], args.threads) * n / rows
        tflops = 2.0 * active * K * dM * dO * n / (c * 1e-3) / 1e12
        gbs = 8.0 * (dO + K + 1 + dM) * n / (c * 1e-3) / 1e9
        lines.append("%9d %3d %3d %3d %3d %-5s %-9s %7d %8.3f %8.3f %9.3f %7.3f %6.2f %7.0f %8.1f %8.1f %10.0f"
                     % (n, d, dO, dM, K, mode, kernel, chunks, e, c, a, active, tflops, gbs, call, call - e - c, t_np))
        print(lines[-1], flush=True)
        del X_o
    ctx.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
