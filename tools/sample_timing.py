"""Times the device sampler (mlhip_em_sample / mlhip_em_sample_data) against today's way to get a mixture sample in this repository,
synth.Mixture.sample on CPU threads, in one process on one GPU.

    python tools/sample_timing.py [--shapes 10000000x32x64,10000000x4x3,1000000x16x16,100000x128x32] [--reps 3] [--threads 16]
                                  [--out profiles/sample_timing.txt]

Per shape (N x d x K), after one warm-up, the medians of `reps` repetitions of
  kernel   HIP-event time of the sampling kernel writing the whole N x d block in ONE launch (the handle form, mlhip_em_sample_data),
           and the bytes it writes per second (8 d + 4 per row) next to the copy rate of the microarchitecture guide;
  normals  the same kernel's rate in Box-Muller pairs per second (ceil(d/2) per row): with the bytes column this shows which of the
           two binds -- the VALU work of the normals (the rate stays put while d changes) or the stores (the bytes do);
  handle   wall time of mlhip_em_sample_data (factorisation, kernel, transpose into the resident layout, the shift);
  host     wall time of mlhip_em_sample: kernel in chunks + download of X and the labels into pageable memory;
  synth    wall time of synth.Mixture.sample(n, threads=...) -- the comparator; it still has to be uploaded afterwards.
Wrap the same command in `rocprofv3 --kernel-trace --stats --` for the profiler's view of the same kernel."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_TBS = 6.29                 # MI355X copy rate (read + write counted), microarchitecture guide


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10000000x32x64,10000000x4x3,1000000x16x16,100000x128x32")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ml_amd import _lib, synth
    ctx = _lib.Context(0)
    lines = ["# medians of %d repetitions after one warm-up; kernel by HIP events, the rest wall clock (ms); synth on %d CPU threads"
             % (args.reps, args.threads),
             "%9s %4s %4s %-12s %9s %8s %8s %10s %9s %9s %9s %10s %10s" % ("N", "d", "K", "route", "kernel", "GB/s", "% copy", "Gpairs/s",
                                                                            "handle", "host", "synth", "synth/host", "synth/hnd")]
    for shape in args.shapes.split(","):
        n, d, K = (int(v) for v in shape.split("x"))
        mix = synth.Mixture(d, K, seed=11)
        pi, mu, S = mix.weights, mix.means, mix.covs
        route = _lib.em_sample_route(d, K)
        t_kernel, t_handle, t_host, t_synth = [], [], [], []
        ctx.timing_enable(True)
        for rep in range(args.reps + 1):
            ctx.timing_reset()
            t0 = time.perf_counter()
            data, _ = ctx.em_sample_data(pi, mu, S, n, seed=rep)
            t1 = time.perf_counter()
            ms, launches = ctx.timing_get("em_sample")
            assert launches == 1
            data.close()
            t2 = time.perf_counter()
            X, labels = ctx.em_sample(pi, mu, S, n, seed=rep)
            t3 = time.perf_counter()
            del X, labels
            t4 = time.perf_counter()
            Xs, _ = mix.sample(n, threads=args.threads)
            t5 = time.perf_counter()
            del Xs
            if rep:
                t_kernel.append(ms)
                t_handle.append(1e3 * (t1 - t0))
                t_host.append(1e3 * (t3 - t2))
                t_synth.append(1e3 * (t5 - t4))
        ctx.timing_enable(False)
        k, h, o, s = (statistics.median(v) for v in (t_kernel, t_handle, t_host, t_synth))
        gbs = n * (8.0 * d + 4.0) / (k * 1e-3) / 1e9
        pairs = n * ((d + 1) // 2) / (k * 1e-3) / 1e9
        lines.append("%9d %4d %4d %-12s %9.3f %8.0f %8.1f %10.2f %9.1f %9.1f %9.1f %10.1f %10.1f"
                     % (n, d, K, route, k, gbs, 100 * gbs / (COPY_TBS * 1e3), pairs, h, o, s, s / o, s / h))
        print(lines[-1], flush=True)
    ctx.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
