"""Device time of one weighted K-means step (mlhip_kmeans_step_weighted: the assignment of the shape's route without its own
accumulation, then the weighted form of the update sweep of device/kmeans.hip) against the unweighted step of the same build on the same
block (mlhip_kmeans_step: assignment + exact update sums), at the two benchmark shapes. Per step the kernels' HIP-event times
(mlhip_timing_*) are summed, and the MEDIAN over the repeated steps after a warm-up is kept.

Every shape runs in a child process of its own under a time limit (the parent never opens the GPU); a child that fails or runs out
of time ends the tool, nothing more is started. Writes profiles/kmeans_weighted_timing.txt.

    python tools/kmeans_weighted_timing.py [--repeats 15] [--warmup 3] [--limit 240] [--out profiles/kmeans_weighted_timing.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(12_500_000, 8, 256), (10_000_000, 32, 64)]


def sample(n, d, K, seed):
    rng = np.random.default_rng(seed)
    centres = 3.0 * rng.standard_normal((K, d))
    X = np.empty((n, d))
    for lo in range(0, n, 1_000_000):                     # in slabs: no second N x d temporary
        hi = min(n, lo + 1_000_000)
        X[lo:hi] = centres[rng.integers(0, K, hi - lo)] + rng.standard_normal((hi - lo, d))
    w = np.exp(rng.standard_normal(n))
    return X, w, centres + 0.2 * rng.standard_normal((K, d))


def timed_steps(ctx, step, kernels, warmup, repeats):
    """Median over `repeats` calls of step() of (device ms per named kernel family, wall ms of the whole call)."""
    for _ in range(warmup):
        step()
    dev, wall = {name: [] for name in kernels}, []
    for _ in range(repeats):
        ctx.timing_reset()
        t0 = time.perf_counter()
        step()
        wall.append(1e3 * (time.perf_counter() - t0))
        for name in kernels:
            ms, launches = ctx.timing_get(name)
            dev[name].append(ms * launches)
    return {name: statistics.median(v) for name, v in dev.items()}, statistics.median(wall)


def run_shape(n, d, K, warmup, repeats):
    from ml_amd import _lib
    ctx = _lib.Context()
    X, w, C0 = sample(n, d, K, 1000 + d)
    dt = _lib.Data(ctx, X)
    del X
    route = dt.kmeans_route(K)
    ctx.timing_enable(True)
    plain, plain_wall = timed_steps(ctx, lambda: dt.kmeans_step(C0), ("kmeans_assign",), warmup, repeats)
    dt.set_weights(w)
    weighted, weighted_wall = timed_steps(ctx, lambda: dt.kmeans_step(C0, weighted=True), ("kmeans_assign", "kmeans_weighted"), warmup, repeats)
    ctx.timing_enable(False)
    dt.close()
    ctx.close()
    return {"n": n, "d": d, "K": K, "route": route["kernel"] + ("+pad" if route["pad"] else ""), "plain": plain["kmeans_assign"],
            "assign": weighted["kmeans_assign"], "sweep": weighted["kmeans_weighted"], "plain_wall": plain_wall, "weighted_wall": weighted_wall}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds per shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_weighted_timing.txt"))
    ap.add_argument("--shape", type=int, nargs=3, help="(child) time this N d K and print one JSON line")
    args = ap.parse_args()
    if args.shape:
        print(json.dumps(run_shape(*args.shape, args.warmup, args.repeats)), flush=True)
        return 0
    lines = ["# tools/kmeans_weighted_timing.py: one K-means step, median of %d steps after %d warm-up steps, one process per shape" % (args.repeats, args.warmup),
             "# (a)  mlhip_kmeans_step: kmeans_assign (assignment + exact update sums)",
             "# (b)  mlhip_kmeans_step_weighted: kmeans_assign (assignment only, accumulate = 0) + kmeans_weighted (sweep + reduction)",
             "# device ms = HIP-event time of the kernels of one step; wall ms = the whole call (upload of the centroids, read-back, closing)",
             "# %10s %4s %4s %8s %10s %12s %11s %10s %8s %9s %9s" % ("N", "d", "K", "route", "(a) dev", "(b) assign", "(b) sweep", "(b) dev", "(b)/(a)",
                                                                 "(a) wall", "(b) wall")]
    costly = []
    for n, d, K in SHAPES:
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", str(n), str(d), str(K), "--repeats", str(args.repeats),
                                "--warmup", str(args.warmup)], capture_output=True, text=True, timeout=args.limit)
        if child.returncode != 0:
            sys.stderr.write(child.stdout + child.stderr)
            return child.returncode
        r = json.loads(child.stdout.strip().splitlines()[-1])
        total = r["assign"] + r["sweep"]
        if r["sweep"] > r["assign"]:
            costly.append(r)
        lines.append("  %10d %4d %4d %8s %10.4f %12.4f %11.4f %10.4f %8.2f %9.3f %9.3f" %
                     (n, d, K, r["route"], r["plain"], r["assign"], r["sweep"], total, total / r["plain"], r["plain_wall"], r["weighted_wall"]))
        print(lines[-1], flush=True)
    for r in costly:
        lines.append("# N=%d d=%d K=%d: the sweep costs MORE than the assignment itself (%.4f against %.4f ms)" %
                     (r["n"], r["d"], r["K"], r["sweep"], r["assign"]))
    if not costly:
        lines.append("# at both shapes the sweep costs less than the assignment itself")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
