"""Silhouette timings behind profiles/silhouette_timing.txt (run on an MI355X: python tools/silhouette_timing.py [output file]): medians of 5 after
one warm-up call, per shape the register tier with both column feeds and the plain tier, alternating in one process, every call's
values compared bit for bit; kernel time from the context's event timers, call time from the host clock; then scikit-learn on the
host's threads at N = 20 000. Writes its lines to the output file too (default: silhouette_timing_run.txt in the working directory)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ml_amd import _lib  # noqa: E402

OUT = open(sys.argv[1] if len(sys.argv) > 1 else "silhouette_timing_run.txt", "w")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    OUT.write(line + "\n")
    OUT.flush()


def pad(d):
    return next(p for p in (2, 4, 8, 16, 32) if d <= p)


def bound_ms(pairs, d, rate):
    return pairs / 64 * (2 * pad(d) + 19) / rate * 1e3


def variants(d):
    return (("scalar", {"MLHIP_SILHOUETTE_FEED": "scalar"}), ("lds", {"MLHIP_SILHOUETTE_FEED": "lds"}), ("plain", {"MLHIP_SILHOUETTE": "plain"}))


def measure(ctx, data, labels, rows, d, pairs, reps=5):
    res = {}
    order = variants(d)
    times = {name: ([], []) for name, _ in order}
    ref = None
    for rep in range(reps + 1):
        for name, env in order:
            if name == "plain" and rep > 0 and times[name][1] and np.median(times[name][1]) > 4.0 and len(times[name][1]) >= 3:
                continue
            for k in ("MLHIP_SILHOUETTE", "MLHIP_SILHOUETTE_FEED"):
                os.environ.pop(k, None)
            os.environ.update(env)
            ctx.timing_reset()
            t0 = time.perf_counter()
            s = _lib.silhouette(data, labels, rows=rows)
            wall = time.perf_counter() - t0
            ms, launches = ctx.timing_get("silhouette")
            if ref is None:
                ref = s
            assert np.array_equal(ref.view(np.uint64), s.view(np.uint64)), name
            if rep > 0:
                times[name][0].append(ms * launches)
                times[name][1].append(wall)
    for name, _ in order:
        k, w = np.median(times[name][0]), np.median(times[name][1])
        res[name] = (k, w, len(times[name][0]))
    say(f"    vector-unit issue bound, {2 * pad(d) + 19} instructions per pair: {bound_ms(pairs, d, 0.484e12):8.2f} ms at the sustained v_fma_f64 rate (5.06 cycles),"
        f" {bound_ms(pairs, d, 0.614e12):8.2f} ms at 4 cycles")
    for name, (k, w, n) in res.items():
        say(f"    {name:7s} kernel {k:10.2f} ms  {pairs / k / 1e6:9.1f} G pairs/s   call {w * 1e3:10.1f} ms   (median of {n})")
    return res


def main():
    ctx = _lib.Context()
    ctx.timing_enable(True)
    rng = np.random.default_rng(0)
    say("# silhouette timing, MI355X, fp64; kernel = the pair kernel's launches of one call (event timers), call = host clock")
    for d in (2, 8, 32):
        for K in (8, 64):
            n = 100_000
            centres = rng.normal(size=(K, d)) * 4
            labels = rng.integers(0, K, size=n)
            X = np.ascontiguousarray(centres[labels] + rng.normal(size=(n, d)))
            data = _lib.Data(ctx, X)
            say(f"N = {n} all rows, d = {d}, K = {K}: {n * n:.3g} pairs")
            measure(ctx, data, labels, None, d, float(n) * n)
            data.close()
    n, d, K, m = 10_000_000, 32, 64, 10_000
    centres = rng.normal(size=(K, d)) * 4
    labels = rng.integers(0, K, size=n)
    X = rng.standard_normal((n, d))
    X += centres[labels]
    data = _lib.Data(ctx, X)
    rows = np.sort(rng.choice(n, m, replace=False))
    say(f"N = {n}, m = {m} evaluated rows, d = {d}, K = {K}: {float(n) * m:.3g} pairs")
    measure(ctx, data, labels, rows, d, float(n) * m)
    data.close()
    del X
    for k in ("MLHIP_SILHOUETTE", "MLHIP_SILHOUETTE_FEED"):
        os.environ.pop(k, None)
    # scikit-learn on the host's threads
    n, d, K = 20_000, 32, 8
    centres = rng.normal(size=(K, d)) * 4
    labels = rng.integers(0, K, size=n)
    X = np.ascontiguousarray(centres[labels] + rng.normal(size=(n, d)))
    try:
        from sklearn.metrics import silhouette_samples
        silhouette_samples(X[:2000], labels[:2000])
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            ref = silhouette_samples(X, labels)
            ts.append(time.perf_counter() - t0)
        say(f"sklearn.metrics.silhouette_samples N = {n}, d = {d}, K = {K}, {os.environ.get('OMP_NUM_THREADS', '?')} threads: {np.median(ts) * 1e3:.1f} ms (median of 5) = {n * n / np.median(ts) / 1e9:.3f} G pairs/s")
        data = _lib.Data(ctx, X)
        _lib.silhouette(data, labels)
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            s = _lib.silhouette(data, labels)
            ts.append(time.perf_counter() - t0)
        say(f"this library, same sample: call {np.median(ts) * 1e3:.1f} ms (median of 5); max |s - sklearn| = {np.max(np.abs(s - ref)):.3g}")
        data.close()
    except ImportError as e:
        say(f"sklearn not available here: {e}: not measured")
    ctx.close()


main()
