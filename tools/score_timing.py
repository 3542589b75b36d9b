"""Times mlhip_em_score against the sequence a caller had before it -- mlhip_em_expectation + mlhip_em_labels on a fresh handle --
in one process on one GPU: HIP-event kernel times (mlhip_timing_get) and the device memory each sequence holds at its peak.

    python tools/score_timing.py [--n 10000000] [--shapes 32x64,2x3,8x32] [--reps 3] [--out profiles/score_timing.txt]

Per shape, after one warm-up of each, `reps` alternating repetitions; the table shows the medians. The fused pass reads the block
once and writes 12 bytes per row: its effective bandwidth (8 d + 12 bytes per row) is set against the streaming read of DESIGN.md
section 3.1. Wrap the same command in `rocprofv3 --kernel-trace --stats --` for the profiler's view of the same kernels."""
import argparse
import ctypes
import os
import statistics
import sys
import threading

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STREAM_READ_TBS = 6.33


def _hip():
    for name in ("libamdhip64.so", "libamdhip64.so.6", "/opt/rocm/lib/libamdhip64.so"):
        try:
            return ctypes.CDLL(name)
        except OSError:
            pass
    return None


def _used_bytes(hip):
    if hip is None:
        return float("nan")
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total))
    return total.value - free.value


class _Peak:
    """Largest device memory in use while the block runs, sampled from a second thread every millisecond."""

    def __init__(self, hip):
        self.hip, self.peak, self._stop = hip, 0, threading.Event()

    def __enter__(self):
        self.peak = _used_bytes(self.hip)
        self._t = threading.Thread(target=self._poll)
        self._t.start()
        return self

    def _poll(self):
        while not self._stop.wait(0.001):
            self.peak = max(self.peak, _used_bytes(self.hip))

    def __exit__(self, *exc):
        self._stop.set()
        self._t.join()
        self.peak = max(self.peak, _used_bytes(self.hip))


def _kernel_ms(ctx, names):
    return sum(ms * cnt for ms, cnt in (ctx.timing_get(n) for n in names))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--shapes", default="32x64,2x3,8x32")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ml_amd import _lib, synth
    hip = _hip()
    ctx = _lib.Context(0)
    lines = ["# n = %d, %d alternating repetitions after one warm-up each; kernel time by HIP events (ms), medians" % (args.n, args.reps),
             "# composed = the E-step kernel of mlhip_em_expectation + the label kernel of mlhip_em_labels (families em_estep + em_resp),",
             "# fused = mlhip_em_score's kernel(s); peak = device memory the call adds",
             "%4s %4s %-10s %10s %10s %7s %9s %12s %12s" % ("d", "K", "route", "composed", "fused", "ratio", "GB/s", "peak comp MB", "peak fused MB")]
    for shape in args.shapes.split(","):
        d, K = (int(v) for v in shape.split("x"))
        mix = synth.Mixture(d, K, seed=11)
        X, _ = mix.sample(args.n)
        pi, mu, S = np.full(K, 1.0 / K), mix.initial_means(), np.stack([np.cov(X[:100000].T)] * K)
        base = _used_bytes(hip)
        dt = _lib.Data(ctx, X)
        resident = _used_bytes(hip)
        route = dt.em_score_route(K)
        ctx.timing_enable(True)
        t_comp, t_fused, peak_comp, peak_fused = [], [], 0, 0
        for rep in range(args.reps + 1):
            fresh = _lib.Data(ctx, X)                       # the composed sequence on a fresh handle, as a caller would
            before = _used_bytes(hip)
            ctx.timing_reset()
            with _Peak(hip) as pk:
                fresh.em_expectation(pi, mu, S)
                fresh.em_labels(K)
            ms = _kernel_ms(ctx, ("em_estep", "em_resp"))
            peak_comp = max(peak_comp, pk.peak - before)
            fresh.close()
            before = _used_bytes(hip)
            ctx.timing_reset()
            with _Peak(hip) as pk:
                dt.em_score(pi, mu, S)
            ms_f = _kernel_ms(ctx, ("em_score", "em_estep"))
            peak_fused = max(peak_fused, pk.peak - before)
            if rep:
                t_comp.append(ms)
                t_fused.append(ms_f)
        ctx.timing_enable(False)
        dt.close()
        c, f = statistics.median(t_comp), statistics.median(t_fused)
        gbs = args.n * (8.0 * d + 12.0) / (f * 1e-3) / 1e9
        lines.append("%4d %4d %-10s %10.3f %10.3f %7.3f %9.0f %12.0f %12.0f   # %.0f %% of %.2f TB/s; resident block %.0f MB"
                     % (d, K, route, c, f, f / c, gbs, peak_comp / 2 ** 20, peak_fused / 2 ** 20, 100 * gbs / (STREAM_READ_TBS * 1e3),
                        STREAM_READ_TBS, (resident - base) / 2 ** 20))
        print(lines[-1], flush=True)
    ctx.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
