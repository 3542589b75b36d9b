#!/usr/bin/env python3
"""Where a tile of the screened E-step (device/em_estep_screen.hip) spends its time: MLHIP_ESTEP_SCREEN_PROFILE=1 runs the kernel's
stamping form -- thread 0 of every workgroup stamps the 100 MHz clock at the phase boundaries of the workgroup's second tile -- and the
runtime prints the spans, averaged over the workgroups, on stderr. This tool runs a few passes of one shape in a child process with
the switch set, reads those lines and prints each span in microseconds, in shader cycles (at --mhz) and as a share of the tile.
The stamping form's fences forbid overlaps the plain kernel has: read the shares, not the length.
The five spans, whatever the tile size the dimension is instantiated with (the line names it): "stage" ends when the sample's
maximum is known (loads, lower bounds, the barrier that joins the halves); "buckets" is the loop that decides the candidates and
ballots them into the lists, the tile's stores, the issue of the next tile's loads and the barrier that closes them; "record copy" and
"evaluation" are wave 0's components (tile / 32 waves share the K components: eight of 64 in the 256-sample form, sixteen in the
128-sample one); "end barrier" is wave 0's wait for the other waves.

    python tools/estep_screen_phases.py [N d K] [--mhz 2400] > profiles/estep_screen_pair_phases.txt
"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(n, d, K):
    sys.path.insert(0, ROOT)
    import numpy as np
    from ml_amd import _lib, synth
    mix = synth.Mixture(d, K)
    X, _ = mix.sample(n, stream=0)
    ctx = _lib.Context()
    dt = _lib.Data(ctx, X)
    _, cov = dt.sample_covariance()
    p = (np.full(K, 1.0 / K), mix.initial_means(), np.stack([cov] * K))
    for _ in range(4):                                  # the first pass is dense, every later one screened (and stamped)
        p = dt.em_step(*p)[1:]
    print("counts", dt.em_screen_counts(), flush=True)
    dt.close()
    ctx.close()


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    mhz = float(sys.argv[sys.argv.index("--mhz") + 1]) if "--mhz" in sys.argv else 2400.0
    if "--mhz" in sys.argv:
        args.remove(sys.argv[sys.argv.index("--mhz") + 1])
    if args and args[0] == "child":
        return child(*(int(v) for v in args[1:4]))
    n, d, K = (int(v) for v in args[:3]) if len(args) >= 3 else (10_000_000, 32, 64)
    env = dict(os.environ, MLHIP_ESTEP_SCREEN="1", MLHIP_ESTEP_SCREEN_PROFILE="1")
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "child", str(n), str(d), str(K)], env=env, capture_output=True, text=True)
    if run.returncode != 0:
        sys.stderr.write(run.stderr)
        sys.exit(f"the profiled run failed ({run.returncode})")
    print(f"screened E-step, stamping form, N={n} d={d} K={K}; cycles at {mhz:.0f} MHz; {run.stdout.strip()}")
    lines = [ln for ln in run.stderr.splitlines() if ln.startswith("[mlhip] screened E-step")]
    for t, ln in enumerate(lines):
        print(f"pass {t + 2}: {ln.split(':', 1)[0].replace('[mlhip] screened E-step, ', '')}")
        spans = re.findall(r"(stage|buckets|record copy|evaluation|end barrier|tile) ([0-9.]+)", ln.split(":", 1)[1])
        whole = float(dict(spans)["tile"])
        for name, us in spans:
            us = float(us)
            print(f"    {name:14s} {us:8.2f} us  {us * mhz:9.0f} cycles  {100 * us / whole:5.1f} %")
    if not lines:
        sys.exit("no stamps came back (no screened pass, or no workgroup had a second tile)")


if __name__ == "__main__":
    main()
