#!/usr/bin/env python3
"""Seeding wall time of KPP and FixedPointKPP on one GPU (d = 8, K = 256 by default), through the path `fit` takes
(`_run_on_device`: upload + the initialiser). The seeding time is the K-centroid call less the 1-centroid call (upload and the
first, uniform pick). Where KPP's draws mostly fall back to the host (N >= --kpp-full-limit), only its first --kpp-draws draws
are timed and the per-draw time is extrapolated to K - 1 draws; the line says so. One JSON line per (initialiser, N).

    python tools/fixed_point_kpp_timing.py [--n 1e6,1.25e7,3e7,1e8] [--k 256] [--fp-only]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ml_amd.cppyml import clustering as cl  # noqa: E402


def timed(init, X, K):
    t = time.perf_counter()
    init._run_on_device(X, K, seed=7)
    return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1e6,1.25e7,3e7,1e8")
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--k", type=int, default=256)
    ap.add_argument("--fp-only", action="store_true")
    ap.add_argument("--kpp-full-limit", type=float, default=2e7)
    ap.add_argument("--kpp-draws", type=int, default=8)
    a = ap.parse_args()
    for n in (int(float(v)) for v in a.n.split(",")):
        X = np.random.default_rng(1).random((n, a.d))
        timed(cl.FixedPointKPP(), X[:4096].copy(), 2)                 # first use of the code objects
        base = min(timed(cl.FixedPointKPP(), X, 1) for _ in range(2))
        full = timed(cl.FixedPointKPP(), X, a.k)
        print(json.dumps({"init": "FixedPointKPP", "n": n, "d": a.d, "k": a.k, "seeding_s": round(full - base, 4),
                          "upload_and_first_s": round(base, 4), "extrapolated": False}), flush=True)
        if a.fp_only:
            continue
        base = min(timed(cl.KPP(), X, 1) for _ in range(2))
        if n < a.kpp_full_limit:
            full, extrapolated = timed(cl.KPP(), X, a.k) - base, False
        else:
            part = timed(cl.KPP(), X, 1 + a.kpp_draws) - base
            full, extrapolated = part / a.kpp_draws * (a.k - 1), True
        print(json.dumps({"init": "KPP", "n": n, "d": a.d, "k": a.k, "seeding_s": round(full, 4), "upload_and_first_s": round(base, 4),
                          "extrapolated": extrapolated, "timed_draws": a.kpp_draws if extrapolated else a.k - 1}), flush=True)


if __name__ == "__main__":
    main()
