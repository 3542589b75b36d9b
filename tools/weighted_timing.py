"""Cost of row weights: seconds per EM iteration (mlhip_em_iterate, tolerances 0) at N=10M d=32 K=64 and N=1M d=4 K=3,
(i) unweighted, (ii) weighted with every weight 1, (iii) weighted with half of the weights 0. One JSON line per shape.
`--unweighted-only`: (i) alone -- what a library without mlhip_data_set_weights can run (MLHIP_LIBRARY selects the library).

    python tools/weighted_timing.py [--steps 10] [--repeats 3] [--unweighted-only]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(10_000_000, 32, 64), (1_000_000, 4, 3)]


def per_iteration(data, pi0, mu0, S0, steps, repeats):
    data.em_iterate(pi0, mu0, S0, 2)                       # warm-up: code objects, workspace
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        done = data.em_iterate(pi0, mu0, S0, steps)[0]
        times.append((time.perf_counter() - t0) / done)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--unweighted-only", action="store_true")
    args = ap.parse_args()
    from ml_amd import _lib, synth
    ctx = _lib.Context(0)
    for n, d, K in SHAPES:
        mix = synth.Mixture(d, K, seed=77)
        X, _ = mix.sample(n)
        data = _lib.Data(ctx, X)
        pi0, mu0 = np.full(K, 1.0 / K), mix.initial_means()
        _, cov = data.sample_covariance()
        S0 = np.stack([cov] * K)
        out = {"N": n, "d": d, "K": K, "steps": args.steps, "library": _lib.LIB_PATH,
               "unweighted_ms": 1e3 * per_iteration(data, pi0, mu0, S0, args.steps, args.repeats),
               "unweighted_route": data.em_route(K)}
        if not args.unweighted_only:
            data.set_weights(np.ones(n))
            out["weighted_route"] = data.em_route(K)
            out["weights_all_one_ms"] = 1e3 * per_iteration(data, pi0, mu0, S0, args.steps, args.repeats)
            w = np.ones(n)
            w[np.random.default_rng(1).random(n) < 0.5] = 0.0
            data.set_weights(w)
            out["weights_half_zero_ms"] = 1e3 * per_iteration(data, pi0, mu0, S0, args.steps, args.repeats)
        data.close()
        print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
