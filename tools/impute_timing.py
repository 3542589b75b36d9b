"""Times mlhip_em_impute (every NaN of a host block replaced by its conditional expectation, a pattern per row) in one process on one
GPU, on both routes, piece by piece.

    python tools/impute_timing.py [--shapes 1000000x16x16,1000000x32x64] [--reps 5] [--composed-rows 10000] [--out profiles/impute_timing.txt]

A shape is N x d x K, full covariances, rows drawn from the model. Pattern sets: `8` (eight fixed patterns dealt round robin),
`b0.1` and `b0.3` (every entry missing with that probability). Per shape and set, after one warm-up, the medians of `reps` calls of
  KERNEL    the whole call (wall clock, ms) and its pieces: plan (the host plan), upload (gathering the rows in plan order and
            enqueueing the copies), records and eval (HIP events of the two kernels, summed over their launches), download (from the
            last launch to the scattered result: it waits for the kernels, so `eval` is taken off), and what is left (the complete rows'
            scoring pass, the result's buffers);
  COMPOSED  the whole call. Where the set has more than a few hundred patterns the composed route is timed on the first
            --composed-rows rows only (one upload, one host conditioning and two launches per pattern: the whole block would take
            minutes) and reported with its own row and pattern counts; `per row` makes the two comparable;
  8 calls   for the 8-pattern set: eight EM.conditional_mean-style calls (mlhip_em_condition on the host + Data upload +
            em_conditional_means), one per pattern, what a user did by hand before.
`spread`: (max - min) / median of the KERNEL calls."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def gaps(X, kind, seed):
    rng = np.random.default_rng(seed)
    n, d = X.shape
    if kind == "8":
        masks = rng.random((8, d)) < 0.3
        masks[:, 0] = False                                      # (something observed)
        masks[:, 1] = True                                       # (something missing)
        missing = masks[np.arange(n) % 8]
    else:
        missing = rng.random((n, d)) < float(kind[1:])
    G = X.copy()
    G[missing] = np.nan
    return G


def timed_call(fn):
    t0 = time.perf_counter()
    out = fn()
    ms = 1e3 * (time.perf_counter() - t0)
    del out
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1000000x16x16,1000000x32x64")
    ap.add_argument("--sets", default="8,b0.1,b0.3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--composed-rows", type=int, default=10000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ml_amd import _lib, synth
    ctx = _lib.Context(0)
    lines = ["# medians of %d calls after one warm-up, ms; kernels by HIP events summed over their launches, the rest wall clock" % args.reps]
    names = ("impute_plan", "impute_upload", "em_impute_records", "em_impute", "impute_download")
    for shape in args.shapes.split(","):
        n, d, K = (int(v) for v in shape.split("x"))
        mix = synth.Mixture(d, K, seed=11)
        pi, mu, S = mix.weights, mix.means, mix.covs
        X, _ = mix.sample(n, threads=16)
        for kind in args.sets.split(","):
            G = gaps(X, kind, 7)
            order, bounds, n_obs = _lib.em_impute_plan(G)
            P = len(n_obs)
            os.environ["MLHIP_IMPUTE"] = "kernel"
            route, launches = _lib.em_impute_route(d, K, G)
            assert route == "kernel"
            calls, parts = [], {k: [] for k in names}
            ctx.timing_enable(True)
            for rep in range(args.reps + 1):
                ctx.timing_reset()
                ms = timed_call(lambda: _lib.em_impute(ctx, pi, mu, S, G))
                if rep:
                    calls.append(ms)
                    for k in names:
                        avg, cnt = ctx.timing_get(k)
                        parts[k].append(avg * cnt)
            ctx.timing_enable(False)
            call = statistics.median(calls)
            p = {k: statistics.median(v) for k, v in parts.items()}
            download = p["impute_download"] - p["em_impute"]
            rest = call - p["impute_plan"] - p["impute_upload"] - p["em_impute_records"] - p["impute_download"]
            lines.append("N %d d %d K %d set %-4s patterns %7d | KERNEL %9.1f (spread %.2f, %d launches): plan %.1f upload %.1f records %.1f eval %.1f "
                         "download %.1f rest %.1f | per row %.3f us"
                         % (n, d, K, kind, P, call, (max(calls) - min(calls)) / call, launches, p["impute_plan"], p["impute_upload"],
                            p["em_impute_records"], p["em_impute"], download, rest, 1e3 * call / n))
            print(lines[-1], flush=True)
            # the composed route: the whole block where the patterns are few, else a prefix
            os.environ["MLHIP_IMPUTE"] = "composed"
            rows = n if P <= 512 else min(n, args.composed_rows)
            Gc = np.ascontiguousarray(G[:rows])
            Pc = len(_lib.em_impute_plan(Gc)[2])
            reps = args.reps if P <= 512 else 3
            comp = [timed_call(lambda: _lib.em_impute(ctx, pi, mu, S, Gc)) for _ in range(reps + 1)][1:]
            c = statistics.median(comp)
            lines.append("N %d d %d K %d set %-4s patterns %7d | COMPOSED on %d rows, %d patterns: %9.1f (spread %.2f, %d calls) | per row %.3f us, per pattern %.3f ms"
                         % (n, d, K, kind, P, rows, Pc, c, (max(comp) - min(comp)) / c, reps, 1e3 * c / rows, c / max(Pc, 1)))
            print(lines[-1], flush=True)
            os.environ.pop("MLHIP_IMPUTE")
            if kind != "8":
                continue

            def by_hand():
                out = G.copy()
                for p0 in range(P):
                    rows_of = order[bounds[p0]:bounds[p0 + 1]]
                    observed = np.nonzero(~np.isnan(G[rows_of[0]]))[0]
                    if len(observed) in (0, d):
                        continue
                    missing = np.nonzero(np.isnan(G[rows_of[0]]))[0]
                    cond = _lib.em_condition(mu, S, observed)
                    data = _lib.Data(ctx, np.ascontiguousarray(G[rows_of][:, observed]))
                    y = data.em_conditional_means(pi, *cond)
                    data.close()
                    out[np.ix_(rows_of, missing)] = y
                return out
            hand = [timed_call(by_hand) for _ in range(args.reps + 1)][1:]
            h = statistics.median(hand)
            lines.append("N %d d %d K %d set %-4s patterns %7d | %d conditional-mean calls by hand: %9.1f (spread %.2f)"
                         % (n, d, K, kind, P, P, h, (max(hand) - min(hand)) / h))
            print(lines[-1], flush=True)
        del X
    ctx.close()
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
