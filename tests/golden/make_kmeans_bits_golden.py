"""Records tests/golden/kmeans_bits.npz: what the K-means entry points return, bit for bit, on the cases of
tests/kmeans_bits_cases.py. Needs a GPU (MI355X, gfx950).

    python tests/golden/make_kmeans_bits_golden.py

The fixture was recorded ONCE, at commit 3d2a3b2, before the family's shared pieces were factored out. A recorded value that differs
from what the library computes means the library changed what it computes: fix the library, do not record again."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                       # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # the repository root

import kmeans_bits_cases as cases  # noqa: E402


def main():
    from ml_amd import _lib
    ctx = _lib.Context()
    recorded, wrong_routes = {}, {}
    for name, run, case in cases.all_cases():
        out, wrong = run(ctx, case)
        recorded.update(out)
        if wrong:
            wrong_routes[name] = wrong
        print(f"{name}: {len(out)} fields" + (f", route differs from the expected one: {wrong}" if wrong else ""), flush=True)
    ctx.close()
    np.savez_compressed(cases.FIXTURE, **recorded)
    print(f"{cases.FIXTURE}: {len(recorded)} fields, {os.path.getsize(cases.FIXTURE)} bytes")
    if wrong_routes:
        sys.exit(f"routes other than the expected ones: {wrong_routes}")


if __name__ == "__main__":
    main()
