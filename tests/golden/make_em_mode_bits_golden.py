"""Records tests/golden/em_mode_bits.npz: what the EM entry points return in the three covariance modes, bit for bit, on the cases
of tests/em_mode_bits_cases.py. Needs a GPU (MI355X, gfx950).

    python tests/golden/make_em_mode_bits_golden.py

Every case is run twice in this process, and nothing is written unless the two runs agree in every bit. The fixture also holds the
device's compute-unit count ("device/compute_units").

The fixture was recorded ONCE, at commit dc32f42, before the covariance mode became one type from the C ABI to EM::fit. A recorded
value that differs from what the library computes means the library changed what it computes: fix the library, do not record again."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                       # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # the repository root

import em_mode_bits_cases as cases  # noqa: E402


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def main():
    from ml_amd import _lib
    ctx = _lib.Context()
    recorded, wrong_routes, unstable = {}, {}, []
    for name, run, case in cases.all_cases():
        out, wrong = run(ctx, case)
        again, _ = run(ctx, case)
        unstable += [key for key in out if key not in again or not same_bits(out[key], again[key])]
        recorded.update(out)
        if wrong:
            wrong_routes[name] = wrong
        print(f"{name}: {len(out)} fields" + (f", route differs from the expected one: {wrong}" if wrong else ""), flush=True)
    ctx.close()
    if unstable:
        sys.exit(f"two runs in one process differ, nothing written: {unstable}")
    import torch
    recorded["device/compute_units"] = np.uint32(torch.cuda.get_device_properties(0).multi_processor_count)
    np.savez_compressed(cases.FIXTURE, **recorded)
    print(f"{cases.FIXTURE}: {len(recorded)} fields, {os.path.getsize(cases.FIXTURE)} bytes")
    if wrong_routes:
        sys.exit(f"routes other than the expected ones: {wrong_routes}")


if __name__ == "__main__":
    main()
