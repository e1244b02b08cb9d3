#!/usr/bin/env python3
"""Write tests/golden/fold_bits_parent.npz: the summaries of tests/test_gpu_fold_bits.py's
cases (astrometry, photometry, covariance, autocorrelation, moments) as the library in the
tree, or OLPE_LIB, computes them on the GPU.

Run it with the library of the commit whose results are to be pinned, before changing the
folds:  python tools/record_fold_bits_golden.py [OUT.npz]
Every case runs twice; nothing is written unless the two runs agree in every bit.
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import test_gpu_fold_bits as T  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden",
                                                             T.GOLDEN + ".npz")
    rec = {}
    for case, run in T.CASES.items():
        a, b = run(), run()
        diff = T.differing(a, b)
        if diff:
            sys.exit(f"{case}: two runs of the same library differ in {diff}; nothing written")
        print(f"{case}: " + ", ".join(f"{k}{list(v.shape)}" for k, v in a.items()))
        rec.update({f"{case}/{k}": v for k, v in a.items()})
    np.savez_compressed(out, **rec)
    print(f"wrote {out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
