#!/usr/bin/env python3
"""Write tests/golden/shape_slots_parent.npz: the run of tests/test_gpu_shape_slots.py
(64x64, 2 sources, FAST, 16 waves, 8 walkers, seeds 1000-1007, the bench's start, 400
iterations, trace on) as the library in the tree computes it on the GPU.

Run it with the library of the commit whose results are to be pinned, before changing
the sampler:  python tools/record_shape_slots_golden.py [OUT.npz]
It also prints the slot-history counts and the distance from the oracle, so that the
test's conditions are known to hold for the recorded run.
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import test_gpu_shape_slots as T  # noqa: E402
from oracle import olpe_oracle as ora  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden",
                                                             T.GOLDEN + ".npz")
    img = T.bench_frame()
    p0 = T.bench_start(img)
    a = T.run(img, p0, {"OLPE_WPB": "16"})
    b = T.run(img, p0, {"OLPE_WPB": "16"})
    T.assert_same(a, b, "two runs of the same library")
    for name, cnt in T.slot_classes(a["trace"]).items():
        print(f"{name}: per walker {cnt.tolist()}")
    dm, err, _, _ = ora.noise_model(img, 1.0, 1, 1, 2)
    worst = 0.0
    for w, sd in enumerate(T.SEEDS):
        ref, rtr = ora.Walker(dm, err, p0, sd).run(T.IT, trace=True)
        same = np.array_equal(a["trace"][w, :, 5] > 0.5, np.array([t[4] for t in rtr], bool))
        with np.errstate(all="ignore"):
            rel = np.nanmax(np.abs(a["chain"][w] - ref) / np.abs(ref))
        worst = max(worst, rel)
        print(f"walker {w}: accept decisions {'equal' if same else 'DIFFER'}, chain rel {rel:.3e}")
    print(f"oracle: worst chain rel {worst:.3e} (tolerance {T.TRAJ_TOL:g})")
    # the guard-edge run whose refused proposals take the 16-wave sampler's exact sweep
    eimg, ep0, eseeds = T.fallback_start("exact")
    e = T.run(eimg, ep0, {"OLPE_WPB": "16"}, eseeds, 200)
    T.assert_same(e, T.run(eimg, ep0, {"OLPE_WPB": "16"}, eseeds, 200), "two guard-edge runs")
    lvl = T.sweeps_taken(ep0, e)
    print(f"guard edge: {(lvl == 3).sum()} proposals take FAST3, {(lvl < 2).sum()} the exact sweep")
    np.savez_compressed(out, p0=p0, seeds=np.array(T.SEEDS), edge_p0=ep0,
                        edge_seeds=np.array(eseeds), **a, **{"edge_" + k: v for k, v in e.items()})
    print(f"wrote {out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
