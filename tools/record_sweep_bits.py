#!/usr/bin/env python
"""Record tests/data/sweep_bits.json: SHA-256 of the chain and the trace bytes, and the
final states, of the cases of tests/sweep_bits_cases.py, run through the Python sampler
API on the MI355X with the library in the tree (or OLPE_LIB).

The recording pins the FAST3 sweep's results bit for bit (tests/test_gpu_sweep_bits.py).
It was made once, with the library of the commit before the shape-table rows of the
64-row sweep were taken from registers.  Re-record only with an explanation of why the
bits changed.

  python tools/record_sweep_bits.py [--out FILE] [--check]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]


def main():
    import sweep_bits_cases as sb
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=sb.RECORDING)
    ap.add_argument("--check", action="store_true",
                    help="compare with the file instead of writing it")
    args = ap.parse_args()

    def delenv(k):
        os.environ.pop(k, None)

    rec = {}
    for cid, (nsrc, _, env) in sb.CASES.items():
        chain, tr, state = sb.run_case(cid, os.environ.__setitem__, delenv)
        rec[cid] = sb.digest(chain, tr, state)
        oc = sb.shape_outcomes(nsrc, tr)
        print(f"{cid} {env}: chain {rec[cid]['chain_sha256'][:16]} trace "
              f"{rec[cid]['trace_sha256'][:16]}; shape proposals " +
              ", ".join(f"{k[0]} {'accepted' if k[1] else 'rejected'} {v}" for k, v in oc.items()))
    if args.check:
        with open(args.out) as f:
            old = json.load(f)
        bad = [c for c in rec if old.get(c) != rec[c]]
        print("differs: " + ", ".join(bad) if bad else "equal to " + args.out)
        return 1 if bad else 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote " + args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
