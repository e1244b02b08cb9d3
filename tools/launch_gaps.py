#!/usr/bin/env python
"""The edge between consecutive sampler launches, from a rocprofv3 kernel trace.

    tools/launch_gaps.py <dir or *_kernel_trace.csv> [skip]

For the olpe_gibbs_kernel dispatches in start order (the first `skip`, default 5, are the
warm-up): the end-to-start gap between consecutive ones (negative = the next launch started
inside its predecessor's tail), the kernels that ran between them, and the step (start to
start).  DESIGN.md §7 / profiles/r17.
"""
import csv
import glob
import os
import sys


def main():
    path = sys.argv[1]
    skip = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    if os.path.isdir(path):
        path = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))[0]
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"],
                         r.get("Queue_Id", "?")))
    rows.sort()
    gibbs = [i for i, r in enumerate(rows) if "olpe_gibbs_kernel" in r[2]][skip:]
    gaps, steps, durs, between, overl = [], [], [], [], 0
    for a, b in zip(gibbs, gibbs[1:]):
        s0, e0 = rows[a][:2]
        s1, e1 = rows[b][:2]
        gaps.append((s1 - e0) / 1e3)
        steps.append((s1 - s0) / 1e3)
        durs.append((e0 - s0) / 1e3)
        overl += s1 < e0
        between.append(sum(1 for r in rows[a + 1:b] if r[0] >= e0 and r[1] <= s1))
    n = len(gaps)
    if not n:
        print("no consecutive sampler dispatches after the warm-up")
        return
    queues = sorted({rows[i][3] for i in gibbs})
    mean = lambda v: sum(v) / len(v)
    print(f"{os.path.basename(path)}: {n + 1} sampler dispatches on queues {queues}")
    print(f"  kernel span      mean {mean(durs):10.1f} us")
    print(f"  start to start   mean {mean(steps):10.1f} us")
    print(f"  end-to-start gap mean {mean(gaps):10.1f} us  min {min(gaps):.1f}  max {max(gaps):.1f}"
          f"  = {100 * mean(gaps) / mean(steps):.2f} % of the step")
    print(f"  launches that started before their predecessor ended: {overl} of {n}")
    print(f"  other kernels wholly inside the gap: {mean(between):.2f} per edge")


if __name__ == "__main__":
    main()
