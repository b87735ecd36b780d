#!/usr/bin/env python3
"""One loop kernel of a plain `bench.py` run, averaged over ranges of generations: a rocprofv3 --kernel-trace CSV is cut at the timed
region exactly like tools/timed_window_stats.py does (a plain run enqueues W warm-up generations, then K timed ones: dispatches
[W, W + K) of the kernel), and the window is split at the given generation numbers.

  python tools/kernel_by_generation.py <rocprof output dir or kernel_trace.csv> <bench json line file> [--kernel k_apply_table] [--cuts 20,200]
"""
import argparse
import csv
import glob
import json
import os


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("bench_json")
    ap.add_argument("--kernel", default="k_apply_table")
    ap.add_argument("--cuts", default="20,200", help="generations at which a new range starts")
    a = ap.parse_args()
    d = json.loads([l for l in open(a.bench_json).read().splitlines() if l.startswith("{")][-1])
    K, W = int(d["steps"]), int(d["warmup"])
    files = [a.trace] if os.path.isfile(a.trace) else glob.glob(os.path.join(a.trace, "**", "*kernel_trace.csv"), recursive=True)
    rows = []
    for f in files:
        for r in csv.DictReader(open(f)):
            if a.kernel in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows.sort()
    assert len(rows) >= W + K, "%s: %d dispatches in the trace, the command enqueued at least %d" % (a.kernel, len(rows), W + K)
    us = [(e - s) / 1e3 for s, e in rows[W:W + K]]
    edges = [0] + [int(c) for c in a.cuts.split(",") if int(c) < K] + [K]
    print("%s, timed region of %d generations (%d warm-up dispatches in front): average us per launch" % (a.kernel, K, W))
    for lo, hi in zip(edges, edges[1:]):
        part = us[lo:hi]
        print("  generations %3d-%3d: avg %6.2f  min %6.2f  max %6.2f  (%d launches, %.1f us in all)"
              % (lo, hi - 1, sum(part) / len(part), min(part), max(part), len(part), sum(part)))
    print("  all               : avg %6.2f  min %6.2f  max %6.2f" % (sum(us) / len(us), min(us), max(us)))


if __name__ == "__main__":
    main()
