#!/usr/bin/env python3
"""Where the converged phase of a plain `bench.py` goes, from a rocprofv3 --kernel-trace CSV of the run: window kernels, launches that return at
once, flushes and full generations, each with the gap in front of its dispatches.

  python tools/converged_split.py <rocprof output dir or kernel_trace.csv> <bench json line file> [--from-window N] [--empty-us X] [--walk-us Y] [--walk-ahead]

The timed region starts at the W-th k_walk_dev dispatch (W warm-up generations of a throw-away search, which commit nothing, are in front).  The
region reported starts at the generation in front of window kernel number N of the timed region (default 10: with bench.py's 50-generation calls
and --profile-every 10 a call has five windows, so window 10 covers generations 101-109 and the generation in front of it is generation 100) and
runs to the last dispatch of the timed search.  Windows are placed by the host alone, so the same N cuts parent and branch at the same generation,
whether or not the launches of committed generations are enqueued.

A generation's three launches are classed `at once` when the sweep-carrying launch took less than --empty-us (default 10; a sweep of the 128^3
field takes 13 us and more, a launch that returns at its top 2-5 us under the profiler), `flush` when they follow launches that returned at once --
or follow the window kernel directly with a walk launch shorter than --walk-us (default 3: a window that committed one generation) --, `full`
otherwise.  A speculative flush (two launches directly behind a window kernel, no walk launch) is a `flush` if its sweep ran and `at once` if it
was cancelled.  With owed evaporations (WA_CONVERGED_OWED) the flush of a carried window is one small launch: the table blocks of
k_apply_table alone, or the speculative pair whose sweep blocks returned at once; both are classed `rows` (a cancelled speculative flush, whose
two launches both return at once, cannot be told from the latter by its times and is counted there too).  The gap in front of a dispatch is its start minus the latest end of everything dispatched
before it.  The classes' kernel time and gaps add up to the region's span.

--walk-ahead: the trace is of a library with the carried walk (WA_CONVERGED_CARRIED_WALK): a carried window has no rows launch, and the walk launch
of the generation behind it stands directly behind the window kernel, enqueued ahead of the verdict.  Three launches directly behind a window kernel
whose sweep ran are then that `full` generation (its short walk is the carried one, not a launch that returned at once), and a walk launch that
nothing of its generation follows -- cancelled: the window was not carried -- is classed `walk ahead`."""
import csv
import glob
import json
import os
import sys

TRIO = ("k_walk_dev", "k_evap_rank_mark", "k_apply_table")


def opt(name, default):
    return float(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    path, jpath = sys.argv[1], sys.argv[2]
    d = json.loads([l for l in open(jpath).read().splitlines() if l.startswith("{")][-1])
    K, W = int(d["steps"]), int(d["warmup"])
    first_window, empty_us, walk_us = int(opt("--from-window", 10)), opt("--empty-us", 10.0), opt("--walk-us", 3.0)
    walk_ahead = "--walk-ahead" in sys.argv
    files = [path] if os.path.isfile(path) else glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for f in files for r in csv.DictReader(open(f)))
    # every dispatch with the gap in front of it
    disp, busy_until = [], None
    for a, b, k in rows:
        gap = 0.0 if busy_until is None else max(a - busy_until, 0) / 1e3
        busy_until = b if busy_until is None else max(busy_until, b)
        kind = "window" if "k_converged_run" in k else next((t for t in TRIO if t in k), None)
        disp.append(dict(kind=kind, us=(b - a) / 1e3, gap=gap, start=a, end=b))
    walks = [i for i, x in enumerate(disp) if x["kind"] == TRIO[0]]
    assert len(walks) > W, "%d walk dispatches in the trace, %d warm-up generations" % (len(walks), W)
    t0 = walks[W]
    if t0 > 0 and disp[t0 - 1]["kind"] == "window":
        t0 -= 1
    timed = [x for x in disp[t0:] if x["kind"]]
    # generations (walk, sweep + rank + mark, apply + table) and windows, in order
    items, i = [], 0
    while i < len(timed):
        if timed[i]["kind"] == "window":
            items.append(("window", [timed[i]]))
            i += 1
            continue
        if timed[i]["kind"] == TRIO[1]:   # a speculative flush: the two launches behind a window, no walk launch
            duo = timed[i:i + 2]
            assert tuple(x["kind"] for x in duo) == TRIO[1:], "dispatch %d of the timed region: %s" % (i, [x["kind"] for x in duo])
            items.append(("rows" if duo[0]["us"] < empty_us else "flush", [None] + duo))
            i += 2
            continue
        if timed[i]["kind"] == TRIO[2]:   # the rows launch of a carried window, alone
            items.append(("rows", [None, None, timed[i]]))
            i += 1
            continue
        if walk_ahead and (i + 1 >= len(timed) or timed[i + 1]["kind"] != TRIO[1]):
            items.append(("walk ahead", [timed[i]]))
            i += 1
            continue
        trio = timed[i:i + 3]
        assert tuple(x["kind"] for x in trio) == TRIO, "dispatch %d of the timed region: %s" % (i, [x["kind"] for x in trio])
        if trio[1]["us"] < empty_us:
            cls = "at once"
        elif items and items[-1][0] == "at once":
            cls = "flush"            # (launches that return at once are followed by the flush of their window)
        elif items and items[-1][0] == "window" and trio[0]["us"] < walk_us and not walk_ahead:
            cls = "flush"            # a window that committed its first generation alone
        else:
            cls = "full"
        items.append((cls, trio))
        i += 3
    wins = [n for n, (c, _) in enumerate(items) if c == "window"]
    assert len(wins) > first_window, "%d windows in the timed region" % len(wins)
    cut = wins[first_window] - 1
    gens_before = sum(1 for c, _ in items[:cut] if c != "window")
    region = items[cut:]
    region = [(c, [x for x in xs if x is not None]) for c, xs in region]
    by_kernel = lambda xs, name: [x for x in xs if x["kind"] == name or (name == "k_converged_run" and x["kind"] == "window")]
    span = (max(x["end"] for _, xs in region for x in xs) - region[0][1][0]["start"]) / 1e3
    print("timed region: %d generations enqueued as launches, %d windows; %d generations' launches in front of the cut (window %d)"
          % (sum(1 for c, _ in items if c != "window"), len(wins), gens_before, first_window))
    print("region: from the generation in front of window %d to the end, span %.1f us" % (first_window, span))
    print("| class | count | kernels us | gaps us | total us | share | per item us |")
    print("|---|---|---|---|---|---|---|")
    total = 0.0
    for cls in ("window", "at once", "flush", "rows", "walk ahead", "full"):
        mine = [xs for c, xs in region if c == cls]
        first_gap = region[0][1][0]["gap"] if region[0][0] == cls else 0.0      # (the gap in front of the region is not part of its span)
        kus, gus = sum(x["us"] for xs in mine for x in xs), sum(x["gap"] for xs in mine for x in xs) - first_gap
        total += kus + gus
        print("| %s | %d | %.1f | %.1f | %.1f | %.1f %% | %.2f |" % (cls, len(mine), kus, gus, kus + gus, 100 * (kus + gus) / span, (kus + gus) / max(len(mine), 1)))
    print("| all | %d | | | %.1f | %.1f %% | |" % (len(region), total, 100 * total / span))
    for cls in ("window", "at once", "flush", "rows", "walk ahead", "full"):
        mine = [xs for c, xs in region if c == cls]
        if not mine:
            continue
        for name in (("k_converged_run",) if cls == "window" else TRIO):
            sel = [x for xs in mine for x in by_kernel(xs, name)]
            if not sel:
                continue
            us, gaps = sorted(x["us"] for x in sel), sorted(x["gap"] for x in sel)
            print("  %-8s %-18s %3d launches  kernel min / median / max %6.2f / %6.2f / %6.2f us   gap in front %5.2f / %5.2f / %6.2f us"
                  % (cls, name, len(sel), us[0], us[len(us) // 2], us[-1], gaps[0], gaps[len(gaps) // 2], gaps[-1]))
    print("bench.py of this run: %.3f us per generation (under the profiler)" % (float(d["ms_per_step"]) * 1e3))
    return 0


if __name__ == "__main__":
    sys.exit(main())
