"""Wall time of wa_gtsp_seam_tour_rules on the device beside wa_gtsp_seam_tour on the same costs, for profiles/seam_rules/README.md.

    python tools/seamrules_time.py                # 32 seams x 4096 starts, 256 seams x 256 starts: the old call, then the new one with
                                                  # no rules, with m random pairs, with m pairs and a quarter of the seams one-way
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/seamrules_time.py --once      # kernel time, in a run of its own

The anchored move set changes the pass counts, so the comparable figure is the time per pass (call time / passes_total)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

JOBS = ((32, 4096), (256, 256))   # (seams, starts), closed, or_len 3: the jobs of profiles/seamtour


def euclid(m, seed):
    rs = np.random.RandomState(seed)
    p = rs.uniform(0, 10, (2 * m, 3))
    return np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--once", action="store_true", help="each call once after its warm-up, nothing else (for a profiler run)")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import seamrules_ref as S
    from welding_robot_amd import api
    ctx = api.Context(0)
    print("device:", ctx.device_name)
    for m, n_starts in JOBS:
        d = euclid(m, m)
        kw = dict(closed=True, or_len=3, n_starts=n_starts, seed=1)
        b, a, fx = S.random_rules(m, m, True)
        calls = (("wa_gtsp_seam_tour", lambda: api.seam_tour(ctx, d, **kw)),
                 ("rules: none", lambda: api.seam_tour_rules(ctx, d, **kw)),
                 ("rules: %d pairs" % m, lambda: api.seam_tour_rules(ctx, d, b, a, None, **kw)),
                 ("rules: %d pairs, %d one-way" % (m, int((fx != 0).sum())), lambda: api.seam_tour_rules(ctx, d, b, a, fx, **kw)))
        for name, call in calls:
            r = call()   # warm-up: code object, LDS attribute, the context's blocks
            ts = []
            for _ in range(1 if args.once else args.reps):
                t = time.perf_counter()
                r = call()
                ts.append(time.perf_counter() - t)
            s = r["summary"]
            print("m=%d starts=%d %-28s: wall min %.4f s median %.4f s | passes per start mean %.1f min %d max %d | %.3f us per pass (wall min / passes_total) | "
                  "best %.3f (start %d)" % (m, n_starts, name, min(ts), float(np.median(ts)), r["start_passes"].mean(), r["start_passes"].min(),
                                            r["start_passes"].max(), 1e6 * min(ts) / s["passes_total"], r["cost"], s["best_start"]))
    ctx.close()


if __name__ == "__main__":
    main()
