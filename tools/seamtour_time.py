"""Wall time of wa_gtsp_seam_tour on the device, for profiles/seamtour/README.md.

    python tools/seamtour_time.py                 # 32 seams x 4096 starts, 256 seams x 256 starts, the gap to the exact tour on M = 12..16
    python tools/seamtour_time.py --numpy         # the same two jobs in the numpy restatement (no device; a sample of the starts, scaled)
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/seamtour_time.py --once     # kernel time, in a run of its own

Evaluations are counted, not measured: passes_total x the moves of one pass (moves_per_pass below)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

JOBS = ((32, 4096), (256, 256))   # (seams, starts), closed, or_len 3


def euclid(m, seed):
    rs = np.random.RandomState(seed)
    p = rs.uniform(0, 10, (2 * m, 3))
    return np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1))


def moves_per_pass(M, or_len):
    a = M * (M + 1) // 2 - 1 if M >= 2 else 0
    b = sum(2 * (M - L + 1) * (M - L - 1) for L in range(1, min(or_len, M - 2) + 1))
    return a + b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--numpy", action="store_true")
    ap.add_argument("--once", action="store_true", help="each job once, nothing else (for a profiler run)")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if args.numpy:
        import seamtour_ref as R
        for m, n_starts in JOBS:
            sample = min(n_starts, 64 if m <= 64 else 2)
            t = time.perf_counter()
            r = R.seam_tour(euclid(m, m), m, n_starts=sample, seed=1)
            dt = time.perf_counter() - t
            print("numpy m=%d: %d of %d starts in %.2f s -> %.1f s for all (%.1f passes per start)"
                  % (m, sample, n_starts, dt, dt * n_starts / sample, r["start_passes"].mean()))
        return
    from welding_robot_amd import api
    ctx = api.Context(0)
    print("device:", ctx.device_name)
    for m, n_starts in JOBS:
        d = euclid(m, m)
        kw = dict(closed=True, or_len=3, n_starts=n_starts, seed=1)
        r = api.seam_tour(ctx, d, **kw)   # warm-up: code object, LDS attribute, the context's blocks
        if args.once:
            continue
        ts = []
        for _ in range(args.reps):
            t = time.perf_counter()
            r = api.seam_tour(ctx, d, **kw)
            ts.append(time.perf_counter() - t)
        s = r["summary"]
        ev = s["passes_total"] * moves_per_pass(s["M"], 3)
        print("m=%d starts=%d: wall min %.4f s median %.4f s | passes per start mean %.1f min %d max %d | %d evaluations, %.3g per s (wall min) | "
              "cost start0 in %.3f, best %.3f (start %d)"
              % (m, n_starts, min(ts), float(np.median(ts)), r["start_passes"].mean(), r["start_passes"].min(), r["start_passes"].max(),
                 ev, ev / min(ts), s["start0_cost_q_in"] / api.SEAM_Q, r["cost"], s["best_start"]))
    if args.once:
        return
    # the searched cost against the optimum, M = 12 .. 16, Euclidean and small-integer costs
    for n_starts in (1, 16, 256):
        gaps, hit = [], 0
        for M in range(12, 17):
            for seed in range(8):
                d = euclid(M, 1000 + 16 * M + seed)
                if seed % 2:
                    d = np.rint(d)
                    d[d == 0] = 1.0
                ex = api.seam_tour_exact(ctx, d)["cost_q"]
                got = api.seam_tour(ctx, d, n_starts=n_starts, seed=seed)["cost_q"]
                gaps.append(got / ex - 1.0)
                hit += got == ex
        print("gap to exact, M = 12..16, %d cases, %d starts: optimum found in %d, mean gap %.3f %%, max %.3f %%"
              % (len(gaps), n_starts, hit, 100 * np.mean(gaps), 100 * np.max(gaps)))
    ctx.close()


if __name__ == "__main__":
    main()
