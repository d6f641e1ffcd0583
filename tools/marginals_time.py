#!/usr/bin/env python3
"""Pose / landmark marginals of a whole bank with a full cadence pending (80 ranks): two routes, timed.
  (a) EkfSlam.marginals() for the whole bank (one read-only kernel, no covariance pass, no mirror);
  (b) evaluation.pose_nees through covariance_block (a flush, then a mirror pass and a copy per trajectory).
Every repetition re-steps the bank (5 steps of m = 8 after a flush: 80 ranks pending), synchronises, then times (a) and
(b) -- in that order: (a) changes nothing, (b) flushes.  Device time from HIP events on the handle's stream (ekf_timer_*),
host time from a clock around the call and a synchronisation.  The active bound is off, so that the ranks cover every
state index (the most a query reads).  `--kernel-only K` instead calls marginals() K times after one warm-up (for a
kernel trace: rocprofv3 --kernel-trace --stats -- python3 tools/marginals_time.py --kernel-only 50).
  python3 tools/marginals_time.py [--landmarks 2000] [--trajectories 32] [--reps 10] [--warmup 3]
Nothing is checked here, only timed."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--landmarks", type=int, default=2000)
    ap.add_argument("--trajectories", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-only", type=int, default=0)
    args = ap.parse_args()
    import slam_duckietown_amd as sd
    import slam_duckietown_amd.evaluation as ev
    import slam_duckietown_amd.synthetic as syn
    N, B, m, cad = args.landmarks, args.trajectories, 8, 5
    n = 3 + 2 * N
    total = args.warmup + max(args.reps, 1)
    streams = [syn.synthetic_stream(N, cad * total, m, t) for t in range(B)]
    truth = np.zeros((B, 3))
    with sd.EkfSlam(n, batch=B) as f:
        f.set_option("active_bound", 0)
        for b, s in enumerate(streams):
            f.set_state_diag(s[0], s[1], b)

        def cadence(r):
            f.flush()
            for k in range(cad * r, cad * (r + 1)):
                f.step(np.array([s[2][k] for s in streams]), np.array([s[3][k] for s in streams]),
                       np.stack([s[4][k] for s in streams]), np.stack([s[5][k] for s in streams]),
                       np.stack([s[6][k] for s in streams]))
            f.sync()

        def timed(fn):
            f.sync()
            t0 = time.perf_counter()
            f.timer_begin()
            fn()
            dev = f.timer_end()
            f.sync()
            return dev, (time.perf_counter() - t0) * 1e3

        if args.kernel_only:
            cadence(0)
            f.marginals()
            for _ in range(args.kernel_only):
                f.marginals()
            print(f"marginals() x {args.kernel_only} at {B} x N = {N}, 80 ranks pending")
            return
        ra, rb, rc = [], [], []
        for r in range(total):
            cadence(r)
            a = timed(lambda: f.marginals())
            c = timed(lambda: ev.marginal_nees(f, truth))
            b = timed(lambda: ev.pose_nees(f, truth))
            if r >= args.warmup:
                ra.append(a)
                rc.append(c)
                rb.append(b)
        kb = 80
        bytes_read = B * (2 * kb * n * 8 + 3 * N * 8) + B * (9 + 4 * N) * 8
        print(f"{B} x N = {N}, {kb} ranks pending, {len(ra)} repetitions after {args.warmup} warm-up "
              f"(median; device events / host clock, ms)")
        for name, rs in (("(a)  marginals(), whole bank", ra), ("(a') evaluation.marginal_nees", rc),
                         ("(b)  evaluation.pose_nees via covariance_block", rb)):
            d, h = np.median([x[0] for x in rs]), np.median([x[1] for x in rs])
            print(f"  {name:48s} device {d:8.3f}  host {h:8.3f}")
        print(f"  speed-up (b) / (a), host clock: {np.median([x[1] for x in rb]) / np.median([x[1] for x in ra]):.1f} x")
        print(f"  bytes the kernel moves (V, W at every index, P_base blocks, results): {bytes_read / 1e6:.1f} MB")


if __name__ == "__main__":
    main()
