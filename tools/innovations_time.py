#!/usr/bin/env python3
"""Cost of the innovation log (EkfSlam.log_innovations): ms per step with the log off and on, in alternated runs of one
process, for three shapes:
  headline   32 x N = 2000, m = 8, run_stream (packed cadences: one copy launch per cadence)
  chained    N = 2000 x 1, m = 8, run_stream (chained solves: the copy launch sits in the serial chain of solves)
  small      N = 20 x 1, m = 8, one step() per call (the small-state path: the log is written by the step's own launch)
Each leg keeps two handles (log off, log on), resets both to the same start before every run, and times the runs in the
order off, on, on, off, ... (device time from HIP events on the handle's stream for the streams; host time around the calls
and a synchronisation for step()).  Writes the table to profiles/innovations.txt (or --out).  Nothing is checked here.
  python3 tools/innovations_time.py [--reps 6] [--out profiles/innovations.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BUDGET = {"headline": 2.0, "chained": 10.0, "small": 5.0}


def stream_leg(sd, syn, N, B, steps, reps):
    streams = [syn.synthetic_stream(N, steps, 8, t) for t in range(B)]
    args = tuple(np.stack([s[i] for s in streams], axis=1) for i in (2, 3, 4, 5, 6))
    handles = {}
    for log in (0, 1):
        f = sd.EkfSlam(3 + 2 * N, batch=B)
        if log:
            f.log_innovations(steps)
        for b, s in enumerate(streams):
            f.set_state_diag(s[0], s[1], b)
        f.stream_upload(*args)
        handles[log] = f

    def run(log):
        f = handles[log]
        for b, s in enumerate(streams):
            f.set_state_diag(s[0], s[1], b)
        f.sync()
        f.timer_begin()
        f.stream_run(0, steps)
        f.flush()
        return f.timer_end() / steps

    run(0), run(1)                                         # warm-up (first launches, allocations on first use)
    times = {0: [], 1: []}
    for r in range(reps):
        for log in ((0, 1) if r % 2 == 0 else (1, 0)):
            times[log].append(run(log))
    for f in handles.values():
        f.close()
    return times


def small_leg(sd, syn, reps, steps=500):
    N = 20
    s = syn.synthetic_stream(N, steps, 8, 0)
    handles = {}
    for log in (0, 1):
        f = sd.EkfSlam(3 + 2 * N)
        if log:
            f.log_innovations(steps)
        handles[log] = f

    def run(log):
        f = handles[log]
        f.set_state_diag(s[0], s[1])
        f.sync()
        t0 = time.perf_counter()
        for k in range(steps):
            f.step(s[2][k], s[3][k], s[4][k], s[5][k], s[6][k])
        f.sync()
        return (time.perf_counter() - t0) * 1e3 / steps

    run(0), run(1)
    times = {0: [], 1: []}
    for r in range(reps):
        for log in ((0, 1) if r % 2 == 0 else (1, 0)):
            times[log].append(run(log))
    for f in handles.values():
        f.close()
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "innovations.txt"))
    args = ap.parse_args()
    import slam_duckietown_amd as sd
    import slam_duckietown_amd.synthetic as syn
    legs = [("headline", "32 x N = 2000, run_stream, 200 steps", lambda: stream_leg(sd, syn, 2000, 32, 200, args.reps)),
            ("chained", "N = 2000 x 1, run_stream, 400 steps", lambda: stream_leg(sd, syn, 2000, 1, 400, args.reps)),
            ("small", "N = 20 x 1, step() per call, 500 steps", lambda: small_leg(sd, syn, args.reps))]
    lines = ["# tools/innovations_time.py: ms per step with the innovation log off / on, alternated runs in one process",
             f"# (median of {args.reps} runs each; m = 8; budget: the issue's estimate of what the log may cost)",
             f"{'shape':10s} {'workload':42s} {'off ms':>9s} {'on ms':>9s} {'cost %':>7s} {'budget %':>8s}  verdict"]
    for key, desc, fn in legs:
        t = fn()
        off, on = float(np.median(t[0])), float(np.median(t[1]))
        cost = 100.0 * (on - off) / off
        verdict = "met" if cost <= BUDGET[key] else f"missed by {cost - BUDGET[key]:.2f} points"
        lines.append(f"{key:10s} {desc:42s} {off:9.4f} {on:9.4f} {cost:7.2f} {BUDGET[key]:8.1f}  {verdict}")
        lines.append(f"#   off runs: {' '.join(f'{x:.4f}' for x in t[0])}")
        lines.append(f"#   on runs:  {' '.join(f'{x:.4f}' for x in t[1])}")
        print(lines[-3], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
