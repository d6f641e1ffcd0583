#!/usr/bin/env python3
"""Cost of the pose log (EkfSlam.log_poses): ms per step with the log off and on, in alternated runs of one process, for
four shapes:
  headline   32 x N = 2000, m = 8, run_stream (packed cadences: the solve workgroups write the rows)
  chained    N = 2000 x 1, m = 8, run_stream (chained solves: the serial chain of solves is where a store would show)
  unchained  the same with chain = 0: the plain solve skips the last landmark's down-date, the logging one does it
  small      N = 20 x 1, m = 8, one step() per call (the small-state path: the row is written by the step's own launch)
and what the log replaces: the same 200-step stream as one-step pieces with mean() and covariance_block(0, 0, 3, 3) after
each (the only way to a trajectory without the log) against run_stream with the log on plus one poses() call (host time).
Each leg keeps two handles (log off, log on), resets both to the same start before every run, and times the runs in the
order off, on, on, off, ... (device time from HIP events on the handle's stream for the streams; host time around the calls
and a synchronisation for step()).  Writes the table to profiles/pose_log.txt (or --out).  Nothing is checked here.
  python3 tools/pose_log_time.py [--reps 6] [--out profiles/pose_log.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stream_leg(sd, syn, N, B, steps, reps, opts=()):
    streams = [syn.synthetic_stream(N, steps, 8, t) for t in range(B)]
    args = tuple(np.stack([s[i] for s in streams], axis=1) for i in (2, 3, 4, 5, 6))
    handles = {}
    for log in (0, 1):
        f = sd.EkfSlam(3 + 2 * N, batch=B)
        for name, v in opts:
            f.set_option(name, v)
        if log:
            f.log_poses(steps)
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
            f.log_poses(steps)
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


def replaces_leg(sd, syn, N, B, steps, reps):
    """Host ms for the whole trajectory: one-step pieces with two blocking downloads each / run_stream + one poses()."""
    streams = [syn.synthetic_stream(N, steps, 8, t) for t in range(B)]
    args = tuple(np.stack([s[i] for s in streams], axis=1) for i in (2, 3, 4, 5, 6))
    f = sd.EkfSlam(3 + 2 * N, batch=B)

    def reset():
        for b, s in enumerate(streams):
            f.set_state_diag(s[0], s[1], b)
        f.sync()

    reset()
    f.stream_upload(*args)

    def pieces():
        f.log_poses(0)
        reset()
        t0 = time.perf_counter()
        for k in range(steps):
            f.stream_run(k, 1)
            for b in range(B):
                f.mean(b)
                f.covariance_block(0, 0, 3, 3, b)
        return (time.perf_counter() - t0) * 1e3

    def traced():
        f.log_poses(steps)
        reset()
        t0 = time.perf_counter()
        f.stream_run(0, steps)
        f.poses()
        return (time.perf_counter() - t0) * 1e3

    pieces(), traced()
    times = {0: [], 1: []}
    for r in range(reps):
        for which in ((0, 1) if r % 2 == 0 else (1, 0)):
            times[which].append(pieces() if which == 0 else traced())
    f.close()
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_log.txt"))
    args = ap.parse_args()
    import slam_duckietown_amd as sd
    import slam_duckietown_amd.synthetic as syn
    legs = [("headline", "32 x N = 2000, run_stream, 200 steps", lambda: stream_leg(sd, syn, 2000, 32, 200, args.reps)),
            ("chained", "N = 2000 x 1, run_stream, 400 steps", lambda: stream_leg(sd, syn, 2000, 1, 400, args.reps)),
            ("unchained", "N = 2000 x 1, run_stream, chain = 0",
             lambda: stream_leg(sd, syn, 2000, 1, 400, args.reps, (("chain", 0),))),
            ("small", "N = 20 x 1, step() per call, 500 steps", lambda: small_leg(sd, syn, args.reps))]
    lines = ["# tools/pose_log_time.py: ms per step with the pose log off / on, alternated runs in one process",
             f"# (median of {args.reps} runs each; m = 8)",
             f"{'shape':10s} {'workload':42s} {'off ms':>9s} {'on ms':>9s} {'cost %':>7s}"]
    for key, desc, fn in legs:
        t = fn()
        off, on = float(np.median(t[0])), float(np.median(t[1]))
        cost = 100.0 * (on - off) / off
        lines.append(f"{key:10s} {desc:42s} {off:9.4f} {on:9.4f} {cost:7.2f}")
        lines.append(f"#   off runs: {' '.join(f'{x:.4f}' for x in t[0])}")
        lines.append(f"#   on runs:  {' '.join(f'{x:.4f}' for x in t[1])}")
        print(lines[-3], flush=True)
    lines.append("# what the log replaces: host ms for a 200-step trajectory with its covariance, one-step pieces + mean() +")
    lines.append("# covariance_block(0, 0, 3, 3) per step and trajectory / run_stream with the log on + one poses() call")
    lines.append(f"{'shape':10s} {'workload':42s} {'pieces ms':>9s} {'trace ms':>9s} {'ratio':>7s}")
    for key, desc, N, B in (("headline", "32 x N = 2000, 200 steps", 2000, 32), ("chained", "N = 2000 x 1, 200 steps", 2000, 1)):
        t = replaces_leg(sd, syn, N, B, 200, max(2, args.reps // 2))
        a, b = float(np.median(t[0])), float(np.median(t[1]))
        lines.append(f"{key:10s} {desc:42s} {a:9.2f} {b:9.2f} {a / b:7.1f}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
