#!/usr/bin/env python3
"""Cost of the NIS gate (EkfSlam.set_nis_gate): ms per step with the gate off and on -- at the chi2_2 99 % quantile, which
none of these streams' updates reaches (the rejection counts are printed) -- in alternated runs of one process, for three
shapes:
  chained    N = 2000 x 1, m = 8, run_stream (chained solves: the gate's test sits in the serial chain of landmark updates)
  headline   32 x N = 2000, m = 8, run_stream (packed cadences)
  small      N = 20 x 256, m = 8, run_stream (a small-state bank: the gate runs in the log instantiations of its kernels)
Each leg keeps two handles (gate off, gate on), resets both to the same start before every run, and times the runs in the
order off, on, on, off, ... (device time from HIP events on the handle's stream).  Writes the table to profiles/nis_gate.txt
(or --out).  Nothing is checked here.
  python3 tools/nis_gate_time.py [--reps 6] [--out profiles/nis_gate.txt]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GATE = 9.21034037197618           # -2 ln(1 - 0.99)


def stream_leg(sd, syn, N, B, steps, reps):
    streams = [syn.synthetic_stream(N, steps, 8, t) for t in range(B)]
    args = tuple(np.stack([s[i] for s in streams], axis=1) for i in (2, 3, 4, 5, 6))
    handles = {}
    for gate in (0, 1):
        f = sd.EkfSlam(3 + 2 * N, batch=B)
        if gate:
            f.set_nis_gate(GATE)
        for b, s in enumerate(streams):
            f.set_state_diag(s[0], s[1], b)
        f.stream_upload(*args)
        handles[gate] = f

    def run(gate):
        f = handles[gate]
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
        for gate in ((0, 1) if r % 2 == 0 else (1, 0)):
            times[gate].append(run(gate))
    rejected = int(handles[1].gate_counts().sum())
    for f in handles.values():
        f.close()
    return times, rejected


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nis_gate.txt"))
    args = ap.parse_args()
    import slam_duckietown_amd as sd
    import slam_duckietown_amd.synthetic as syn
    legs = [("chained", "N = 2000 x 1, run_stream, 400 steps", lambda: stream_leg(sd, syn, 2000, 1, 400, args.reps)),
            ("headline", "32 x N = 2000, run_stream, 200 steps", lambda: stream_leg(sd, syn, 2000, 32, 200, args.reps)),
            ("small", "N = 20 x 256, run_stream, 400 steps", lambda: stream_leg(sd, syn, 20, 256, 400, args.reps))]
    lines = ["# tools/nis_gate_time.py: ms per step with the NIS gate off / on (threshold 9.21, the chi2_2 99 % quantile),",
             f"# alternated runs in one process (median of {args.reps} runs each; m = 8; 'rejected': updates the gate rejected)",
             f"{'shape':10s} {'workload':42s} {'off ms':>9s} {'on ms':>9s} {'cost %':>7s} {'rejected':>8s}"]
    for key, desc, fn in legs:
        t, rejected = fn()
        off, on = float(np.median(t[0])), float(np.median(t[1]))
        cost = 100.0 * (on - off) / off
        lines.append(f"{key:10s} {desc:42s} {off:9.4f} {on:9.4f} {cost:7.2f} {rejected:8d}")
        lines.append(f"#   off runs: {' '.join(f'{x:.4f}' for x in t[0])}")
        lines.append(f"#   on runs:  {' '.join(f'{x:.4f}' for x in t[1])}")
        print(lines[-3], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
