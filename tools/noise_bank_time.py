#!/usr/bin/env python3
"""Cost of the per-trajectory noise table (EkfSlam.set_noise): ms per step with the table off (the handle's constants) and on
(a distinct row per trajectory, drawn around the handle's constants), in alternated runs of one process, for three shapes:
  chained    N = 2000 x 1, m = 8, run_stream (chained solves: the row is loaded once per cadence solve)
  headline   32 x N = 2000, m = 8, run_stream (packed cadences)
  small      N = 20 x 256, m = 8, run_stream (a small-state bank: the table runs in the log instantiations of its kernels)
Each leg keeps two handles (table off, table on), resets both to the same start before every run, and times the runs in the
order off, on, on, off, ... (device time from HIP events on the handle's stream).  Then one evaluation.tune_noise call on a
16 x 16 grid (256 trajectories, one bank) at N = 12, 500 steps, timed end to end on the host (upload, run, log download,
statistics).  Writes the table to profiles/noise_bank.txt (or --out).  Nothing is checked here.
  python3 tools/noise_bank_time.py [--reps 6] [--out profiles/noise_bank.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stream_leg(sd, syn, N, B, steps, reps):
    streams = [syn.synthetic_stream(N, steps, 8, t) for t in range(B)]
    args = tuple(np.stack([s[i] for s in streams], axis=1) for i in (2, 3, 4, 5, 6))
    rng = np.random.default_rng(7)
    cfg = sd.EkfConfig()
    ms = cfg.motion_sigma * rng.uniform(0.5, 2.0, B)
    qs = cfg.meas_sigma * rng.uniform(0.5, 2.0, B)
    handles = {}
    for on in (0, 1):
        f = sd.EkfSlam(3 + 2 * N, batch=B)
        if on:
            f.set_noise(ms, qs)
        for b, s in enumerate(streams):
            f.set_state_diag(s[0], s[1], b)
        f.stream_upload(*args)
        handles[on] = f

    def run(on):
        f = handles[on]
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
        for on in ((0, 1) if r % 2 == 0 else (1, 0)):
            times[on].append(run(on))
    for f in handles.values():
        f.close()
    return times


def tune_leg(syn, reps):
    import slam_duckietown_amd.evaluation as ev
    N, steps = 12, 500
    s = syn.synthetic_stream(N, steps, 4, 0)
    grid_m = np.geomspace(0.02, 0.5, 16)
    grid_q = np.geomspace(0.1, 2.0, 16)
    out = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        res = ev.tune_noise(tuple(np.asarray(s[i]) for i in (2, 3, 4, 5, 6)), grid_m, grid_q, s[0], s[1])
        out.append(1e3 * (time.perf_counter() - t0))
    return out[1:], res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise_bank.txt"))
    args = ap.parse_args()
    import slam_duckietown_amd as sd
    import slam_duckietown_amd.synthetic as syn
    legs = [("chained", "N = 2000 x 1, run_stream, 400 steps", lambda: stream_leg(sd, syn, 2000, 1, 400, args.reps)),
            ("headline", "32 x N = 2000, run_stream, 200 steps", lambda: stream_leg(sd, syn, 2000, 32, 200, args.reps)),
            ("small", "N = 20 x 256, run_stream, 400 steps", lambda: stream_leg(sd, syn, 20, 256, 400, args.reps))]
    lines = ["# tools/noise_bank_time.py: ms per step with the noise table off / on (a distinct row per trajectory),",
             f"# alternated runs in one process (median of {args.reps} runs each; m = 8)",
             f"{'shape':10s} {'workload':42s} {'off ms':>9s} {'on ms':>9s} {'cost %':>7s}"]
    for key, desc, fn in legs:
        t = fn()
        off, on = float(np.median(t[0])), float(np.median(t[1]))
        cost = 100.0 * (on - off) / off
        lines.append(f"{key:10s} {desc:42s} {off:9.4f} {on:9.4f} {cost:7.2f}")
        lines.append(f"#   off runs: {' '.join(f'{x:.4f}' for x in t[0])}")
        lines.append(f"#   on runs:  {' '.join(f'{x:.4f}' for x in t[1])}")
        print(lines[-3], flush=True)
    t, res = tune_leg(syn, max(2, args.reps // 2))
    lines.append(f"tune_noise 16 x 16 grid, N = 12, 500 steps, m = 4 (bank sizes {res.bank_sizes}): "
                 f"{float(np.median(t)):.1f} ms per call (host wall time; runs {' '.join(f'{x:.1f}' for x in t)}); "
                 f"best pair {res.best[0]:.4g}, {res.best[1]:.4g}")
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
