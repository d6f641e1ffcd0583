#!/usr/bin/env python3
"""EkfSlam.localize() / run_localize() -- pose-only steps on a frozen map, two launches per step, never a covariance pass --
timed beside step() / stream_run() on the same build and the same dense starting state, at four settings:
  1. 32 x N = 2000, m = 8;
  2. N = 2000 x 1, m = 8;
  3. N = 8000 x 1, m = 8;
  4. 256 x N = 20, m = 8 (small-state path).
Every state index is active ("active_bound" 0).  A setting's start: a block-diagonal state, the first `--warm` steps of a
synthetic stream as SLAM steps, flush().  Then `--steps` further steps of that stream, per mode: (a) host clock around the
enqueue of all of them, (b) host clock including the final sync(), (c) device time (the handle's event pair around them), each
divided by the number of steps.  The localisation modes run first: they leave the map, and nothing pending, so the SLAM modes
behind them start from the same map; the covariance passes step() and stream_run() cause -- one per 40 observations, and the
flush() that ends the measurement -- are charged to them.  For localize() also the two kernels alone (event pairs: option
"profile_kernels", classes 9 and 10 of profile_read_class).  Medians over `--reps` repetitions, with the spread (min .. max).
The parity figures the tests print (tests/test_localize_cpu.py, tests/test_gpu_localize.py, run with -s) are kept at the end of
the file: `--keep` names the file whose lines from "Parity" on are carried over.
  python3 tools/localize_time.py [--steps 40] [--reps 5] [--out profiles/localize.txt]
Nothing is checked here, only timed."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(xs):
    xs = np.asarray(xs)
    return f"{np.median(xs):9.1f} ({np.min(xs):.1f} .. {np.max(xs):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localize.txt"))
    ap.add_argument("--keep", default=None)
    ap.add_argument("--only", type=int, default=0, help="one setting (1..4) only")
    args = ap.parse_args()
    import slam_duckietown_amd as sd
    import slam_duckietown_amd.synthetic as syn
    K, W = args.steps, args.warm
    lines = ["EkfSlam.localize() / run_localize() beside step() / stream_run(): microseconds per step for the whole bank, median (min .. max)",
             f"(tools/localize_time.py; {K} steps per repetition behind {W} SLAM steps and a flush, {args.reps} repetitions, m = 8, every index active)",
             ""]

    def setting(title, N, B):
        m = 8
        streams = [syn.synthetic_stream(N, W + K, m, t) for t in range(B)]
        stack = lambda i: np.stack([s[i] for s in streams], 1)
        with sd.EkfSlam(3 + 2 * N, batch=B) as f:
            f.set_option("active_bound", 0)
            for b, s in enumerate(streams):
                f.set_state_diag(s[0], s[1], b)
            f.stream_upload(stack(2), stack(3), stack(4), stack(5), stack(6))
            f.stream_run(0, W)
            f.flush()
            f.sync()
            step_args = [(stack(2)[k], stack(3)[k], stack(4)[k], stack(5)[k], stack(6)[k]) for k in range(W, W + K)]

            def loc_calls():
                for a in step_args:
                    f.localize(*a)

            def slam_calls():
                for a in step_args:
                    f.step(*a)
                f.flush()

            def slam_run():
                f.stream_run(W, K)
                f.flush()

            modes = [("localize()", loc_calls), ("run_localize()", lambda: f.run_localize(W, K)), ("step()", slam_calls),
                     ("stream_run()", slam_run)]
            rows, dev = [title], {}
            for name, fn in modes:
                fn()                                         # warm-up (allocations on first use)
                f.sync()
                ta, tb, tc = [], [], []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    fn()
                    ta.append((time.perf_counter() - t0) * 1e6 / K)
                    f.sync()
                    tb.append((time.perf_counter() - t0) * 1e6 / K)
                for _ in range(args.reps):
                    f.timer_begin()
                    fn()
                    tc.append(f.timer_end() * 1e3 / K)
                dev[name] = float(np.median(tc))
                rows += [f"    {name:<16}(a) enqueue      {med(ta)}", f"    {'':<16}(b) with sync    {med(tb)}",
                         f"    {'':<16}(c) device       {med(tc)}"]
            f.set_option("profile_kernels", 1)
            ks, kr = [], []
            for _ in range(args.reps):
                f.profile_enable(True)
                for a in step_args[:10]:
                    f.localize(*a)
                (ms9, n9), (ms10, n10) = f.profile_read_class(9), f.profile_read_class(10)
                f.profile_read()
                ks.append(ms9 * 1e3 / max(n9, 1))
                kr.append(ms10 * 1e3 / max(n10, 1))
            f.profile_enable(False)
            rows += [f"    k_loc_solve alone                {med(ks)}", f"    k_loc_rows alone                 {med(kr)}",
                     f"    device time per step: localize() / step() = {dev['localize()'] / dev['step()']:.2f}, run_localize() / stream_run() = "
                     f"{dev['run_localize()'] / dev['stream_run()']:.2f}"]
            for r in rows:
                print(r, flush=True)
            lines.extend(rows + [""])

    todo = [("32 x N = 2000", 2000, 32), ("N = 2000 x 1", 2000, 1), ("N = 8000 x 1", 8000, 1), ("256 x N = 20 (small-state path)", 20, 256)]
    for i, t in enumerate(todo):
        if args.only in (0, i + 1):
            setting(*t)
    kept = []
    if args.keep and os.path.exists(args.keep):
        old = open(args.keep).read().splitlines()
        at = next((i for i, ln in enumerate(old) if ln.startswith("Parity")), None)
        kept = old[at:] if at is not None else []
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines + kept) + "\n")


if __name__ == "__main__":
    main()
