#!/usr/bin/env python3
"""EkfSlam.localize_detections() -- one window of raw detections per trajectory against a frozen map: k_loc_associate, then the two
launches of localize(), no host round trip -- timed per window at three settings, 8 tags x 3 frames per trajectory:
  1. 32 x N = 2000;
  2. N = 2000 x 1;
  3. 256 x N = 20 (small-state handle).
A setting's start: a block-diagonal state, the first `--warm` steps of a synthetic stream as SLAM steps (dense cross terms),
flush(), a tag table over the landmarks (the first 1000 where the map has more: tag ids end at 1024).  Every state index is active
("active_bound" 0).  The window shows the eight landmarks nearest to each trajectory's pose, as the mean itself sees them.  Modes:
  localize_detections()   the call;
  k_loc_associate alone   its event pair (option "profile_kernels", class 11 of profile_read_class), device time;
  host route              what the call replaces: per trajectory tag_index() + mean() + frontend.associate_known, then localize();
  step_detections()       the mapping call on the same window (it moves the map: run last; its passes are charged to it).
Per mode: (a) host clock around the enqueue of `--steps` calls, (b) including the final sync(), (c) device time (the handle's
event pair), each divided by the number of calls.  Medians over `--reps` repetitions, with the spread (min .. max).
  python3 tools/localize_detections_time.py [--steps 20] [--reps 5] [--out profiles/localize_detections.txt]
Nothing is checked here, only timed."""
import argparse
import os
import sys
import time
from types import SimpleNamespace as NS

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(xs):
    xs = np.asarray(xs)
    return f"{np.median(xs):9.1f} ({np.min(xs):.1f} .. {np.max(xs):.1f})"


def window(mean, tags_known, frames=3, tags=8):
    """The `tags` landmarks (of the first `tags_known`) nearest to the pose, in `frames` frames, as the mean sees them."""
    d = mean[3:3 + 2 * tags_known].reshape(-1, 2) - mean[:2]
    near = np.argsort(np.hypot(d[:, 0], d[:, 1]))[:tags]
    c, s = np.cos(mean[2]), np.sin(mean[2])
    out = []
    for fr in range(frames):
        out.append((float(fr), [NS(tag_id=int(j), pose_R=np.eye(3), pose_err=1e-3,
                                   pose_t=np.array([[-(-s * d[j, 0] + c * d[j, 1])], [0.0], [c * d[j, 0] + s * d[j, 1]]]))
                                for j in near]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localize_detections.txt"))
    ap.add_argument("--only", type=int, default=0, help="one setting (1..3) only")
    args = ap.parse_args()
    import slam_duckietown_amd as sd
    import slam_duckietown_amd.synthetic as syn
    from slam_duckietown_amd import frontend
    K, W = args.steps, args.warm
    lines = ["EkfSlam.localize_detections(): microseconds per window for the whole bank, median (min .. max)",
             f"(tools/localize_detections_time.py; {K} calls per repetition behind {W} SLAM steps and a flush, {args.reps} repetitions, "
             "8 tags x 3 frames per trajectory, every index active)", ""]

    def setting(title, N, B):
        streams = [syn.synthetic_stream(N, W, 8, t) for t in range(B)]
        stack = lambda i: np.stack([s[i] for s in streams], 1)
        known = min(N, 1000)
        with sd.EkfSlam(3 + 2 * N, batch=B) as f:
            f.set_option("active_bound", 0)
            for b, s in enumerate(streams):
                f.set_state_diag(s[0], s[1], b)
                f.set_tag_index({j: j for j in range(known)}, b)
            f.stream_upload(stack(2), stack(3), stack(4), stack(5), stack(6))
            f.stream_run(0, W)
            f.flush()
            f.sync()
            wins = [window(f.mean(b), known) for b in range(B)]
            lin, ang = 0.004, 0.02

            def call():
                for _ in range(K):
                    f.localize_detections(lin, ang, wins if B > 1 else wins[0])

            def host_route():
                for _ in range(K):
                    tags = [frontend.associate_known(wins[b], f.tag_index(b), f.mean(b)[:3])[0] for b in range(B)]
                    idx = [list(t) for t in tags]
                    zr = [[t[k][4] for k in ks] for t, ks in zip(tags, idx)]
                    zb = [[t[k][5] for k in ks] for t, ks in zip(tags, idx)]
                    f.localize(lin, ang, idx, zr, zb)

            def mapping():
                for _ in range(K):
                    f.step_detections(lin, ang, wins if B > 1 else wins[0])
                f.flush()

            rows = [title]
            for name, fn in (("localize_detections()", call), ("host route", host_route), ("step_detections()", mapping)):
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
                rows += [f"    {name:<22}(a) enqueue      {med(ta)}", f"    {'':<22}(b) with sync    {med(tb)}",
                         f"    {'':<22}(c) device       {med(tc)}"]
                if name == "localize_detections()":
                    f.set_option("profile_kernels", 1)
                    ka = []
                    for _ in range(args.reps):
                        f.profile_enable(True)
                        for _ in range(10):
                            f.localize_detections(lin, ang, wins if B > 1 else wins[0])
                        ms, n = f.profile_read_class(11)
                        f.profile_read()
                        ka.append(ms * 1e3 / max(n, 1))
                    f.profile_enable(False)
                    f.set_option("profile_kernels", 0)
                    rows.append(f"    k_loc_associate alone  (c) device       {med(ka)}")
            for r in rows:
                print(r, flush=True)
            lines.extend(rows + [""])

    todo = [("32 x N = 2000", 2000, 32), ("N = 2000 x 1", 2000, 1), ("256 x N = 20 (small-state handle)", 20, 256)]
    for i, t in enumerate(todo):
        if args.only in (0, i + 1):
            setting(*t)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
