#!/usr/bin/env python3
"""A hypothesis bank driven by raw detections -- HypothesisBank.step_detections / upload_detections / run on a detection stream --
against the host route it replaces (frontend.associate_known per window, then `step` / `upload_stream`), at N = 2000, windows of
8 tags x 3 frames, 200 windows, for K = 32, 1024 and 4096 hypotheses seeded around the map's pose.  Host-clocked from the first
call to the end of the bank's sync, medians over `--reps` repetitions with the spread (min .. max); every repetition starts from
the same reset bank.
  association on the device   200 step_detections calls and one sync less 200 `step` calls with the lists the device reported
                              and one sync, per window: what the window's upload (9 KB) and k_hyp_associate add to a step.  The bank
                              has no profile brackets, so this is a DIFFERENCE of two back-to-back runs, not an event pair; it is
                              device time where the steps keep the device busy (K >= 1024).
  one window, call + sync     step_detections + sync against associate_known + step + sync.
  upload, 200 windows         upload_detections (blocking) against 200 x associate_known + upload_stream (blocking), milliseconds.
  run, per step               run(0, 200) + sync on the detection stream against the index stream of the reported lists, without
                              resampling and with fraction 0.5, split 0.5.
  python3 tools/hyp_detections_time.py [--reps 5] [--out profiles/hyp_detections.txt]
Nothing is checked here, only timed."""
import argparse
import os
import sys
import time
from types import SimpleNamespace as NS

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, TAGS, FRAMES, STEPS, COUNTS, FRACTION, SPLIT = 2000, 8, 3, 200, (32, 1024, 4096), 0.5, 0.5
TAGGED = 1000                                              # landmarks 0 .. 999 carry tag ids (the device's table ends at 1024)
GATE = 1e3                                                 # the synthetic world is larger than the reference's 1.5 m gate
LIN, ANG = 0.004, 0.02
SEED_COV = np.diag([0.02, 0.02, 0.005])


def med(xs, per=1.0):
    xs = np.asarray(xs) / per
    return f"{np.median(xs):9.1f} ({np.min(xs):.1f} .. {np.max(xs):.1f})"


def clock(bank, reset, work, reps):
    """Microseconds of `work()` + sync behind a reset bank, per repetition (the first one warms up and is dropped)."""
    ts = []
    for _ in range(reps + 1):
        reset()
        bank.sync()
        t0 = time.perf_counter()
        work()
        bank.sync()
        ts.append((time.perf_counter() - t0) * 1e6)
    return ts[1:]


def windows(mean, rng):
    """200 windows of 8 tagged landmarks x 3 frames as the map's pose sees them (camera frame: x = -y_robot, z = x_robot)."""
    out = []
    for _ in range(STEPS):
        lms = rng.choice(TAGGED, TAGS, replace=False)
        d = mean[3:].reshape(-1, 2)[lms] - mean[:2]
        r, b = np.hypot(d[:, 0], d[:, 1]), np.arctan2(d[:, 1], d[:, 0]) - mean[2]
        win = []
        for fr in range(FRAMES):
            rr, bb = r + rng.normal(0.0, 0.01, TAGS), b + rng.normal(0.0, 0.005, TAGS)
            win.append((float(fr), [NS(tag_id=int(j), pose_R=np.eye(3), pose_t=np.array([[-rr[i] * np.sin(bb[i])], [0.0], [rr[i] * np.cos(bb[i])]]),
                                       pose_err=1e-3) for i, j in enumerate(lms)]))
        out.append(win)
    return out


def run(args):
    import slam_duckietown_amd as sd
    import slam_duckietown_amd.synthetic as syn
    from slam_duckietown_amd import frontend
    n, W, reps = 3 + 2 * N, args.warm, args.reps
    lines = ["A hypothesis bank driven by raw detections against the host route: microseconds, median (min .. max)",
             f"(tools/hyp_detections_time.py; N = {N}, windows of {TAGS} tags x {FRAMES} frames, {STEPS} windows, {reps} repetitions behind "
             f"{W} SLAM steps and a flush; fraction {FRACTION}, split {SPLIT} where a run resamples)", ""]
    s = syn.synthetic_stream(N, W, 8, 0)
    rng = np.random.default_rng(1)
    index = {j: j for j in range(TAGGED)}
    with sd.EkfSlam(n, batch=1) as f:
        f.set_option("active_bound", 0)
        f.set_state_diag(s[0], s[1])
        f.stream_upload(*(np.asarray(s[i])[:, None] for i in (2, 3, 4, 5, 6)))
        f.stream_run(0, W)
        f.flush()
        f.set_tag_index(index)
        f.set_association(GATE, ())
        f.sync()
        mean = f.mean(0)
        wins = windows(mean, rng)
        lin, ang = [LIN] * STEPS, [ANG] * STEPS
        for K in COUNTS:
            seeds = mean[:3] + rng.multivariate_normal(np.zeros(3), 4.0 * SEED_COV, K)
            u, z = rng.random(STEPS), rng.standard_normal((STEPS, K, 3))
            rows = [f"K = {K}"]
            with f.hypotheses(K) as bank:
                def reset():
                    bank.reset(seeds, SEED_COV)

                def host_lists(win):
                    tags, _ = frontend.associate_known(win, index, np.zeros(3), GATE, (), n_landmarks=N)
                    idx = list(tags)
                    return idx, [tags[k][4] for k in idx], [tags[k][5] for k in idx]

                bank.upload_detections(lin, ang, wins)
                lists = [bank.tags(step=k) for k in range(STEPS)]
                dev = [(list(t), [t[k][2] for k in t], [t[k][3] for k in t]) for t in lists]
                assert all(len(t) == TAGS for t in lists), "a window did not match its 8 tags"

                def dets():
                    for k in range(STEPS):
                        bank.step_detections(LIN, ANG, wins[k])

                def steps():
                    for k in range(STEPS):
                        bank.step(LIN, ANG, *dev[k])

                def one_device():
                    for k in range(STEPS):
                        bank.step_detections(LIN, ANG, wins[k])
                        bank.sync()

                def one_host():
                    for k in range(STEPS):
                        bank.step(LIN, ANG, *host_lists(wins[k]))
                        bank.sync()

                td, ts = clock(bank, reset, dets, reps), clock(bank, reset, steps, reps)
                rows += [f"    {'200 step_detections, one sync, per window':<56}{med(td, STEPS)}",
                         f"    {'200 step (reported lists), one sync, per window':<56}{med(ts, STEPS)}   association on the device: "
                         f"{(np.median(td) - np.median(ts)) / STEPS:+.1f} per window"]
                t1, t2 = clock(bank, reset, one_device, reps), clock(bank, reset, one_host, reps)
                rows += [f"    {'one window: step_detections + sync':<56}{med(t1, STEPS)}",
                         f"    {'one window: associate_known + step + sync':<56}{med(t2, STEPS)}   host / device {np.median(t2) / np.median(t1):.2f}"]
                ta = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    for k in range(STEPS):
                        host_lists(wins[k])
                    ta.append((time.perf_counter() - t0) * 1e6)
                rows.append(f"    {'associate_known alone, per window':<56}{med(ta, STEPS)}")

                def up_host():
                    hl = [host_lists(w) for w in wins]
                    bank.upload_stream(lin, ang, [h[0] for h in hl], [h[1] for h in hl], [h[2] for h in hl])
                tu = clock(bank, reset, lambda: bank.upload_detections(lin, ang, wins), reps)
                th = clock(bank, reset, up_host, reps)
                rows += [f"    {'upload_detections, 200 windows (ms)':<56}{med(tu, 1e3)}",
                         f"    {'200 x associate_known + upload_stream (ms)':<56}{med(th, 1e3)}   host / device {np.median(th) / np.median(tu):.2f}"]
                for name, kw in (("no resampling", dict(fraction=0.0)), (f"fraction {FRACTION}, split {SPLIT}", dict(fraction=FRACTION, split=SPLIT, u=u, z=z))):
                    bank.upload_detections(lin, ang, wins)
                    tr = clock(bank, reset, lambda: bank.run(0, STEPS, **kw), reps)
                    bank.upload_stream(lin, ang, [d[0] for d in dev], [d[1] for d in dev], [d[2] for d in dev])
                    ti = clock(bank, reset, lambda: bank.run(0, STEPS, **kw), reps)
                    rows += [f"    {'run on the detection stream, per step, ' + name:<56}{med(tr, STEPS)}",
                             f"    {'run on the index stream, per step, ' + name:<56}{med(ti, STEPS)}   detection / index {np.median(tr) / np.median(ti):.3f}"]
            for r in rows:
                print(r, flush=True)
            lines.extend(rows + [""])
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hyp_detections.txt"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    lines = run(args)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
