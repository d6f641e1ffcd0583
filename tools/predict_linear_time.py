#!/usr/bin/env python3
"""EkfSlam.predict_linear() -- a prediction with the caller's motion model, applied to rows 0..2 of the covariance on the
device, never a covariance pass -- timed at six settings:
  1. 32 x N = 2000, nothing pending;
  2. 32 x N = 2000, 78 ranks pending (80 as whole k-tiles: the most a handle ever holds);
  3. N = 2000 x 1, nothing pending;
  4. N = 2000 x 1, 78 ranks pending;
  5. N = 8000 x 1 under a small active bound (landmarks 0 .. 39 observed: bound 83);
  6. 256 x N = 20 (small-state path).
Per setting, for predict_linear() and for the built-in predict() -- the yardstick; its code is the parent commit's, this call
leaves it untouched -- at the same state: (a) the enqueue (host clock around the asynchronous call), (b) call + sync() (host
clock), (c) device time (the handle's event pair around the call); for predict_linear also (d) k_predict_pose alone (event
pair: option "profile_kernels", class 7, in repetitions of its own).  Then (e) the host route, state() + the NumPy model +
set_state() for every trajectory of the bank (where nothing is pending), and for the single-trajectory settings (f)
predict_dense() with the n x n F = blockdiag(F, I) and Q.  Every state index is active ("active_bound" 0) except in setting 5.
Medians, with the spread (min .. max) of the repetitions.  The file ends with the registers, LDS and scratch of both
instantiations of k_predict_pose (tools/kernel_resources.py).
  python3 tools/predict_linear_time.py [--reps 200] [--slow-reps 2] [--out profiles/predict_linear.txt]
Nothing is checked here, only timed."""
import argparse
import contextlib
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def med(xs, unit=1e3):
    xs = np.asarray(xs) * unit
    return f"{np.median(xs):10.1f} ({np.min(xs):.1f} .. {np.max(xs):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--slow-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_linear.txt"))
    ap.add_argument("--only", type=int, default=0, help="one setting (1..6) only")
    args = ap.parse_args()
    import slam_duckietown_amd as sd
    import slam_duckietown_amd.synthetic as syn
    lines = ["EkfSlam.predict_linear() beside the built-in predict(): microseconds per call for the whole bank, median (min .. max)",
             f"(tools/predict_linear_time.py; {args.reps} repetitions after 5 warm-up, the host route and predict_dense {args.slow_reps})", ""]

    def setting(title, N, B, pending, bound_all=True, dense=False):
        rng = np.random.default_rng(N + B)
        streams = [syn.synthetic_stream(N, 6, 8, t) for t in range(B)]
        with sd.EkfSlam(3 + 2 * N, batch=B) as f:
            if bound_all:
                f.set_option("active_bound", 0)
            f.set_option("fused_cadence", 0)
            f.set_option("flush_every", 64)                  # (the ranks stay pending up to the last slot)
            f.set_option("profile_kernels", 1)
            for b, s in enumerate(streams):
                f.set_state_diag(s[0], s[1], b)
            for t in range(5):
                m = 7 if t == 4 else 8                       # 4 x 16 + 14 = 78 ranks
                f.step(np.array([s[2][t] for s in streams]), np.array([s[3][t] for s in streams]),
                       np.stack([s[4][t][:m] for s in streams]), np.stack([s[5][t][:m] for s in streams]),
                       np.stack([s[6][t][:m] for s in streams]))
            if not pending:
                f.flush()
            poses = np.stack([f.joint([], b)[0][:3] for b in range(B)])
            F = np.eye(3) + 0.001 * rng.normal(size=(B, 3, 3))
            A = rng.normal(size=(B, 3, 3)) * 0.01
            Q = A @ A.transpose(0, 2, 1)
            lin, ang = np.full(B, 0.01), np.full(B, 0.02)
            calls = {"predict_linear": lambda: f.predict_linear(poses, F, Q), "predict": lambda: f.predict(lin, ang)}
            rows = [f"{title}"]
            res = {}
            # while ranks are pending a predict() counts as a step for "flush_every" (64 at most): its repetitions are cut so
            # that 5 steps + every predict() of this setting stay below it, and the ranks pending throughout
            reps_of = {"predict_linear": args.reps, "predict": min(args.reps, 17) if pending else args.reps}
            td = []
            for name, fn in calls.items():
                reps = reps_of[name]
                for _ in range(5):
                    fn()
                f.sync()
                ta, tb, tc = [], [], []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    fn()
                    ta.append(time.perf_counter() - t0)
                    f.sync()
                for _ in range(reps):
                    t0 = time.perf_counter()
                    fn()
                    f.sync()
                    tb.append(time.perf_counter() - t0)
                for _ in range(reps):
                    f.timer_begin()
                    fn()
                    tc.append(f.timer_end())
                res[name] = (np.array(ta) * 1e3, np.array(tb) * 1e3, np.array(tc))
                if name == "predict_linear":
                    for _ in range(min(args.reps, 50)):
                        f.profile_enable(True)
                        fn()
                        td.append(f.profile_read_class(7)[0])
                        f.profile_read()
                    f.profile_enable(False)
            assert not pending or 5 + 5 + 3 * reps_of["predict"] < 64
            la, lb, lc = res["predict_linear"]
            pa, pb, pc = res["predict"]
            rows += [f"    predict_linear  (a) enqueue        {med(la)}",
                     f"                    (b) call + sync    {med(lb)}",
                     f"                    (c) device         {med(lc)}",
                     f"                    (d) k_predict_pose {med(td)}",
                     f"    predict()       (a) enqueue        {med(pa)}",
                     f"                    (b) call + sync    {med(pb)}",
                     f"                    (c) device         {med(pc)}",
                     f"    predict_linear / predict():  (a) {np.median(la) / np.median(pa):.2f}   (b) {np.median(lb) / np.median(pb):.2f}   "
                     f"(c) {np.median(lc) / np.median(pc):.2f}"]
            if not pending:
                te = []
                for _ in range(args.slow_reps):
                    f.sync()
                    t0 = time.perf_counter()
                    for b in range(B):
                        mean, cov = f.state(b)
                        mean, cov = np.array(mean), np.array(cov)
                        x = F[b] @ cov[:3, :]
                        cov[:3, :] = x
                        cov[:, :3] = x.T
                        cov[:3, :3] = x[:, :3] @ F[b].T + Q[b]
                        mean[:3] = poses[b]
                        f.set_state(mean, cov, b)
                    f.sync()
                    te.append(time.perf_counter() - t0)
                rows.append(f"    (e) state() + NumPy + set_state()  {med(te, 1e6)}   (e) / (b) = {np.median(te) * 1e3 / np.median(lb):.0f} x")
            if dense and not pending:
                n = 3 + 2 * N
                Fd, Qd = np.eye(n), np.zeros((n, n))
                Fd[:3, :3], Qd[:3, :3] = F[0], Q[0]
                tf = []
                for _ in range(args.slow_reps + 1):
                    f.sync()
                    t0 = time.perf_counter()
                    f.predict_dense(Fd, Qd)
                    f.sync()
                    tf.append(time.perf_counter() - t0)
                tf = tf[1:]                                  # (the first call allocates its operands)
                rows.append(f"    (f) predict_dense()                {med(tf, 1e6)}   (f) / (b) = {np.median(tf) * 1e3 / np.median(lb):.0f} x")
            for r in rows:
                print(r, flush=True)
            lines.extend(rows + [""])

    todo = [("32 x N = 2000, nothing pending", 2000, 32, False, True, False),
            ("32 x N = 2000, 78 ranks pending (80 as whole k-tiles)", 2000, 32, True, True, False),
            ("N = 2000 x 1, nothing pending", 2000, 1, False, True, True),
            ("N = 2000 x 1, 78 ranks pending", 2000, 1, True, True, False),
            ("N = 8000 x 1, active bound 83 of 16003, nothing pending", 8000, 1, False, False, True),
            ("256 x N = 20 (small-state path)", 20, 256, False, True, False)]
    for i, t in enumerate(todo):
        if args.only in (0, i + 1):
            setting(*t)
    import kernel_resources
    buf = io.StringIO()
    argv = sys.argv
    sys.argv = [argv[0], "k_predict_pose"]
    with contextlib.redirect_stdout(buf):
        kernel_resources.main()
    sys.argv = argv
    lines += ["k_predict_pose's instantiations (tools/kernel_resources.py k_predict_pose):"] + buf.getvalue().splitlines()
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
