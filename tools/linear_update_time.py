#!/usr/bin/env python3
"""EkfSlam.update_linear() -- a dense H over the pose and up to 16 landmarks, applied on the device -- timed at four settings:
  1. 32 x N = 2000, D = 4 rows over 2 landmarks per trajectory (one k-tile);
  2. 32 x N = 2000, D = 32 rows over 16 landmarks per trajectory (eight k-tiles);
  3. N = 2000 x 1, D = 32;
  4. 256 x N = 20 (small-state path), D = 4.
Per setting: (a) the whole call (host clock around the call, which blocks); (b) k_linear alone and (c) the covariance pass
behind it (event pairs: option "profile_kernels", class 5 and ekf_profile_read); against (d) update_direct() at the same
kpad -- landmark fixes with as many rows -- as a whole call, (e) its k_direct alone (class 4) and (f) its pass; and (g) the
route without the call: state() + the NumPy update + set_state() for every trajectory of the bank.
Every state index is active ("active_bound" 0), so that the passes of both calls cover the same triangle.  Medians, with the
spread (min .. max) of the repetitions.  The file ends with the registers, LDS and scratch of every k_linear instantiation
(tools/kernel_resources.py).
  python3 tools/linear_update_time.py [--reps 10] [--slow-reps 2] [--out profiles/linear_update.txt]
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


def med(xs):
    return f"{np.median(xs):9.3f} ({np.min(xs):.3f} .. {np.max(xs):.3f})"


def host_route(f, meas):
    for b, (lms, H, R, z) in enumerate(meas):
        mean, cov = f.state(b)
        s = [0, 1, 2]
        for l in lms:
            s += [3 + 2 * l, 4 + 2 * l]
        U = H @ cov[s, :]
        S = U[:, s] @ H.T + R
        f.set_state(mean + U.T @ np.linalg.solve(S, z - H @ mean[s]), cov - U.T @ np.linalg.solve(S, U), b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--slow-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_update.txt"))
    args = ap.parse_args()
    import slam_duckietown_amd as sd
    import slam_duckietown_amd.synthetic as syn
    lines = ["EkfSlam.update_linear(): ms per call for the whole bank, median (min .. max)",
             f"(tools/linear_update_time.py; {args.reps} repetitions after 2 warm-up, the host route {args.slow_reps})", ""]

    def setting(title, N, B, D):
        rng = np.random.default_rng(N + B + D)
        k = D // 2
        streams = [syn.synthetic_stream(N, 12, 8, t) for t in range(B)]
        with sd.EkfSlam(3 + 2 * N, batch=B) as f:
            f.set_option("active_bound", 0)
            f.set_option("fused_cadence", 0)
            f.set_option("profile_kernels", 1)
            for b, s in enumerate(streams):
                f.set_state_diag(s[0], s[1], b)
            for t in range(4):
                f.step(np.array([s[2][t] for s in streams]), np.array([s[3][t] for s in streams]),
                       np.stack([s[4][t] for s in streams]), np.stack([s[5][t] for s in streams]),
                       np.stack([s[6][t] for s in streams]))
            f.flush()
            meas, fixes = [], []
            for b in range(B):
                mu = f.mean(b)
                lms = [int(j) for j in rng.permutation(min(32, N))[:k]]
                s = [0, 1, 2] + [3 + 2 * l + a for l in lms for a in range(2)]
                H = rng.uniform(-1.0, 1.0, (D, len(s)))
                meas.append((lms, H, np.diag(np.full(D, 0.05 ** 2)), H @ mu[s] + rng.normal(0.0, 0.02, D)))
                z = [np.concatenate([mu[3 + 2 * l:5 + 2 * l] + rng.normal(0.0, 0.02, 2), [0.0]]) for l in lms]
                fixes.append((lms, z, [np.diag([0.05 ** 2, 0.05 ** 2, 1.0])] * k))
            call = lambda: f.update_linear([m[0] for m in meas], [m[1] for m in meas], [m[2] for m in meas], z=[m[3] for m in meas])
            direct = lambda: f.update_direct([x[0] for x in fixes], [x[1] for x in fixes], [x[2] for x in fixes])
            times = {}
            for name, fn, cls in (("linear", call, 5), ("direct", direct, 4)):
                fn()
                fn()
                ta, tb, tc = [], [], []
                for _ in range(args.reps):
                    f.profile_enable(True)
                    f.sync()
                    t0 = time.perf_counter()
                    fn()
                    ta.append((time.perf_counter() - t0) * 1e3)
                    tb.append(f.profile_read_class(cls)[0])
                    tc.append(f.profile_read()[0])
                times[name] = (ta, tb, tc)
            la, lb, lc = times["linear"]
            da, db, dc = times["direct"]
            tiles = (D + 3) // 4
            rows = [f"{title}  (D = {D} over {k} landmarks, {tiles} k-tile{'s' if tiles > 1 else ''}; last pass {f.last_pass()})",
                    f"    (a) whole call                    {med(la)}",
                    f"    (b) k_linear                      {med(lb)}",
                    f"    (c) its covariance pass           {med(lc)}",
                    f"    (d) update_direct, {D} rows: call  {med(da)}   (a) - (d) = {np.median(la) - np.median(da):+.3f}",
                    f"    (e) k_direct                      {med(db)}   (b) - (e) = {np.median(lb) - np.median(db):+.3f}",
                    f"    (f) its covariance pass           {med(dc)}"]
            tg = []
            for _ in range(args.slow_reps):
                f.sync()
                t0 = time.perf_counter()
                host_route(f, meas)
                f.sync()
                tg.append((time.perf_counter() - t0) * 1e3)
            rows.append(f"    (g) state() + NumPy + set_state() {med(tg)}   (g) / (a) = {np.median(tg) / np.median(la):.1f} x")
            for r in rows:
                print(r, flush=True)
            lines.extend(rows + [""])

    setting("32 x N = 2000", 2000, 32, 4)
    setting("32 x N = 2000", 2000, 32, 32)
    setting("N = 2000 x 1", 2000, 1, 32)
    setting("256 x N = 20 (small-state path)", 20, 256, 4)
    import kernel_resources
    buf = io.StringIO()
    argv = sys.argv
    sys.argv = [argv[0], "k_linear"]
    with contextlib.redirect_stdout(buf):
        kernel_resources.main()
    sys.argv = argv
    lines += ["k_linear's instantiations (tools/kernel_resources.py k_linear):"] + buf.getvalue().splitlines()
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
