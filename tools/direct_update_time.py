#!/usr/bin/env python3
"""EkfSlam.update_direct() -- absolute pose fixes and surveyed landmarks applied on the device -- timed at five settings:
  1. 32 x N = 2000, a pose fix per trajectory (D = 3: one k-tile);
  2. 32 x N = 2000, a position fix plus 15 landmarks per trajectory (D = 32: eight k-tiles);
  3. N = 2000 x 1, D = 32;
  4. N = 8000 x 1 (P_base in column panels), D = 32;
  5. 256 x N = 20 (small-state path), a pose fix per trajectory.
Per setting: (a) the whole call (host clock around the call, which blocks); (b) k_direct alone and (c) the covariance pass
behind it (event pairs: option "profile_kernels", class 4 and ekf_profile_read); against (d) a plain covariance pass with the
same number of k-tiles (step()s that leave as many ranks pending, then flush(), ekf_profile_read; not on the small-state path,
where nothing is ever pending and (c) is the only pass such a handle ever runs) and (e) the route without
the call: state() + the NumPy update + set_state() for every trajectory of the bank (not at N = 8000: a 2 GB download).
Every state index is active ("active_bound" 0), so that (c) and (d) cover the same triangle.  Medians, with the spread
(min .. max) of the repetitions.
  python3 tools/direct_update_time.py [--reps 10] [--slow-reps 2] [--out profiles/direct_update.txt]
Nothing is checked here, only timed."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(xs):
    return f"{np.median(xs):9.3f} ({np.min(xs):.3f} .. {np.max(xs):.3f})"


def host_route(f, fixes):
    for b, (t, z, R) in enumerate(fixes):
        mean, cov = f.state(b)
        s = []
        for x in t:
            s += [0, 1, 2] if x == -1 else [0, 1] if x == -2 else [3 + 2 * x, 4 + 2 * x]
        D = len(s)
        zz, RR, o = np.zeros(D), np.zeros((D, D)), 0
        for x, zi, Ri in zip(t, z, R):
            d = 3 if x == -1 else 2
            zz[o:o + d], RR[o:o + d, o:o + d] = zi[:d], Ri[:d, :d]
            o += d
        U = cov[s, :]
        S = cov[np.ix_(s, s)] + RR
        f.set_state(mean + U.T @ np.linalg.solve(S, zz - mean[s]), cov - U.T @ np.linalg.solve(S, U), b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--slow-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "direct_update.txt"))
    args = ap.parse_args()
    import slam_duckietown_amd as sd
    import slam_duckietown_amd.synthetic as syn
    lines = ["EkfSlam.update_direct(): ms per call for the whole bank, median (min .. max)",
             f"(tools/direct_update_time.py; {args.reps} repetitions after 2 warm-up, the host route {args.slow_reps})", ""]

    def setting(title, N, B, landmarks, host):
        rng = np.random.default_rng(N + B)
        streams = [syn.synthetic_stream(N, 12, 8, t) for t in range(B)]
        with sd.EkfSlam(3 + 2 * N, batch=B) as f:
            f.set_option("active_bound", 0)
            f.set_option("fused_cadence", 0)
            f.set_option("profile_kernels", 1)
            for b, s in enumerate(streams):
                f.set_state_diag(s[0], s[1], b)
            step = lambda k, m: f.step(np.array([s[2][k] for s in streams]), np.array([s[3][k] for s in streams]),
                                       np.stack([s[4][k][:m] for s in streams]), np.stack([s[5][k][:m] for s in streams]),
                                       np.stack([s[6][k][:m] for s in streams]))
            for k in range(4):
                step(k, 8)
            f.flush()
            fixes = []
            for b in range(B):
                mu = f.mean(b)
                t = ([-2] + [int(j) for j in rng.permutation(32)[:landmarks]]) if landmarks else [-1]
                z, R = [], []
                for x in t:
                    d = 3 if x == -1 else 2
                    a = 0 if x < 0 else 3 + 2 * x
                    zi, Ri = np.zeros(3), np.zeros((3, 3))
                    zi[:d] = mu[a:a + d] + rng.normal(0.0, 0.02, d)
                    Ri[:d, :d] = np.diag(np.full(d, 0.05 ** 2))
                    z.append(zi)
                    R.append(Ri)
                fixes.append((t, z, R))
            call = lambda: f.update_direct([x[0] for x in fixes], [x[1] for x in fixes], [x[2] for x in fixes])
            D = 3 if not landmarks else 2 + 2 * landmarks
            tiles = (D + 3) // 4
            call()
            call()
            ta, tb, tc = [], [], []
            for _ in range(args.reps):
                f.profile_enable(True)
                f.sync()
                t0 = time.perf_counter()
                call()
                ta.append((time.perf_counter() - t0) * 1e3)
                tb.append(f.profile_read_class(4)[0])
                tc.append(f.profile_read()[0])
            # a plain pass of as many k-tiles: steps that leave 4 * tiles ranks pending, then the flush
            td = []
            for r in range(args.reps + 2):
                left, k = 2 * tiles, 4 + (r % 8)
                while left > 0:
                    step(k, min(8, left))
                    left -= min(8, left)
                f.profile_enable(True)
                f.flush()
                td.append(f.profile_read()[0])
            td = td[2:]
            rows = [f"{title}  (D = {D}, {tiles} k-tile{'s' if tiles > 1 else ''}; last pass {f.last_pass()})",
                    f"    (a) whole call          {med(ta)}",
                    f"    (b) k_direct            {med(tb)}",
                    f"    (c) its covariance pass {med(tc)}",
                    (f"    (d) plain pass, {tiles} k-tile{'s' if tiles > 1 else ' '} {med(td)}   (c) / (d) = {np.median(tc) / np.median(td):.3f}"
                     if np.median(td) > 0 else
                     "    (d) no plain pass exists on this path: a small-state handle never has ranks pending, flush() launches nothing")]
            if host:
                te = []
                for _ in range(args.slow_reps):
                    f.sync()
                    t0 = time.perf_counter()
                    host_route(f, fixes)
                    f.sync()
                    te.append((time.perf_counter() - t0) * 1e3)
                rows.append(f"    (e) state() + NumPy + set_state() {med(te)}   (e) / (a) = {np.median(te) / np.median(ta):.1f} x")
            for r in rows:
                print(r, flush=True)
            lines.extend(rows + [""])

    setting("32 x N = 2000, pose fix", 2000, 32, 0, True)
    setting("32 x N = 2000, position + 15 landmarks", 2000, 32, 15, True)
    setting("N = 2000 x 1, position + 15 landmarks", 2000, 1, 15, True)
    setting("N = 8000 x 1, position + 15 landmarks", 8000, 1, 15, False)
    setting("256 x N = 20, pose fix (small-state path)", 20, 256, 0, True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
