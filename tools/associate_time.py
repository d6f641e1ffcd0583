#!/usr/bin/env python3
"""Likelihood association of unlabelled observations (EkfSlam.associate), timed against the host route, at four shapes, each
with a full cadence pending (80 ranks; the small-state shape never has anything pending) and with nothing pending:
  (a) EkfSlam.associate() for the whole bank (one read-only kernel + its finishing launch, no covariance pass);
  (b) the host route: marginals() for the whole bank, covariance_block(0, 3, 3, 2N, b) and mean(b) per trajectory (the cross
      terms; the block download applies the pending update), then the same scores in vectorised NumPy;
  (c) marginals() alone: the floor for a kernel that reads the same V and W.
Writes the table to --out (default profiles/associate.txt).
  python3 tools/associate_time.py [--reps 5] [--warmup 2] [--out profiles/associate.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(32, 2000), (1, 2000), (1, 8000), (256, 20)]      # trajectories x landmarks, m = 8


def host_scores(mu, pose, lms, cross, zr, zb, qd):
    """NIS (m, N) and ln det S (N,) of one trajectory from the marginal blocks and the 3 x 2N cross terms, in NumPy."""
    N = lms.shape[0]
    lm = mu[3:].reshape(N, 2)
    d = lm - mu[:2]
    q = (d * d).sum(1)
    sq = np.sqrt(q)
    H = np.zeros((N, 2, 5))
    H[:, 0, 0], H[:, 0, 1], H[:, 0, 3], H[:, 0, 4] = -d[:, 0] / sq, -d[:, 1] / sq, d[:, 0] / sq, d[:, 1] / sq
    H[:, 1, 0], H[:, 1, 1], H[:, 1, 2], H[:, 1, 3], H[:, 1, 4] = d[:, 1] / q, -d[:, 0] / q, -1.0, -d[:, 1] / q, d[:, 0] / q
    P5 = np.zeros((N, 5, 5))
    P5[:, :3, :3] = pose
    P5[:, 3:, 3:] = lms
    c = cross.reshape(3, N, 2).transpose(1, 0, 2)
    P5[:, :3, 3:] = c
    P5[:, 3:, :3] = c.transpose(0, 2, 1)
    S = H @ P5 @ H.transpose(0, 2, 1)
    S[:, 0, 0] += qd
    S[:, 1, 1] += qd
    det = S[:, 0, 0] * S[:, 1, 1] - S[:, 0, 1] * S[:, 1, 0]
    y0 = zr[:, None] - sq[None, :]
    y1 = (zb[:, None] - (np.arctan2(d[:, 1], d[:, 0]) - mu[2])[None, :] + np.pi) % (2 * np.pi) - np.pi
    nis = (S[:, 1, 1] * y0 * y0 - (S[:, 0, 1] + S[:, 1, 0]) * y0 * y1 + S[:, 0, 0] * y1 * y1) / det
    return nis, np.log(det)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "associate.txt"))
    args = ap.parse_args()
    import slam_duckietown_amd as sd
    import slam_duckietown_amd.synthetic as syn
    m, cad = 8, 5
    lines = [f"EkfSlam.associate() against the host route, m = {m} observations per trajectory; median of {args.reps} repetitions "
             f"after {args.warmup} warm-up, host clock, ms (device events in brackets)",
             "(a) associate()   (b) marginals() + covariance_block(0, 3, 3, 2N, b) + mean(b) per trajectory + NumPy scores   "
             "(c) marginals() alone", ""]
    rng = np.random.default_rng(0)
    for B, N in SHAPES:
        n = 3 + 2 * N
        total = args.warmup + args.reps
        streams = [syn.synthetic_stream(N, cad * total * 2, m, t % 32) for t in range(B)]
        zr, zb = rng.uniform(0.3, 3.0, (B, m)), rng.uniform(-3.0, 3.0, (B, m))
        with sd.EkfSlam(n, batch=B) as f:
            f.set_option("active_bound", 0)
            for b, s in enumerate(streams):
                f.set_state_diag(s[0], s[1], b)
            qd = f.config.meas_sigma ** 2
            step = [0]

            def cadence():
                f.flush()
                for k in range(step[0], step[0] + cad):
                    f.step(np.array([s[2][k] for s in streams]), np.array([s[3][k] for s in streams]),
                           np.stack([s[4][k] for s in streams]), np.stack([s[5][k] for s in streams]),
                           np.stack([s[6][k] for s in streams]))
                step[0] += cad
                f.sync()

            def timed(fn):
                f.sync()
                t0 = time.perf_counter()
                f.timer_begin()
                fn()
                dev = f.timer_end()
                f.sync()
                return (time.perf_counter() - t0) * 1e3, dev

            def host_route():
                pose, lms, counts = f.marginals()
                out = []
                for b in range(B):
                    cross = f.covariance_block(0, 3, 3, 2 * N, b)
                    out.append(host_scores(f.mean(b), pose[b], lms[b, :counts[b]], cross, zr[b], zb[b], qd))
                return out

            for pending in (True, False):
                ra, rb, rc = [], [], []
                for r in range(total):
                    cadence()
                    if not pending:
                        f.flush()
                        f.sync()
                    a = timed(lambda: f.associate(zr, zb))
                    c = timed(lambda: f.marginals())
                    b_ = timed(host_route)                 # (last: its block downloads apply what is pending)
                    if r >= args.warmup:
                        ra.append(a)
                        rb.append(b_)
                        rc.append(c)
                med = lambda rs, i: float(np.median([x[i] for x in rs]))
                state = "80 ranks pending" if pending and n > 131 else ("nothing pending" if not pending else
                                                                        "small-state path: nothing is ever pending")
                lines.append(f"{B:4d} x N = {N:5d}, {state:42s} (a) {med(ra, 0):8.3f} [{med(ra, 1):7.3f}]   "
                             f"(b) {med(rb, 0):9.3f}   (c) {med(rc, 0):8.3f} [{med(rc, 1):7.3f}]")
                print(lines[-1], flush=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
