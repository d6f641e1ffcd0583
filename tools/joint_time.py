#!/usr/bin/env python3
"""EkfSlam.joint() -- the joint covariance of the pose and a landmark subset, read without a covariance pass -- against the
routes that give the same sub-matrix without it, timed at four settings:
  1. 32 x N = 2000, k = 8, 32 and 64 landmarks per trajectory, a full cadence pending (5 steps of m = 8: 80 ranks);
  2. N = 2000 x 1, a chained stream stopped mid-cadence, k = 32;
  3. N = 8000 x 1 (P_base in column panels), k = 8, ranks pending;
  4. 256 x N = 20 (small-state path: nothing is ever pending), every landmark.
Routes: (a) joint() for the whole bank; (b) flush() + covariance_block per block pair (pose and landmarks: (k + 1)(k + 2) / 2
downloads per trajectory; only where that is at most 45 per trajectory); (c) flush() + state() per trajectory + np.ix_
(not at N = 8000: a 2 GB download).  (a) changes nothing and is repeated on the same pending state; (b) and (c) flush, so the
pending state is rebuilt before each of their repetitions.  Host clock around the call and a synchronisation, median.
  python3 tools/joint_time.py [--reps 10] [--slow-reps 3] [--out profiles/joint.txt]
Nothing is checked here, only timed."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def clock(f, fn):
    f.sync()
    t0 = time.perf_counter()
    fn()
    f.sync()
    return (time.perf_counter() - t0) * 1e3


def route_blocks(f, sels):
    f.flush()
    for b, sel in enumerate(sels):
        starts = [(0, 3)] + [(3 + 2 * j, 2) for j in sel]
        for a, (r0, rows) in enumerate(starts):
            for c0, cols in starts[a:]:
                f.covariance_block(r0, c0, rows, cols, b)


def route_state(f, sels):
    f.flush()
    for b, sel in enumerate(sels):
        ix = [0, 1, 2] + [3 + 2 * j + d for j in sel for d in range(2)]
        f.state(b)[1][np.ix_(ix, ix)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--slow-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "joint.txt"))
    args = ap.parse_args()
    import slam_duckietown_amd as sd
    import slam_duckietown_amd.synthetic as syn
    lines = ["EkfSlam.joint() against the routes through flush(): host clock, median, ms per call for the whole bank",
             f"(tools/joint_time.py; joint() {args.reps} repetitions after 2 warm-up, the flushing routes {args.slow_reps})", ""]
    rng = np.random.default_rng(0)

    def report(title, f, sels, rebuild, blocks, state):
        f.joint(sels)
        f.joint(sels)
        ta = np.median([clock(f, lambda: f.joint(sels)) for _ in range(args.reps)])
        row = f"  {title:44s} joint() {ta:9.3f}"
        for name, on, fn in (("flush + covariance_block", blocks, route_blocks), ("flush + state()", state, route_state)):
            if not on:
                continue
            ts = []
            for _ in range(args.slow_reps):
                ts.append(clock(f, lambda: fn(f, sels)))
                rebuild()
            t = np.median(ts)
            row += f"   {name} {t:10.3f} ({t / ta:7.1f} x)"
        lines.append(row)
        print(row, flush=True)

    # 1. the headline bank, a full cadence pending
    N, B, m, cad = 2000, 32, 8, 5
    streams = [syn.synthetic_stream(N, cad * 64, m, t) for t in range(B)]
    with sd.EkfSlam(3 + 2 * N, batch=B) as f:
        f.set_option("active_bound", 0)
        for b, s in enumerate(streams):
            f.set_state_diag(s[0], s[1], b)
        at = [0]

        def cadence():
            f.flush()
            for k in range(cad * at[0], cad * (at[0] + 1)):
                f.step(np.array([s[2][k] for s in streams]), np.array([s[3][k] for s in streams]),
                       np.stack([s[4][k] for s in streams]), np.stack([s[5][k] for s in streams]),
                       np.stack([s[6][k] for s in streams]))
            at[0] += 1
            f.sync()

        cadence()
        for k in (8, 32, 64):
            sels = [[int(j) for j in rng.permutation(N)[:k]] for _ in range(B)]
            report(f"32 x N = 2000, k = {k}, 80 ranks pending", f, sels, cadence, k <= 8, True)

    # 2. one long trajectory, chained, mid-cadence
    N = 2000
    s = syn.synthetic_stream(N, 22, 8, 77)
    args_s = tuple(np.asarray(a)[:, None] for a in (s[2], s[3], s[4], s[5], s[6]))
    with sd.EkfSlam(3 + 2 * N, batch=1) as f:
        def rebuild():
            f.set_state_diag(s[0], s[1])
            f.stream_run(0, 7)
            f.sync()
        f.stream_upload(*args_s)
        rebuild()
        sels = [[int(j) for j in rng.permutation(N)[:32]]]
        report("N = 2000 x 1, chained, mid-cadence, k = 32", f, sels, rebuild, False, True)
        lib = sd.load_library()
        note = (f"    (that handle: ekf_debug_chained = {lib.ekf_debug_chained(f._h)}, cadences / steps = "
                f"{f.cadence_counters()}, ekf_debug_lookaheads = {lib.ekf_debug_lookaheads(f._h)})")
        lines.append(note)
        print(note, flush=True)

    # 3. column panels
    N = 8000
    s = syn.synthetic_stream(N, 3 * (args.slow_reps + 2), 8, 5)
    with sd.EkfSlam(3 + 2 * N, batch=1) as f:
        f.set_option("active_bound", 0)
        f.set_option("fused_cadence", 0)
        f.set_state_diag(s[0], s[1])
        at = [0]

        def steps3():
            f.flush()
            for k in range(3 * at[0], 3 * (at[0] + 1)):
                f.step(s[2][k], s[3][k], s[4][k], s[5][k], s[6][k])
            at[0] += 1
            f.sync()
        steps3()
        sels = [[int(j) for j in np.concatenate([rng.permutation(2040)[:4], 2047 + rng.permutation(5000)[:4]])]]
        report("N = 8000 x 1, k = 8, 48 ranks pending", f, sels, steps3, True, False)

    # 4. the small-state path
    N, B = 20, 256
    streams = [syn.synthetic_stream(N, 12, 8, t) for t in range(B)]
    with sd.EkfSlam(3 + 2 * N, batch=B) as f:
        for b, st in enumerate(streams):
            f.set_state_diag(st[0], st[1], b)
        f.run_stream(*(np.stack([st[i] for st in streams], 1) for i in (2, 3, 4, 5, 6)))
        f.sync()
        sels = [list(range(N)) for _ in range(B)]
        report("256 x N = 20, every landmark, small-state path", f, sels, lambda: None, False, True)

    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
