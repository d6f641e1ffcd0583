#!/usr/bin/env python3
"""Cost of EkfSlam.fork / copy_from (ekf_copy_trajectories; k_copy_traj, csrc/ekf_copy.hip) against the route without it:
one state() into pinned memory plus one set_state() per destination.

Shapes: 32 x N = 2000 fork 1 -> 31; N = 2000 handle -> handle 1 -> 1; N = 8000 x 2 fork 1 -> 1; 256 x N = 20 fork 1 -> 255.
Per shape a real state (diagonal start, a few stream steps), then what is pending is flushed and the stream drained BEFORE
the timed region, so the copy alone is timed: HIP events on the destination handle's stream around the call (the call's
own table upload, its launch and its two synchronisations), the median of `--reps` repetitions after `--warm` warm ones.
Bytes moved = (sources + destinations) x 8 n (n + 1) / 2; the yardstick is the measured float4 copy rate of the part,
6.29 TB/s, not the 8 TB/s of the data sheet.  The first shape is timed with nontemporal and with plain stores
(EKFSLAM_HIP_COPY_NT, read per call).  Kernel times without the call's host part come from a kernel trace:
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python3 tools/copy_trajectories_time.py
(profiles/copy_trajectories.txt)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12


def prepared(sd, orc, N, B, steps=6):
    n = 3 + 2 * N
    mean0, diag0, lin, ang, idx, zr, zb = orc.synthetic_stream(N, steps, 8, 0)
    rep = lambda a: np.repeat(a[:, None], B, 1)
    f = sd.EkfSlam(n, batch=B)
    for b in range(B):
        f.set_state_diag(mean0 + 0.01 * b, diag0, b)
    f.run_stream(rep(lin), rep(ang), rep(idx), rep(zr), rep(zb))
    f.flush()
    f.sync()
    return f


def timed(dst, call, warm, reps):
    ms = []
    for i in range(warm + reps):
        dst.flush()
        dst.sync()
        dst.timer_begin()
        call()
        t = dst.timer_end()
        if i >= warm:
            ms.append(t)
    return float(np.median(ms)), float(min(ms))


def report(name, n, srcs, dsts, med, lo):
    gb = (srcs + dsts) * 8.0 * n * (n + 1) / 2
    rate = gb / (med * 1e-3)
    print(f"{name:44s} n={n:6d}  moved {gb / 1e9:7.3f} GB  median {med:9.3f} ms (min {lo:.3f})  {rate / 1e12:5.2f} TB/s = "
          f"{rate / COPY_RATE:4.2f} of the 6.29 TB/s copy rate", flush=True)
    return med


def host_route(f, g, dsts, reps):
    """state(0) of f into pinned memory, then set_state into every destination of g: wall time."""
    ms = []
    for _ in range(reps):
        f.sync()
        t0 = time.perf_counter()
        mu, P = f.state(0)
        for d in dsts:
            g.set_state(mu, P, d)
        ms.append(1e3 * (time.perf_counter() - t0))
        del mu, P
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1,2,3,4")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=2)
    a = ap.parse_args()
    import slam_duckietown_amd as sd
    from oracle import ekf_oracle as orc
    shapes = [int(x) for x in a.shapes.split(",")]
    if 1 in shapes:
        f = prepared(sd, orc, 2000, 32)
        n = f.size(0)
        for nt in ("1", "0"):
            os.environ["EKFSLAM_HIP_COPY_NT"] = nt
            med = report(f"32 x N=2000 fork 1 -> 31 ({'nontemporal' if nt == '1' else 'plain'} stores)", n, 1, 31,
                         *timed(f, lambda: f.fork(0), a.warm, a.reps))
        os.environ.pop("EKFSLAM_HIP_COPY_NT")
        med = report("32 x N=2000 fork 1 -> 31 (default)", n, 1, 31, *timed(f, lambda: f.fork(0), a.warm, a.reps))
        host = host_route(f, f, range(1, 32), a.host_reps)
        print(f"{'  state() + 31 x set_state()':44s} wall median {host:9.3f} ms: the fork is {host / med:.0f} x faster", flush=True)
        f.close()
    if 2 in shapes:
        f, g = prepared(sd, orc, 2000, 1), prepared(sd, orc, 2000, 1)
        n = f.size(0)
        med = report("N=2000 handle -> handle 1 -> 1", n, 1, 1, *timed(g, lambda: g.copy_from(f), a.warm, a.reps))
        host = host_route(f, g, [0], a.host_reps)
        print(f"{'  state() + set_state()':44s} wall median {host:9.3f} ms: the copy is {host / med:.0f} x faster", flush=True)
        f.close()
        g.close()
    if 3 in shapes:
        f = prepared(sd, orc, 8000, 2, steps=3)
        n = f.size(0)
        med = report("2 x N=8000 fork 1 -> 1", n, 1, 1, *timed(f, lambda: f.fork(0, 1), a.warm, a.reps))
        host = host_route(f, f, [1], 1)
        print(f"{'  state() + set_state()':44s} wall median {host:9.3f} ms: the fork is {host / med:.0f} x faster", flush=True)
        f.close()
    if 4 in shapes:
        f = prepared(sd, orc, 20, 256)
        n = f.size(0)
        med = report("256 x N=20 fork 1 -> 255", n, 1, 255, *timed(f, lambda: f.fork(0), a.warm, a.reps))
        host = host_route(f, f, range(1, 256), a.host_reps)
        print(f"{'  state() + 255 x set_state()':44s} wall median {host:9.3f} ms: the fork is {host / med:.0f} x faster", flush=True)
        f.close()


if __name__ == "__main__":
    main()
