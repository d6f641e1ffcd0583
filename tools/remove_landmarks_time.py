#!/usr/bin/env python3
"""Cost of EkfSlam.remove_landmarks (k_remove, csrc/ekf_remove.hip) on a bank: the worst case (landmark 0: the whole triangle
moves up by two rows), the cheapest (the last landmark: only the vacated corner), and 100 scattered landmarks.

Per case a fresh state (diagonal start, a few stream steps, ranks left pending so the call forces its covariance pass first),
then one removal; `--reps` of each, in this order.  Prints the moved bytes (read + write of every stored upper-triangle entry
that moves) and the call's wall time.  Kernel times come from a run under the kernel trace, which lists every launch in order
(profiles/remove_landmarks.txt):
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python3 tools/remove_landmarks_time.py
    python3 tools/remove_landmarks_time.py --trace OUT        (per-case k_remove / pass times from the trace)
"""
import argparse
import csv
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12


def cases(N):
    rng = np.random.default_rng(0)
    return [("index 0", [0]), ("last index", [N - 1]), ("100 scattered", sorted(rng.choice(N, 100, replace=False).tolist()))]


def moved_bytes(n, lms, batch):
    """read + write of the stored upper-triangle entries that move (those with both indices below the first removed one stay)."""
    r0 = 3 + 2 * min(lms)
    n_new = n - 2 * len(lms)
    return 16.0 * batch * (n_new * (n_new + 1) / 2 - r0 * (r0 + 1) / 2)


def run(args):
    import slam_duckietown_amd as sd
    from oracle import ekf_oracle as orc
    N, B = args.N, args.batch
    n = 3 + 2 * N
    mean0, diag0, lin, ang, idx, zr, zb = orc.synthetic_stream(N, 12, 8, 0)
    rep = lambda a: np.repeat(a[:, None], B, 1)
    with sd.EkfSlam(n, batch=B) as f:
        for name, lms in cases(N):
            ms = []
            for _ in range(args.reps):
                for b in range(B):
                    f.set_state_diag(mean0, diag0, b)
                f.run_stream(rep(lin), rep(ang), rep(idx), rep(zr), rep(zb))
                f.sync()
                t0 = time.perf_counter()
                f.remove_landmarks(lms, None)
                ms.append(1e3 * (time.perf_counter() - t0))
                assert f.size(0) == n - 2 * len(lms) and f.flags(0) == 0
            mb = moved_bytes(n, lms, B)
            print(f"{name:14s} k={len(lms):3d}  moved {mb / 1e9:6.3f} GB  call wall median {np.median(ms):7.3f} ms  "
                  f"(min {min(ms):.3f})", flush=True)


def launches(out_dir):
    """(name, start ns, end ns) of every kernel launch of a trace, in order: the rocpd database rocprofv3 writes by default
    (its `kernels` view), else the CSV of --output-format csv."""
    import sqlite3
    rows = []
    for fn in glob.glob(os.path.join(out_dir, "**", "*_results.db"), recursive=True):
        con = sqlite3.connect(fn)
        rows += con.execute("select name, start, end from kernels").fetchall()
        con.close()
    for fn in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(fn) as fh:
            rows += [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(fh)]
    return sorted(rows, key=lambda r: r[1])


def trace(args):
    """Per case, the k_remove launches and the covariance passes right before them (the pending update the call applies first),
    from a kernel trace of `run`."""
    rows = launches(args.trace)
    N, B = args.N, args.batch
    n = 3 + 2 * N
    rm, last_pass, before = [], None, {}
    for r in rows:
        if "k_flush" in r[0]:
            last_pass = r
        elif "k_remove" in r[0]:
            rm.append(r)
            before[len(rm) - 1] = last_pass
    for c, (name, lms) in enumerate(cases(N)):
        sel = range(c * args.reps, (c + 1) * args.reps)
        us = [(rm[i][2] - rm[i][1]) / 1e3 for i in sel]
        fl = [(before[i][2] - before[i][1]) / 1e3 for i in sel if before[i]]
        mb = moved_bytes(n, lms, B)
        med = float(np.median(us))
        frac = f"{mb / (med * 1e-6) / 1e12:.2f} TB/s = {mb / (med * 1e-6) / PEAK:.2f} of peak" if mb else "nothing moves"
        print(f"{name:14s} k={len(lms):3d} {rm[sel[0]][0].split('(')[0]:18s} median {med:8.1f} us (min {min(us):.1f}, "
              f"{len(us)} launches)  moved {mb / 1e9:.3f} GB: {frac};  the forced pass before it: median {np.median(fl):.1f} us")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=2000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace", default=None)
    a = ap.parse_args()
    trace(a) if a.trace else run(a)
