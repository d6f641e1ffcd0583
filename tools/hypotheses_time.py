#!/usr/bin/env python3
"""HypothesisBank.step() -- K pose hypotheses on ONE frozen map, two launches per step -- timed beside EkfSlam.localize() on a
bank of forked slots holding the same map, with the bytes both routes allocate, and HypothesisBank.adopt():
  1. N = 2000, m = 8, shared observations, K = 32, 1024, 4096 hypotheses; beside them localize() on a 32-slot forked bank;
  2. N = 8000, K = 32; beside it localize() on a 32-slot forked bank (64 GB: --no-big-fork leaves it out).
A setting's map: a block-diagonal state, the first `--warm` steps of a synthetic stream as SLAM steps, flush(), every state index
active ("active_bound" 0).  Then `--steps` further steps of that stream per repetition: (a) host clock around the enqueue of all
of them, (b) host clock including the final sync, each divided by the number of steps; for localize() also (c) device time (the
handle's event pair).  Steps follow one another on one stream, so (b) is the device's time per step wherever the enqueue (a) is
shorter.  Medians over `--reps` repetitions with the spread (min .. max).  Bytes: what the layout asks for (computed from the
shapes), and what the runtime reports as the drop in free device memory across the allocation.
Per-kernel device times come from a kernel trace of the same work, taken in a run of its own:
    rocprofv3 --kernel-trace --output-format csv -d OUT -o run -- python3 tools/hypotheses_time.py --trace-run
    python3 tools/hypotheses_time.py --kernels OUT --out profiles/hypotheses.txt      # appends the table; needs no device
  python3 tools/hypotheses_time.py [--steps 200] [--reps 5] [--out profiles/hypotheses.txt]
Nothing is checked here, only timed."""
import argparse
import collections
import csv
import ctypes as C
import glob
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

M = 8
SETTINGS = [(2000, (32, 1024, 4096)), (8000, (32,))]
FORK = 32


def med(xs):
    xs = np.asarray(xs)
    return f"{np.median(xs):9.1f} ({np.min(xs):.1f} .. {np.max(xs):.1f})"


def free_bytes():
    """Free device memory as the HIP runtime the library has loaded reports it."""
    path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)
    free, total = C.c_size_t(), C.c_size_t()
    assert C.CDLL(path).hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def layout(n):
    """(ld, doubles of one stored triangle) as ekf_create lays a trajectory out (csrc/ekf_device.h: p_alloc)."""
    rows = (n + 63) // 64 * 64
    if n <= 4096:
        ld = 64
        while ld < n:
            ld *= 2
        return ld, rows * ld
    return rows, -(-rows // 4096) * rows * 4096


def timed(fn, sync, steps, reps):
    fn()
    sync()
    ta, tb = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ta.append((time.perf_counter() - t0) * 1e6 / steps)
        sync()
        tb.append((time.perf_counter() - t0) * 1e6 / steps)
    return ta, tb


def run(args, trace):
    import slam_duckietown_amd as sd
    import slam_duckietown_amd.synthetic as syn
    steps, W, reps = (20, args.warm, 1) if trace else (args.steps, args.warm, args.reps)
    lines = ["HypothesisBank.step() beside EkfSlam.localize() on forked slots: microseconds per step for all hypotheses, median (min .. max)",
             f"(tools/hypotheses_time.py; {steps} steps per repetition behind {W} SLAM steps and a flush, {reps} repetitions, m = {M}, shared "
             "observations, every index active)", ""]
    for N, counts in SETTINGS:
        n = 3 + 2 * N
        ld, tri = layout(n)
        s = syn.synthetic_stream(N, W + 40, M, 0)
        obs = [(s[2][W + k % 40], s[3][W + k % 40], s[4][W + k % 40], s[5][W + k % 40], s[6][W + k % 40]) for k in range(steps)]
        with sd.EkfSlam(n, batch=1) as f:
            f.set_option("active_bound", 0)
            f.set_state_diag(s[0], s[1])
            f.stream_upload(*(np.asarray(s[i])[:, None] for i in (2, 3, 4, 5, 6)))
            f.stream_run(0, W)
            f.flush()
            f.sync()
            rows = [f"N = {N} (n = {n}, one stored triangle {tri * 8 / 1e6:.1f} MB)"]
            for K in counts:
                before = free_bytes()
                with f.hypotheses(K) as bank:
                    used = before - free_bytes()
                    asked = 8 * (tri + ld) + K * (112 + 24 * ld + 928)
                    ta, tb = timed(lambda: [bank.step(*o) for o in obs], bank.sync, steps, reps)
                    rows += [f"    bank, K = {K:<5d}    (a) enqueue      {med(ta)}", f"    {'':<19}(b) with sync    {med(tb)}",
                             f"    {'':<19}bytes: map {8 * (tri + ld) / 1e6:.1f} MB + hypotheses {K * (1040 + 24 * ld) / 1e6:.2f} MB = {asked / 1e6:.1f} MB "
                             f"asked for; free device memory fell by {used / 1e6:.1f} MB"]
                    if K == counts[0]:
                        with sd.EkfSlam(n, batch=2) as g:      # adopt: into a fork of the source (slot 1 of a copy of it)
                            g.set_option("active_bound", 0)
                            g.copy_from(f, [0, 0], [0, 1])
                            g.sync()
                            tw = []
                            for r in range(max(reps, 3)):
                                t0 = time.perf_counter()
                                bank.adopt(r % K, g, 1)
                                tw.append((time.perf_counter() - t0) * 1e6)
                            rows += [f"    adopt (blocking: compare of both triangles, the write, two synchronisations)  {med(tw[1:])} us per call"]
            if N == 2000 or not (args.no_big_fork or trace):
                before = free_bytes()
                with sd.EkfSlam(n, batch=FORK) as g:
                    g.set_option("active_bound", 0)
                    g.copy_from(f, [0] * FORK, list(range(FORK)))
                    g.sync()
                    used = before - free_bytes()
                    lo = [(np.full(FORK, o[0]), np.full(FORK, o[1]), np.tile(o[2], (FORK, 1)), np.tile(o[3], (FORK, 1)), np.tile(o[4], (FORK, 1)))
                          for o in obs]
                    ta, tb = timed(lambda: [g.localize(*o) for o in lo], g.sync, steps, reps)
                    tc = []
                    for _ in range(reps):
                        g.timer_begin()
                        for o in lo:
                            g.localize(*o)
                        tc.append(g.timer_end() * 1e3 / steps)
                    rows += [f"    localize(), {FORK} forked slots   (a) enqueue      {med(ta)}", f"    {'':<30}(b) with sync    {med(tb)}",
                             f"    {'':<30}(c) device       {med(tc)}",
                             f"    {'':<30}bytes: {FORK} stored triangles = {FORK * 8 * tri / 1e6:.1f} MB asked for; free device memory fell by "
                             f"{used / 1e6:.1f} MB (the handle's other buffers included)"]
            else:
                rows += [f"    localize(), {FORK} forked slots: not measured (--no-big-fork); {FORK} stored triangles = {FORK * 8 * tri / 1e6:.1f} MB"]
        for r in rows:
            print(r, flush=True)
        lines.extend(rows + [""])
    return lines


def kernels(directory):
    """Per (kernel, grid): calls and median / min duration in microseconds from rocprofv3's *_kernel_trace.csv under `directory`."""
    agg = collections.defaultdict(list)
    for path in sorted(glob.glob(os.path.join(directory, "**", "*_kernel_trace.csv"), recursive=True)):
        for r in csv.DictReader(open(path)):
            name = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("ekf::", "")
            if name.startswith(("k_hyp_", "k_loc_")):
                agg[(name, int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]), int(r["Grid_Size_Y"]))].append(
                    int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    lines = ["Kernels alone (rocprofv3 --kernel-trace of `--trace-run`, a run of its own; microseconds; workgroups x rows of the grid: k_hyp_solve "
             "K x 1, k_hyp_rows column groups x K, k_loc_* the same with the slots for K)"]
    for (name, gx, gy), v in sorted(agg.items()):
        lines.append(f"    {name:<16} grid {gx:>5d} x {gy:<5d} calls {len(v):5d}   median {statistics.median(v) / 1e3:8.1f}   min {min(v) / 1e3:8.1f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hypotheses.txt"))
    ap.add_argument("--no-big-fork", action="store_true", help="leave out localize() on 32 forked slots at N = 8000 (64 GB)")
    ap.add_argument("--trace-run", action="store_true", help="the same work, briefly and untimed: the program to put behind rocprofv3")
    ap.add_argument("--kernels", default=None, help="append the per-kernel table from the kernel trace under this directory to --out")
    args = ap.parse_args()
    if args.trace_run:
        run(args, True)
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.kernels:
        with open(args.out, "a") as fh:
            fh.write("\n".join(kernels(args.kernels)) + "\n")
        return
    lines = run(args, False)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
