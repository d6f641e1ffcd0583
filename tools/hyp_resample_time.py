#!/usr/bin/env python3
"""HypothesisBank.resample() -- weights, systematic resampling, copy and split on the device -- timed at N = 2000 for K = 32, 1024
and 4096 hypotheses, beside HypothesisBank.step() at the same K:
  typical   log-likelihoods shaped so that the effective sample size is about K / 2 (one update per hypothesis of one landmark
            seen at its predicted range + 2.5 sigma of the range innovation x a normal draw);
  one-hot   one hypothesis takes every offspring: K - 1 copies of one source, the most bytes a resampling can move;
each without and with a split (s = 0.5), the one-hot copy also with plain instead of nontemporal stores (EKFSLAM_HIP_HYP_COPY_NT=0).
A repetition shapes the weights again (a resampling leaves them uniform), synchronises, and then clocks on the host (a) the call
with every output NULL (asynchronous) and (b) the same including the bank's sync; (c) is the blocking form with all outputs.
Medians over `--reps` repetitions with the spread (min .. max).  Bytes: what the plan says the copy and the split move -- per dead
slot 24 ldx bytes written and as many read, per split slot 24 ldx read and written in place, the 112-byte records beside them; a
one-hot copy reads ONE source again and again, which the caches serve: its reads are counted once -- and the bytes over (b) as a
fraction of the 4.8 TB/s EkfSlam.fork was measured at (profiles/copy_trajectories.txt): a LOWER bound of the kernels' rate, (b)
holding three or four launches and the synchronisation.
Per-kernel device times come from a kernel trace of the same work, taken in a run of its own:
    rocprofv3 --kernel-trace --output-format csv -d OUT -o run -- python3 tools/hyp_resample_time.py --trace-run
    python3 tools/hyp_resample_time.py --kernels OUT --out profiles/hyp_resample.txt      # appends the table; needs no device
  python3 tools/hyp_resample_time.py [--reps 7] [--out profiles/hyp_resample.txt]
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

N, M, COUNTS, SPLIT = 2000, 8, (32, 1024, 4096), 0.5
FORK_RATE = 4.8e12


def med(xs):
    xs = np.asarray(xs)
    return f"{np.median(xs):9.1f} ({np.min(xs):.1f} .. {np.max(xs):.1f})"


def range_precision(f, idx, r0, b0):
    """(S^-1)_rr of landmark idx's innovation at the map's own pose, from two hypotheses one metre apart in range."""
    with f.hypotheses(2) as probe:
        probe.update([idx] * 2, [[r0], [r0 + 1.0]], [[b0]] * 2)
        ll = probe.loglik
    return -2.0 * (ll[1] - ll[0])


def run(args, trace):
    import slam_duckietown_amd as sd
    import slam_duckietown_amd.synthetic as syn
    reps, W = (2, args.warm) if trace else (args.reps, args.warm)
    lib = sd.load_library()
    dp = C.POINTER(C.c_double)
    n = 3 + 2 * N
    ld = 64
    while ld < n:
        ld *= 2
    lines = ["HypothesisBank.resample(): microseconds per call, median (min .. max)",
             f"(tools/hyp_resample_time.py; N = {N}, ldx = {ld}, {reps} repetitions behind {W} SLAM steps and a flush; split s = {SPLIT})", ""]
    s = syn.synthetic_stream(N, W + 40, M, 0)
    rng = np.random.default_rng(1)
    with sd.EkfSlam(n, batch=1) as f:
        f.set_option("active_bound", 0)
        f.set_state_diag(s[0], s[1])
        f.stream_upload(*(np.asarray(s[i])[:, None] for i in (2, 3, 4, 5, 6)))
        f.stream_run(0, W)
        f.flush()
        f.sync()
        mean = f.mean(0)
        lm = int(s[4][W - 1][0])                                               # a landmark the map has seen
        dxy = mean[3 + 2 * lm:5 + 2 * lm] - mean[:2]
        r0, b0 = float(np.hypot(*dxy)), float(np.arctan2(dxy[1], dxy[0]) - mean[2])
        idx = np.array([lm], dtype=np.int32)
        sigma = 1.0 / np.sqrt(range_precision(f, idx, r0, b0))
        obs = (s[2][W], s[3][W], s[4][W], s[5][W], s[6][W])
        for K in COUNTS:
            z = rng.standard_normal((K, 3))
            onehot = np.full(K, 60.0 * sigma)
            onehot[K // 3] = 0.0
            shapes = {"typical": 2.5 * sigma * rng.standard_normal(K), "one-hot": onehot}
            rows = [f"K = {K} (pose rows {K * 24 * ld / 1e6:.1f} MB)"]
            with f.hypotheses(K) as bank:
                def shape(d):
                    bank.update([idx] * K, [[r0 + x] for x in d], [[b0]] * K)
                    bank.sync()

                ts = []
                for _ in range(max(reps, 3)):
                    t0 = time.perf_counter()
                    bank.step(*obs)
                    bank.sync()
                    ts.append((time.perf_counter() - t0) * 1e6)
                rows.append(f"    step (m = {M}, shared), call + sync {'':<22}{med(ts[1:])}")
                for name, d in shapes.items():
                    for split, nt in ((0.0, "1"), (SPLIT, "1")) + (((0.0, "0"),) if name == "one-hot" else ()):
                        os.environ["EKFSLAM_HIP_HYP_COPY_NT"] = nt
                        zp = z.ctypes.data_as(dp) if split > 0.0 else None
                        ta, tb, tc, plan = [], [], [], None
                        for r in range(reps + 1):                              # (the first repetition warms up)
                            shape(d)
                            ess = bank.ess()
                            t0 = time.perf_counter()
                            rc = lib.ekf_hypotheses_resample(bank._h, 0.37, split, zp, None, None, None, None)
                            t1 = time.perf_counter()
                            bank.sync()
                            t2 = time.perf_counter()
                            assert rc == 0
                            shape(d)
                            t3 = time.perf_counter()
                            plan = bank.resample(u=0.37, split=split, z=z if split > 0.0 else None)
                            t4 = time.perf_counter()
                            if r:
                                ta.append((t1 - t0) * 1e6), tb.append((t2 - t0) * 1e6), tc.append((t4 - t3) * 1e6)
                        dead = int((plan.offspring == 0).sum())
                        moved = int((plan.offspring[plan.ancestors] >= 2).sum()) if split > 0.0 else 0
                        each = 24 * ld + 112                                  # a hypothesis's rows and record
                        wrote = (dead + moved) * each                          # the copy writes dead slots, the split rewrites its slots
                        read = wrote if name != "one-hot" else moved * each + each   # (one-hot: ONE source, re-read from cache)
                        rw, rr = wrote / (np.median(tb) * 1e-6), (wrote + read) / (np.median(tb) * 1e-6)
                        what = f"{name}, {'split' if split > 0.0 else 'copy only'}{'' if nt == '1' else ', plain stores'}"
                        rows += [f"    {what:<34} ESS {ess:8.1f}, {dead} dead slots, {moved} split slots, {wrote / 1e6:.2f} MB written, "
                                 f"{read / 1e6:.2f} MB read from memory",
                                 f"    {'':<34} (a) enqueue      {med(ta)}", f"    {'':<34} (b) with sync    {med(tb)}",
                                 f"    {'':<34} (c) blocking     {med(tc)}",
                                 f"    {'':<34} (b) writes {rw / 1e12:.3f} TB/s, moves {rr / 1e12:.3f} TB/s = {100.0 * rr / FORK_RATE:.1f} % of fork's "
                                 "4.8 TB/s (a lower bound)"]
                os.environ.pop("EKFSLAM_HIP_HYP_COPY_NT", None)
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
            if name.startswith(("k_hyp_weigh", "k_hyp_plan", "k_hyp_copy", "k_hyp_split", "k_hyp_solve", "k_hyp_rows")):
                agg[(name, int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]), int(r["Grid_Size_Y"]))].append(
                    int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    lines = ["Kernels alone (rocprofv3 --kernel-trace of `--trace-run`, a run of its own; microseconds; grid: workgroups in x -- K for "
             "k_hyp_copy / k_hyp_split / k_hyp_solve -- by rows in y; typical and one-hot cases, copies and splits are pooled per grid)"]
    for (name, gx, gy), v in sorted(agg.items()):
        lines.append(f"    {name:<22} grid {gx:>5d} x {gy:<5d} calls {len(v):5d}   median {statistics.median(v) / 1e3:8.1f}   min {min(v) / 1e3:8.1f}"
                     f"   max {max(v) / 1e3:8.1f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hyp_resample.txt"))
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
