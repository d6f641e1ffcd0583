#!/usr/bin/env python3
"""A hypothesis bank stepped from UNLABELLED observations -- HypothesisBank.associate / step_unlabelled (k_hyp_score,
csrc/ekf_hyp_assoc.hip) -- against the host route it replaces, at N = 2000, lists of m = 8 observations, for K = 32, 1024 and 4096
hypotheses seeded around the map's pose.  Host-clocked from the first call to the end of the bank's sync unless it says otherwise,
medians over `--reps` repetitions with the spread (min .. max); every repetition starts from the same reset bank.
  associate, call + sync        bank.associate(ranges, bearings): the query, its four candidate arrays copied back.
  k_hyp_score alone             ekf_debug_hyp_score_time: 20 launches of the query between one event pair, per launch.
  step_unlabelled, per step     200 calls behind one sync: prediction, scoring + resolve on the device, solve, rows.
  host route, per step          the sequence of the header's guarantee: step with m = 0, associate, frontend.resolve_associations per
                                hypothesis on the host, update with the K resulting lists; `--host-steps` steps, one sync each.
  labelled step, per step       200 `step` calls with the TRUE labels (one shared list) behind one sync: what ids would cost.
  python3 tools/hyp_associate_time.py [--reps 5] [--out profiles/hyp_associate.txt]
Nothing is checked here, only timed; the one comparison drawn is device route against host route per K, with both spreads."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, M, STEPS, COUNTS = 2000, 8, 200, (32, 1024, 4096)
MAPPED = 160                                                # landmarks the mapping steps observe: the ones the lists draw from
LIN, ANG, ACCEPT = 0.004, 0.02, 9.21
SEED_COV = np.diag([0.02 ** 2, 0.02 ** 2, 0.01 ** 2])
KERNEL_REPS = 20
RECORDED = "---- recorded once"                             # the profile's second part (tools/assoc_hash.py on both trees)


def med(xs, per=1.0):
    xs = np.asarray(xs) / per
    return f"{np.median(xs):10.1f} ({np.min(xs):.1f} .. {np.max(xs):.1f})"


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


def run(args):
    import slam_duckietown_amd as sd
    from slam_duckietown_amd import evaluation as ev
    from slam_duckietown_amd import frontend
    lib = sd.load_library()
    n, reps, hsteps = 3 + 2 * N, args.reps, args.host_steps
    cfg = sd.EkfConfig(motion_sigma=0.02, meas_sigma=0.03)
    miss = ev.clutter_loglik(ACCEPT, cfg.meas_sigma)
    lines = ["A hypothesis bank stepped from unlabelled observations against the host route: microseconds, median (min .. max)",
             f"(tools/hyp_associate_time.py; N = {N}, m = {M}, {STEPS} steps, {reps} repetitions; the map: {MAPPED} landmarks observed once "
             f"from a known pose, then flushed; accept {ACCEPT}, miss {miss:.3f}; the host route over {hsteps} steps)", ""]
    rng = np.random.default_rng(1)
    world = rng.uniform(-3.0, 3.0, (N, 2))
    mean0 = np.concatenate([np.zeros(3), world.ravel()])
    diag0 = np.full(n, 1e4)
    diag0[:3] = 1e-6

    def sight(pose, lms, noise):
        d = world[lms] - pose[:2]
        return np.hypot(d[:, 0], d[:, 1]) + rng.normal(0, noise, len(lms)), np.arctan2(d[:, 1], d[:, 0]) - pose[2] + rng.normal(0, noise, len(lms))

    with sd.EkfSlam(n, batch=1, config=cfg) as f:
        f.set_option("active_bound", 0)
        f.set_state_diag(mean0, diag0)
        for c in range(0, MAPPED, 16):
            lms = np.arange(c, c + 16)
            f.step(0.0, 0.0, lms.astype(np.int32), *sight(np.zeros(3), lms, 0.01))
        f.flush()
        f.sync()
        mean = f.mean(0)
        # the robot moves as the motion model says from the map's pose; every step sees M mapped landmarks
        pose, lists = mean[:3].copy(), []
        for _ in range(STEPS):
            c, s = np.cos(pose[2]), np.sin(pose[2])
            pose = pose + [LIN * c, LIN * s, ANG]
            lms = rng.choice(MAPPED, M, replace=False)
            lists.append((lms.astype(np.int32),) + sight(pose, lms, 0.01))
        for K in COUNTS:
            seeds = mean[:3] + rng.multivariate_normal(np.zeros(3), SEED_COV, K)
            rows = [f"K = {K}"]
            with f.hypotheses(K) as bank:
                def reset():
                    bank.reset(seeds, SEED_COV)

                def unlabelled():
                    for _, r, b in lists:
                        bank.step_unlabelled(LIN, ANG, r, b, accept=ACCEPT, miss=miss)

                def labelled():
                    for i, r, b in lists:
                        bank.step(LIN, ANG, i, r, b)

                def host_route():
                    for _, r, b in lists[:hsteps]:
                        bank.step(LIN, ANG, [], [], [])
                        a = bank.associate(r, b)
                        idx, rr, bb = [], [], []
                        for k in range(K):
                            assign, _, _ = frontend.resolve_associations(a.cand[k], a.nis[k], a.min_nis[k], ACCEPT, np.inf)
                            keep = np.flatnonzero(assign >= 0)
                            idx.append(assign[keep].astype(np.int32))
                            rr.append(r[keep])
                            bb.append(b[keep])
                        bank.update(idx, rr, bb)
                        bank.sync()

                def one_device():
                    for _, r, b in lists[:hsteps]:
                        bank.step_unlabelled(LIN, ANG, r, b, accept=ACCEPT, miss=miss)
                        bank.sync()

                ta = clock(bank, reset, lambda: bank.associate(lists[0][1], lists[0][2]), reps)
                tk = []
                for _ in range(reps):
                    us = C.c_double()
                    dp = C.POINTER(C.c_double)
                    rc = lib.ekf_debug_hyp_score_time(bank._h, lists[0][1].ctypes.data_as(dp), lists[0][2].ctypes.data_as(dp), M, KERNEL_REPS, C.byref(us))
                    assert rc == 0, lib.ekf_hyp_last_error(bank._h)
                    tk.append(us.value)
                tu, tl = clock(bank, reset, unlabelled, reps), clock(bank, reset, labelled, reps)
                td, th = clock(bank, reset, one_device, reps), clock(bank, reset, host_route, reps)
                reset()
                bank.step_unlabelled(LIN, ANG, lists[0][1], lists[0][2], accept=ACCEPT, miss=miss)
                got = bank.assignments()
                right = float((got == lists[0][0][None, :]).mean())
                d, h = np.asarray(td) / hsteps, np.asarray(th) / hsteps
                faster = d.max() < h.min()
                rows += [f"    {'associate, call + sync':<52}{med(ta)}",
                         f"    {'k_hyp_score alone (event pair, per launch)':<52}{med(tk)}",
                         f"    {'step_unlabelled, 200 calls, one sync, per step':<52}{med(tu, STEPS)}",
                         f"    {'labelled step (true ids), 200 calls, one sync, per step':<52}{med(tl, STEPS)}",
                         f"    {'step_unlabelled + sync, per step':<52}{med(td, hsteps)}",
                         f"    {'host route of the guarantee + sync, per step':<52}{med(th, hsteps)}   host / device {np.median(h) / np.median(d):.1f}: "
                         f"the device route is {'faster by more than both spreads' if faster else 'NOT clearly faster (the spreads overlap)'}",
                         f"    (first step: {100.0 * right:.1f} % of the observations take their true landmark)"]
            for r in rows:
                print(r, flush=True)
            lines.extend(rows + [""])
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hyp_associate.txt"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    kept = ""                                                  # what the profile records once, below the table, stays
    if os.path.exists(args.out):
        old = open(args.out).read()
        kept = old[old.index(RECORDED):] if RECORDED in old else ""
    lines = run(args)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n" + kept)


if __name__ == "__main__":
    main()
