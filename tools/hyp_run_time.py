#!/usr/bin/env python3
"""HypothesisBank.run() -- an uploaded stream with the resampling decided on the device -- against the host loop it replaces,
`step` + `resample_if(0.5, split=0.5)` per step, at N = 2000, m = 8 shared observations, 200 steps, for K = 32, 1024 and 4096
hypotheses seeded around the map's pose.  Microseconds per step, clocked on the host from the first call to the end of the bank's
sync, medians over `--reps` repetitions with the spread (min .. max); every repetition starts from the same reset bank and uses the
same offsets u and draws z.  Both with the log off and with the log on (the host loop then also reads `mixture()` per step, which is
what the log replaces).  `run` includes what the binding does per call: it stages all 200 x K x 3 draws at once.
Beside them:
  run, no resampling      fraction 0, log off: the two step launches per step and nothing else, back to back;
  steps alone             200 `step` calls and one sync: ekf_hyp_step's rate when the host does not wait;
  gate closed             run with a fraction so small that the gate never opens: k_hyp_weigh and the three launches that
                          leave at once on top of a step -- against `run, no resampling`;
  weigh + mixture         run with fraction 0 and the log on against the log off: k_hyp_weigh + k_hyp_mixture per step;
  k_hyp_mixture alone     the blocking `mixture()` against the blocking `ess()`, which differ by that one launch.
  python3 tools/hyp_run_time.py [--reps 5] [--out profiles/hyp_run.txt] [--gaps pytest-output]
--gaps appends the "largest gap" lines of `pytest tests/test_gpu_hyp_run.py -s` (the mixture against the longdouble model).
Nothing is checked here, only timed."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, M, STEPS, COUNTS, FRACTION, SPLIT = 2000, 8, 200, (32, 1024, 4096), 0.5, 0.5
SEED_COV = np.diag([0.02, 0.02, 0.005])


def med(xs):
    xs = np.asarray(xs) / STEPS
    return f"{np.median(xs):9.1f} ({np.min(xs):.1f} .. {np.max(xs):.1f})"


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
    import slam_duckietown_amd.synthetic as syn
    n, W, reps = 3 + 2 * N, args.warm, args.reps
    lines = ["HypothesisBank.run() against step + resample_if: microseconds PER STEP, median (min .. max)",
             f"(tools/hyp_run_time.py; N = {N}, m = {M} shared, {STEPS} steps, {reps} repetitions behind {W} SLAM steps and a flush; "
             f"fraction {FRACTION}, split {SPLIT})", ""]
    s = syn.synthetic_stream(N, W + STEPS, M, 0)
    rng = np.random.default_rng(1)
    with sd.EkfSlam(n, batch=1) as f:
        f.set_option("active_bound", 0)
        f.set_state_diag(s[0], s[1])
        f.stream_upload(*(np.asarray(s[i])[:, None] for i in (2, 3, 4, 5, 6)))
        f.stream_run(0, W)
        f.flush()
        f.sync()
        mean = f.mean(0)
        stream = [tuple(s[i][W + k] for i in (2, 3, 4, 5, 6)) for k in range(STEPS)]
        for K in COUNTS:
            seeds = mean[:3] + rng.multivariate_normal(np.zeros(3), 4.0 * SEED_COV, K)
            u, z = rng.random(STEPS), rng.standard_normal((STEPS, K, 3))
            rows = [f"K = {K}"]
            with f.hypotheses(K) as bank:
                bank.upload_stream(*[[st[i] for st in stream] for i in range(5)])
                fired = [0]

                def reset():
                    bank.reset(seeds, SEED_COV)

                def host_loop(log):
                    def work():
                        fired[0] = 0
                        for k in range(STEPS):
                            bank.step(*stream[k])
                            if log:
                                bank.mixture()
                            fired[0] += bank.resample_if(FRACTION, u=u[k], split=SPLIT, z=z[k]) is not None
                    return work

                def steps_alone():
                    for k in range(STEPS):
                        bank.step(*stream[k])
                for log in (False, True):
                    bank.log(STEPS if log else 0)
                    name = "log on" if log else "log off"
                    th = clock(bank, reset, host_loop(log), reps)
                    tr = clock(bank, reset, lambda: bank.run(0, STEPS, fraction=FRACTION, split=SPLIT, u=u, z=z), reps)
                    did = int(bank.trace().resampled.sum()) if log else fired[0]
                    rows += [f"    {name + ': host loop (step + resample_if' + (' + mixture)' if log else ')'):<48}{med(th)}   resampled at {fired[0]} steps",
                             f"    {name + ': run':<48}{med(tr)}   resampled at {did} steps   host loop / run {np.median(th) / np.median(tr):.2f}"]
                bank.log(0)
                t0 = clock(bank, reset, lambda: bank.run(0, STEPS, fraction=0.0), reps)
                ts = clock(bank, reset, steps_alone, reps)
                tg = clock(bank, reset, lambda: bank.run(0, STEPS, fraction=1e-12, u=u), reps)
                bank.log(STEPS)
                tl = clock(bank, reset, lambda: bank.run(0, STEPS, fraction=0.0), reps)
                bank.log(0)
                rows += [f"    {'run, no resampling (log off)':<48}{med(t0)}",
                         f"    {'steps alone: 200 step calls, one sync':<48}{med(ts)}",
                         f"    {'gate closed: run, fraction 1e-12 (log off)':<48}{med(tg)}   over run, no resampling: "
                         f"{(np.median(tg) - np.median(t0)) / STEPS:+.1f} (k_hyp_weigh and three launches that leave at once)",
                         f"    {'run, no resampling, log on':<48}{med(tl)}   over the log off: {(np.median(tl) - np.median(t0)) / STEPS:+.1f} "
                         "(k_hyp_weigh + k_hyp_mixture)"]
                reset()
                bank.run(0, 20, fraction=0.0)
                bank.sync()
                tm, te = [], []
                for _ in range(10 * reps):
                    t1 = time.perf_counter()
                    bank.mixture()
                    t2 = time.perf_counter()
                    bank.ess()
                    t3 = time.perf_counter()
                    tm.append((t2 - t1) * 1e6), te.append((t3 - t2) * 1e6)
                rows.append(f"    {'blocking mixture() / ess(), per call':<48}{np.median(tm):9.1f} / {np.median(te):.1f}   k_hyp_mixture alone: "
                            f"{np.median(tm) - np.median(te):+.1f}")
            for r in rows:
                print(r, flush=True)
            lines.extend(rows + [""])
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hyp_run.txt"))
    ap.add_argument("--gaps", default=None, help="append the model gaps from this output of pytest tests/test_gpu_hyp_run.py -s to --out")
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.gaps:
        found = [ln.strip().lstrip(".") for ln in open(args.gaps) if "the mixture against the model, largest gap" in ln]
        with open(args.out, "a") as fh:
            fh.write("\n".join(["The mixture against tests/hyp_run_model.py in longdouble (tests/test_gpu_hyp_run.py -s; mean, covariance, ess "
                                "and evidence, rel = |got - want| / max(1, |want|)):"] + ["    " + ln for ln in found]) + "\n")
        return
    lines = run(args)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
