#!/usr/bin/env python3
"""Cost of EkfSlam.join (ekf_join_maps; k_join, csrc/ekf_join.hip) against the route without it: state() of both filters, the
dense NumPy product J P J^T (tests/join_model.py: join_dense) and set_state().

Settings: 32 pairs N_A = 1500 + N_B = 500 between two handles; 1 pair 1900 + 100; 256 pairs 10 + 8 on the small-state path;
1 pair 2030 + 40 into n_max = 4203 (the appended columns straddle the column-panel boundary at 4096).  Sequential mode.
Per setting real states (diagonal start, a few stream steps); before every timed call the destinations are restored from a
parked copy (copy_from), what is pending is flushed and the stream drained, so the join alone is timed: HIP events on the
destination handle's stream around the CALL (its flag read-backs, table upload, the snapshot and the join launch, the size
upload and its synchronisations), the median of `--reps` repetitions after `--warm` warm ones.  The kernels alone: the same
repetitions again under ekf_set_option("profile_kernels", 1), class 6 of ekf_profile_read_class (the snapshot launch and
k_join between one event pair).  Bytes moved = 8 x (entries written + the source's stored triangle + the pose rows read and
snapshotted); the yardsticks are the fork's 4.8 TB/s (profiles/copy_trajectories.txt) and the part's 6.29 TB/s copy rate.
Writes its report to stdout (profiles/join.txt)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORK_RATE = 4.8e12
COPY_RATE = 6.29e12


def prepared(sd, orc, N, n_max, B, steps=6, seed=0):
    mean0, diag0, lin, ang, idx, zr, zb = orc.synthetic_stream(N, steps, 8, seed)
    rep = lambda a: np.repeat(a[:, None], B, 1)
    f = sd.EkfSlam(n_max, batch=B)
    for b in range(B):
        f.set_state_diag(mean0 + 0.01 * b, diag0, b)
    f.run_stream(rep(lin), rep(ang), rep(idx), rep(zr), rep(zb))
    f.flush()
    f.sync()
    return f


def moved_bytes(NA, NB, pairs):
    nA, n = 3 + 2 * NA, 3 + 2 * (NA + NB)
    nB = 3 + 2 * NB
    written = n * (n + 1) // 2 - nA * (nA + 1) // 2 + 3 * nA
    return 8.0 * pairs * (written + nB * (nB + 1) // 2 + 2 * 3 * nA)


def timed(dst, src, spare, pairs, warm, reps, profile):
    every = np.arange(pairs)
    call_ms, kern_ms = [], []
    if profile:
        dst.set_option("profile_kernels", 1)
        dst.profile_enable(True)
    for i in range(warm + reps):
        dst.copy_from(spare, every, every)
        dst.flush()
        dst.sync()
        if profile:
            dst.profile_read()                                      # (resets the event pool)
        dst.timer_begin()
        dst.join(src, every, every)
        t = dst.timer_end()
        if profile:
            ms, cnt = dst.profile_read_class(6)
            assert cnt == 1, cnt
            t = ms
        if i >= warm:
            (kern_ms if profile else call_ms).append(t)
    if profile:
        dst.profile_enable(False)
        dst.set_option("profile_kernels", 0)
    ms = kern_ms if profile else call_ms
    return float(np.median(ms)), float(min(ms))


def host_route(jm, dst, src, spare, reps):
    """One pair through the host: state() of both, the dense product, set_state(): wall time."""
    ms = []
    for _ in range(reps):
        dst.copy_from(spare, 0, 0)
        dst.sync()
        t0 = time.perf_counter()
        xA, PA = dst.state(0)
        xB, PB = src.state(0)
        x, P = jm.join_dense(xA, PA, xB, PB, with_bound=False)[:2]
        dst.set_state(x, P, 0)
        ms.append(1e3 * (time.perf_counter() - t0))
        del xA, PA, xB, PB, x, P
    return float(np.median(ms))


def setting(sd, orc, jm, name, NA, NB, n_max, pairs, a, host_reps):
    dst = prepared(sd, orc, NA, n_max, pairs, seed=1)
    src = prepared(sd, orc, NB, 3 + 2 * NB, pairs, seed=2)
    spare = sd.EkfSlam(n_max, batch=pairs)
    every = np.arange(pairs)
    spare.copy_from(dst, every, every)
    gb = moved_bytes(NA, NB, pairs)
    med, lo = timed(dst, src, spare, pairs, a.warm, a.reps, False)
    kmed, klo = timed(dst, src, spare, pairs, a.warm, a.reps, True)
    small = sd.load_library().ekf_debug_small_launches(dst._h) > 0
    print(f"{name:40s} moved {gb / 1e9:7.4f} GB  call median {med:8.3f} ms (min {lo:.3f})  kernels (class 6) {kmed:8.3f} ms "
          f"(min {klo:.3f})  {gb / (kmed * 1e-3) / 1e12:5.2f} TB/s = {gb / (kmed * 1e-3) / FORK_RATE:4.2f} of the fork's 4.8 TB/s, "
          f"{gb / (kmed * 1e-3) / COPY_RATE:4.2f} of the 6.29 TB/s copy rate{'  [small-state path]' if small else ''}", flush=True)
    if host_reps:
        host = host_route(jm, dst, src, spare, host_reps)
        print(f"{'  state() x 2 + NumPy J P J^T + set_state(), ONE pair':40s} wall median {host:9.1f} ms: per pair the join is "
              f"{host / (med / pairs):.0f} x faster", flush=True)
    for f in (dst, src, spare):
        f.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settings", default="1,2,3,4")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=1)
    a = ap.parse_args()
    import slam_duckietown_amd as sd
    from oracle import ekf_oracle as orc
    from tests import join_model as jm
    which = [int(x) for x in a.settings.split(",")]
    if 1 in which:
        setting(sd, orc, jm, "32 pairs N_A=1500 + N_B=500", 1500, 500, 3 + 2 * 2000, 32, a, a.host_reps)
    if 2 in which:
        setting(sd, orc, jm, "1 pair 1900 + 100", 1900, 100, 3 + 2 * 2000, 1, a, a.host_reps)
    if 3 in which:
        setting(sd, orc, jm, "256 pairs 10 + 8 (small-state path)", 10, 8, 3 + 2 * 18, 256, a, a.host_reps)
    if 4 in which:
        setting(sd, orc, jm, "1 pair 2030 + 40, n_max = 4203 (panels)", 2030, 40, 4203, 1, a, a.host_reps)


if __name__ == "__main__":
    main()
