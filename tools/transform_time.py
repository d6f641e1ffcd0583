#!/usr/bin/env python3
"""Cost of EkfSlam.transform (ekf_transform; k_transform, csrc/ekf_transform.hip) against the routes without it:
(a) the host route -- state(), the NumPy congruence of tests/transform_model.py, set_state() -- for ONE trajectory;
(b) joining the map into an empty second handle through the frame (join(transform=, cov=)), which needs a second allocation of
    the full triangle and drops the pose with its correlations;
(c) for the same bytes, the fork's rate (profiles/copy_trajectories.txt: 4.8 TB/s on the 32-trajectory bank) and the part's
    measured 6.29 TB/s copy rate.

Settings: 32 x N = 2000, 1 x N = 2000, 1 x N = 8000 (column panels), 256 x N = 20 (small-state path); each with and without a
frame covariance.  Per setting real states (diagonal start, a few stream steps), then one transform WITH a covariance so that
every trajectory is fully correlated and its active bound is its size: the call without a covariance then also walks the whole
stored triangle.  Timed: HIP events on the handle's stream around the CALL (flag read-back, the pending flush -- nothing is
pending --, table and frame uploads, the copy of the means, the launch, the synchronisations), the median of `--reps`
repetitions after `--warm` warm ones; the kernel alone: the same repetitions again under ekf_set_option("profile_kernels", 1),
class 8 of ekf_profile_read_class; on the 32-trajectory bank also with plain stores (EKFSLAM_HIP_TRANSFORM_NT=0, read per call)
against the nontemporal ones the library uses.  The transform is applied again and again to the same bank (a rigid motion each time).
Bytes moved = trajectories x 2 x 8 n (n + 1) / 2 (the stored triangle read and written once).
Writes its report to stdout (profiles/transform.txt)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORK_RATE = 4.8e12
COPY_RATE = 6.29e12
T = np.array([5.0, -3.0, 1.0])
COV = np.array([[0.04, 0.01, -0.002], [0.01, 0.09, 0.003], [-0.002, 0.003, 0.002]])


def prepared(sd, orc, N, B, steps=6, seed=0):
    mean0, diag0, lin, ang, idx, zr, zb = orc.synthetic_stream(N, steps, 8, seed)
    rep = lambda a: np.repeat(a[:, None], B, 1)
    f = sd.EkfSlam(3 + 2 * N, batch=B)
    for b in range(B):
        f.set_state_diag(mean0 + 0.01 * b, diag0, b)
    f.run_stream(rep(lin), rep(ang), rep(idx), rep(zr), rep(zb))
    f.transform(T, COV)                                            # fully correlated: the bound is the size
    f.sync()
    return f


def timed(f, cov, warm, reps, profile):
    out = []
    if profile:
        f.set_option("profile_kernels", 1)
        f.profile_enable(True)
    for i in range(warm + reps):
        f.sync()
        if profile:
            f.profile_read()                                        # (resets the event pool)
        f.timer_begin()
        f.transform(T, cov)
        t = f.timer_end()
        if profile:
            ms, cnt = f.profile_read_class(8)
            assert cnt == 1, cnt
            t = ms
        if i >= warm:
            out.append(t)
    if profile:
        f.profile_enable(False)
        f.set_option("profile_kernels", 0)
    return float(np.median(out)), float(min(out))


def host_route(tm, f, cov, reps):
    """One trajectory through the host: state(), the congruence, set_state(): wall time."""
    ms = []
    for _ in range(reps):
        f.sync()
        t0 = time.perf_counter()
        x, P = f.state(0)
        R = tm.rot(T[2])
        Pn = tm._congruence(P, R)
        if cov is not None:
            A = tm.frame_rows(x, T)
            Pn += A @ cov @ A.T
        xn = x.copy()
        xn[:2] = T[:2] + R @ x[:2]
        xn[2] += T[2]
        xn[3:] = (T[:2] + x[3:].reshape(-1, 2) @ R.T).ravel()
        f.set_state(xn, Pn, 0)
        ms.append(1e3 * (time.perf_counter() - t0))
        del x, P, Pn
    return float(np.median(ms))


def join_route(sd, f, cov, reps):
    """One trajectory joined into an empty second handle through the frame: the call alone (the second handle's allocation,
    as large as the first, is not timed)."""
    ms = []
    with sd.EkfSlam(f.n_max) as other:
        for _ in range(reps + 1):
            other.set_state_diag(np.zeros(3), np.full(3, 0.1))
            other.sync()
            other.timer_begin()
            other.join(f, 0, 0, transform=T, cov=cov)
            ms.append(other.timer_end())
    return float(np.median(ms[1:]))


def setting(sd, orc, tm, name, N, B, a):
    f = prepared(sd, orc, N, B)
    n = 3 + 2 * N
    gb = B * 2 * 8.0 * n * (n + 1) / 2
    small = sd.load_library().ekf_debug_small_launches(f._h) > 0
    for cov, tag in ((None, "without cov"), (COV, "with cov   ")):
        med, lo = timed(f, cov, a.warm, a.reps, False)
        kmed, klo = timed(f, cov, a.warm, a.reps, True)
        rate = gb / (kmed * 1e-3)
        print(f"{name:22s} {tag} moved {gb / 1e9:7.4f} GB  call + sync median {med:8.3f} ms (min {lo:.3f})  kernel (class 8) "
              f"{kmed:8.3f} ms (min {klo:.3f})  {rate / 1e12:5.2f} TB/s = {rate / FORK_RATE:4.2f} of the fork's 4.8 TB/s (the fork "
              f"would take {gb / FORK_RATE * 1e3:.3f} ms for these bytes), {rate / COPY_RATE:4.2f} of the 6.29 TB/s copy rate"
              f"{'  [small-state path]' if small else ''}", flush=True)
        if a.stores and B > 1 and N >= 1000:                        # the store variants, in this process, on this bank
            os.environ["EKFSLAM_HIP_TRANSFORM_NT"] = "0"
            pmed, plo = timed(f, cov, a.warm, a.reps, True)
            os.environ["EKFSLAM_HIP_TRANSFORM_NT"] = "1"
            nmed, nlo = timed(f, cov, a.warm, a.reps, True)
            del os.environ["EKFSLAM_HIP_TRANSFORM_NT"]
            print(f"{'  stores: kernel with plain / nontemporal stores':60s} {pmed:8.3f} ms (min {plo:.3f}) / {nmed:8.3f} ms (min {nlo:.3f})",
                  flush=True)
        if a.host_reps:
            host = host_route(tm, f, cov, a.host_reps)
            print(f"{'  (a) state() + NumPy + set_state(), ONE trajectory':60s} wall median {host:9.1f} ms: per trajectory the call "
                  f"is {host / (med / B):.0f} x faster", flush=True)
        if a.join_reps:
            jn = join_route(sd, f, cov, a.join_reps)
            print(f"{'  (b) join into an empty second handle, ONE trajectory':60s} call median {jn:9.3f} ms "
                  f"(and a second allocation of {8.0 * n * n / 1e9:.2f} GB; the pose is dropped)", flush=True)
    f.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settings", default="1,2,3,4")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--join-reps", type=int, default=3)
    ap.add_argument("--stores", type=int, default=1, help="1: also time plain against nontemporal stores on the large bank")
    a = ap.parse_args()
    import slam_duckietown_amd as sd
    from oracle import ekf_oracle as orc
    from tests import transform_model as tm
    which = [int(x) for x in a.settings.split(",")]
    if 1 in which:
        setting(sd, orc, tm, "32 x N = 2000", 2000, 32, a)
    if 2 in which:
        setting(sd, orc, tm, "1 x N = 2000", 2000, 1, a)
    if 3 in which:
        setting(sd, orc, tm, "1 x N = 8000 (panels)", 8000, 1, a)
    if 4 in which:
        setting(sd, orc, tm, "256 x N = 20", 20, 256, a)


if __name__ == "__main__":
    main()
