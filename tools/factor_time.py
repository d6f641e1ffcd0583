#!/usr/bin/env python3
"""ekf_factor -- the Cholesky factor of the whole covariance, formed on the device -- against the host route that gives the
same factor, covariance(b) + np.linalg.cholesky per trajectory, at four settings:
  32 x N = 2000, 1 x N = 2000, 1 x N = 8000 (P_base in column panels) and 256 x N = 20.
Every trajectory starts from the synthetic stream's diagonal state and runs its first five steps, so P is a real EKF-SLAM
covariance; flush() before the clock starts, so the timed span holds a flush with nothing pending: no pass.  ekf_factor is timed with
ekf_timer_begin / ekf_timer_end (median of --reps), the host route with the host clock in the same run (--host-reps, NumPy on
the threads the environment gives it: OMP_NUM_THREADS).  Also: the achieved TFLOP/s at n^3 / 3 per trajectory, the time of
ekf_factor_solve for 1 and 16 right-hand sides (events around the call: upload, kernel and download), and -- at 1 x N = 2000
and 256 x N = 20 -- the measured ratios to the bounds tests/test_gpu_factor.py asserts.
  python3 tools/factor_time.py [--reps 5] [--host-reps 1] [--skip-8000] [--out profiles/factor.txt]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EPS = 2.0 ** -53
_dp = C.POINTER(C.c_double)


def gamma(k):
    return k * EPS / (1.0 - k * EPS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--skip-8000", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "factor.txt"))
    args = ap.parse_args()
    import slam_duckietown_amd as sd
    import slam_duckietown_amd.synthetic as syn
    lib = sd.load_library()
    lines = ["ekf_factor against covariance(b) + np.linalg.cholesky per trajectory (tools/factor_time.py)",
             f"device: events around ekf_factor, nothing pending, median of {args.reps} after one warm-up; host route: host clock, "
             f"median of {args.host_reps}, OMP_NUM_THREADS = {os.environ.get('OMP_NUM_THREADS', 'unset')}",
             "TFLOP/s at n^3 / 3 per trajectory (the dense product P <- F P F^T + Q reaches 56); solve: ekf_factor_solve, "
             "upload + kernel + download", ""]

    def emit(row):
        lines.append(row)
        print(row, flush=True)

    def timed(f, fn):
        f.timer_begin()
        fn()
        return f.timer_end()

    def setting(title, N, B, steps, check):
        n = 3 + 2 * N
        with sd.EkfSlam(n, batch=B) as f:
            first = syn.synthetic_stream(N, steps, 8, 0)    # (every trajectory runs the same stream: the same covariance B times)
            for b in range(B):
                f.set_state_diag(first[0], first[1], b)
            for k in range(steps):
                f.step(np.full(B, first[2][k]), np.full(B, first[3][k]), np.tile(first[4][k], (B, 1)), np.tile(first[5][k], (B, 1)),
                       np.tile(first[6][k], (B, 1)))
            f.flush()
            f.sync()
            fac = f.factor()
            assert (fac.info == 0).all(), fac.info
            t_dev = float(np.median([timed(f, lambda: lib.ekf_factor(f._h, 0, B, None, None)) for _ in range(args.reps)]))
            fac = f.factor()
            x = np.random.default_rng(0).standard_normal((B, 16, n))
            quad = np.empty((B, 16))
            t_solve = []
            for nrhs in (1, 16):
                part = np.ascontiguousarray(x[:, :nrhs])
                call = lambda: lib.ekf_factor_solve(f._h, 0, B, part.ctypes.data_as(_dp), nrhs, n, None, quad.ctypes.data_as(_dp))
                call()
                t_solve.append(float(np.median([timed(f, call) for _ in range(args.reps)])))
            ts = []
            for _ in range(args.host_reps):
                t0 = time.perf_counter()
                for b in range(B):
                    np.linalg.cholesky(f.covariance(b))
                ts.append((time.perf_counter() - t0) * 1e3)
            t_host = float(np.median(ts))
            tflops = B * n ** 3 / 3.0 / (t_dev * 1e-3) / 1e12
            emit(f"  {title:18s} n = {n:5d}  ekf_factor {t_dev:10.3f} ms  {tflops:6.2f} TFLOP/s   host route {t_host:11.1f} ms "
                 f"({t_host / t_dev:7.1f} x)   solve 1 rhs {t_solve[0]:8.3f} ms, 16 rhs {t_solve[1]:8.3f} ms")
            if check:
                P, U = f.covariance(0), fac.upper(0)
                ev = np.linalg.eigvalsh(P)
                kappa = ev[-1] / ev[0]
                res = np.linalg.norm(U.T @ U - P) / (gamma(n + 1) * np.linalg.norm(np.abs(U.T) @ np.abs(U)))
                dl = abs(fac.logdet[0] - 2.0 * np.log(np.diag(np.linalg.cholesky(P))).sum()) / (2 * n * gamma(n + 1) * kappa)
                q = fac.mahalanobis(x[:, :16])[0]
                qref = np.einsum("ki,ik->k", x[0], np.linalg.solve(P, x[0].T))
                rq = (np.abs(q - qref) / qref).max() / (10 * n * EPS * kappa)
                emit(f"  {'':18s} trajectory 0: kappa_2 = {kappa:.3g}; ratios to the tests' bounds: residual {res:.3g}, logdet {dl:.3g}, "
                     f"quad (16 rhs) {rq:.3g}")

    setting("32 x N = 2000", 2000, 32, 5, False)
    setting("1 x N = 2000", 2000, 1, 5, True)
    if args.skip_8000:
        emit("  1 x N = 8000       not measured yet")
    else:
        setting("1 x N = 8000", 8000, 1, 5, False)
    setting("256 x N = 20", 20, 256, 5, True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
