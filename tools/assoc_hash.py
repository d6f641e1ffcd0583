#!/usr/bin/env python3
"""A hash of EkfSlam.associate(full=True)'s six output arrays on fixed inputs: run it on two trees (two commits) and compare the
lines to see whether a change left ekf_associate's bits alone.  Three filters: N = 20 (the small-state path) and N = 70 and 200
on the general kernels, each after 12 steps of a synthetic stream WITHOUT a flush -- so the query folds pending ranks in -- and
once more behind a flush, and once with a per-trajectory noise table; 8 unlabelled observations (the stream's next step) per query.
  python3 tools/assoc_hash.py [--root TREE]        (TREE: the checkout whose package and library are loaded; default: this one)
Prints one line per query and one for all of them.  Nothing is checked here."""
import argparse
import hashlib
import os
import sys

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import slam_duckietown_amd as sd
    import slam_duckietown_amd.synthetic as syn
    sd.load_library()
    total = hashlib.sha256()
    for N in (20, 70, 200):
        steps, m = 12, 8
        mean0, diag0, lin, ang, idx, zr, zb = syn.synthetic_stream(N, steps + 1, m, 3)[:7]
        with sd.EkfSlam(3 + 2 * N, batch=1) as f:
            f.set_state_diag(mean0, diag0)
            for k in range(steps):
                f.step(lin[k], ang[k], idx[k], zr[k], zb[k])
            for what in ("pending", "flushed", "noise"):
                if what == "noise":                        # (the per-trajectory noise table: the other source of Q)
                    f.set_noise(motion_sigma=[0.05], meas_sigma=[0.4])
                a = f.associate(np.asarray(zr[steps])[None, :], np.asarray(zb[steps])[None, :], full=True)
                h = hashlib.sha256()
                for arr in (a.cand, a.nis, a.logdet, a.min_nis, a.all_nis, a.all_logdet):
                    h.update(np.ascontiguousarray(arr).tobytes())
                total.update(h.digest())
                print(f"N = {N:4d} {what:8s} {h.hexdigest()}  (best candidates {list(a.cand[0, :, 0])})")
                f.flush()
    print(f"all queries      {total.hexdigest()}")


if __name__ == "__main__":
    main()
