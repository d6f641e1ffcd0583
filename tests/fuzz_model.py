"""The oracle's view of a bank of trajectories under the whole filter surface, for tests/test_gpu_fuzz_features.py.

Test infrastructure only (oracle/ and tests/ helpers).  `Bank` mirrors what each EkfSlam call does to every trajectory:

* per-trajectory noise (`set_noise`): each trajectory predicts and updates under its own EkfConfig; None is the handle's
  config value, `set_noise()` the handle's constants; augmentation, `predict_dense` and the association gate ignore the table;
* the NIS gate, through tests/gated_oracle.py's `gated_update` / `gated_step`: every update leaves (idx, y, S, NIS,
  rejected) in application order, and a rejection leaves the state as it was;
* margin-safe gating: before an update op is issued, its observations are run on a copy; while some NIS lies within a factor
  of BAND of the threshold, the first such observation is dropped and the rest run again (the set shrinks, so this ends),
  so that rounding can never flip a decision.  The caller issues what is left;
* removal: np.delete on both axes, the tag -> index map renumbered (a removed tag seen again is a new landmark at the end);
* the innovation log's step rule (csrc/ekf_api.hip: a lone predict is no logged step; every update / step / step_state /
  step_detections call and every stream step is one, a window of more than 16 tags too; log_innovations(cap) restarts the
  count at 0);
* the reference's association (orc.associate + orc.augment) for step_detections windows, with the untagged landmarks of
  the map (set_state, add_landmarks) held by placeholder ids, as the library's host front end does.
"""
import dataclasses
import math

import numpy as np

from oracle import ekf_oracle as orc
from tests.gated_oracle import gated_step
from tests.gpu_support import tag

BAND = 4.0              # no NIS within a factor of BAND of the threshold


class Traj:
    """One trajectory: mean, covariance, its noise config, its tags and its rejections since the last set_nis_gate."""

    def __init__(self, mean, cov, base):
        self.mean, self.cov = np.array(mean, dtype=float), np.array(cov, dtype=float)
        self.base = base
        self.cfg = base
        self.tags = {}                                   # tag id -> landmark index (tagged landmarks only)
        self.seen = np.zeros(self.n_lm, dtype=bool)     # landmarks whose rows an update or a dense product has touched
        self.rejections = 0

    @property
    def n_lm(self):
        return (len(self.mean) - 3) // 2

    def set_noise(self, ms, qs):
        self.cfg = dataclasses.replace(self.base, motion_sigma=self.base.motion_sigma if ms is None else float(ms),
                                       meas_sigma=self.base.meas_sigma if qs is None else float(qs))

    def observed(self):
        return np.flatnonzero(self.seen)


def ambiguous(nis, g):
    """Index of the first NIS within a factor of BAND of the threshold g, or None."""
    if not math.isfinite(g):
        return None
    bad = np.flatnonzero((np.asarray(nis) > g / BAND) & (np.asarray(nis) < g * BAND))
    return int(bad[0]) if len(bad) else None


def safe_run(run, idx, zr, zb, g):
    """run(idx, zr, zb) -> (..., nis, rej) on copies, dropping the first ambiguous observation until none is left.
    -> (idx, zr, zb) kept, the last result, observations dropped."""
    idx, zr, zb = list(idx), list(zr), list(zb)
    dropped = 0
    while True:
        out = run(idx, zr, zb)
        j = ambiguous(out[-2], g)
        if j is None:
            return (idx, zr, zb), out, dropped
        del idx[j], zr[j], zb[j]
        dropped += 1


class Bank:
    """The model of one EkfSlam handle (every trajectory), fed the same calls."""

    def __init__(self, states, base=None):
        self.base = base or orc.EkfConfig()
        self.t = [Traj(m, P, self.base) for m, P in states]
        self.gate = math.inf
        self.log_cap, self.log_steps, self.log = 0, 0, {}
        self.dropped = 0

    # -- settings ------------------------------------------------------------------------------------------------------------
    def set_noise(self, ms=None, qs=None):
        """As EkfSlam.set_noise: scalars, (B,) arrays or None."""
        B = len(self.t)
        ms = None if ms is None else np.broadcast_to(np.asarray(ms, dtype=float), (B,))
        qs = None if qs is None else np.broadcast_to(np.asarray(qs, dtype=float), (B,))
        for b, tr in enumerate(self.t):
            tr.set_noise(None if ms is None else ms[b], None if qs is None else qs[b])

    def noise(self):
        return np.array([tr.cfg.motion_sigma for tr in self.t]), np.array([tr.cfg.meas_sigma for tr in self.t])

    def set_nis_gate(self, g):
        self.gate = math.inf if g is None else float(g)
        for tr in self.t:
            tr.rejections = 0

    def log_innovations(self, cap):
        self.log_cap, self.log_steps, self.log = int(cap), 0, {}

    def _logged(self, rows):
        """rows: per trajectory (idx, ys, Ss, nis, rej) of one logged step."""
        if self.log_cap:
            self.log[self.log_steps] = rows
            self.log.pop(self.log_steps - self.log_cap, None)
            self.log_steps += 1

    def ring(self):
        """{step number: rows} of the steps the ring still holds."""
        return dict(self.log)

    # -- the filter ----------------------------------------------------------------------------------------------------------
    def _apply(self, tr, idx, out):
        tr.mean, tr.cov = out[0], out[1]
        tr.rejections += int(np.sum(out[5]))
        if len(idx):
            tr.seen[np.asarray(idx, dtype=int)] = True
        return (np.asarray(idx, dtype=np.int64), out[2], out[3], out[4], out[5])

    def step(self, lin, ang, obs, predict=True, logged=True):
        """predict (if `predict`) + gated update of every trajectory; obs: per trajectory (idx, zr, zb).  Returns the
        observations kept by the margin filter (what the filter is to be given)."""
        kept, rows = [], []
        for b, tr in enumerate(self.t):
            def run(i, r, z, tr=tr, b=b):
                return gated_step(tr.mean, tr.cov, lin[b], ang[b], i, r, z, tr.cfg, self.gate, predict=predict)
            o, out, d = safe_run(run, *obs[b], self.gate)
            self.dropped += d
            kept.append(o)
            rows.append(self._apply(tr, o[0], out))
        if logged:
            self._logged(rows)
        return kept

    def update(self, obs):
        return self.step(np.zeros(len(self.t)), np.zeros(len(self.t)), obs, predict=False)

    def predict(self, lin, ang):
        for b, tr in enumerate(self.t):
            tr.mean, tr.cov = gated_step(tr.mean, tr.cov, lin[b], ang[b], [], [], [], tr.cfg, self.gate)[:2]

    def predict_dense(self, F, Q, b):
        tr = self.t[b]
        P = F @ tr.cov @ F.T + Q
        tr.cov = np.triu(P) + np.triu(P, 1).T                # (the device keeps the upper triangle)
        tr.seen[:] = True

    def grow(self, xy, b):
        tr = self.t[b]
        k, n = len(xy), len(tr.mean)
        tr.mean = np.concatenate([tr.mean, np.asarray(xy, dtype=float).reshape(-1)])
        cov = np.zeros((n + 2 * k, n + 2 * k))
        cov[:n, :n] = tr.cov
        cov[np.arange(n, n + 2 * k), np.arange(n, n + 2 * k)] = self.base.landmark_init_var
        tr.cov = cov
        tr.seen = np.concatenate([tr.seen, np.zeros(k, dtype=bool)])

    def remove(self, lms, b):
        """remove_landmarks(lms, b) (b None: every trajectory).  -> old_to_new of the (first) trajectory touched."""
        o2n = None
        for t in (range(len(self.t)) if b is None else (b,)):
            tr = self.t[t]
            rows = np.array([3 + 2 * int(l) + e for l in sorted(lms) for e in (0, 1)], dtype=int)
            keep = np.ones(tr.n_lm, dtype=bool)
            keep[np.asarray(lms, dtype=int)] = False
            m = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
            tr.mean = np.delete(tr.mean, rows)
            tr.cov = np.delete(np.delete(tr.cov, rows, axis=0), rows, axis=1)
            tr.seen = tr.seen[keep]
            tr.tags = {tag: int(m[j]) for tag, j in tr.tags.items() if m[j] >= 0}
            o2n = m if o2n is None else o2n
        return o2n

    def window(self, lin, ang, wins):
        """step_detections: per trajectory the reference's association (placeholders for untagged landmarks), augmentation
        (the handle's config), then a gated step under the trajectory's noise, in association order.  The margin filter
        drops the tags (all their detections) of ambiguous updates.  Returns (windows kept, per trajectory the update
        order)."""
        kept, orders, rows = [], [], []
        for b, (tr, win) in enumerate(zip(self.t, wins)):
            while True:
                index = dict(tr.tags)
                for j in range(tr.n_lm):
                    if j not in tr.tags.values():
                        index[-1 - j] = j
                tags = orc.associate(win, index, tr.mean, self.base)
                mean, cov = orc.augment(tr.mean, tr.cov, len(index), tags, self.base)
                order = list(tags.keys())
                out = gated_step(mean, cov, lin[b], ang[b], order, [tags[i][4] for i in order], [tags[i][5] for i in order],
                                 tr.cfg, self.gate)
                j = ambiguous(out[4], self.gate)
                if j is None:
                    break
                gone = tags[order[j]][3]
                win = [(ts, [tg for tg in tl if tg.tag_id != gone]) for ts, tl in win]
                self.dropped += 1
            grown = (len(mean) - len(tr.mean)) // 2
            tr.seen = np.concatenate([tr.seen, np.zeros(grown, dtype=bool)])
            tr.tags = {t: j for t, j in index.items() if t >= 0}
            rows.append(self._apply(tr, order, out))
            kept.append(win)
            orders.append((order, tags))
        self._logged(rows)
        return kept, orders


def window_of(rng, tr, ids, new_xz, frames, jitter=0.004):
    """A detection window of trajectory `tr` seeing tags `ids`: known tags where the model places them (seen from the model's
    pose; those outside the 1.5 m gate are left out), new ones at camera-frame (x, z) new_xz[tag]; `frames` frames."""
    c, s = math.cos(tr.mean[2]), math.sin(tr.mean[2])
    pos = {}
    for i in ids:
        if i in tr.tags:
            j = tr.tags[i]
            d = tr.mean[3 + 2 * j:5 + 2 * j] - tr.mean[0:2]
            xr, yr = c * d[0] + s * d[1], -s * d[0] + c * d[1]
            if xr * xr + yr * yr > 1.4 ** 2:
                continue
            pos[i] = (-yr, xr)
        else:
            pos[i] = new_xz[i]
    return [(0.1 * fr, [tag(i, x + rng.normal(0, jitter), z + rng.normal(0, jitter)) for i, (x, z) in pos.items()])
            for fr in range(frames)]
