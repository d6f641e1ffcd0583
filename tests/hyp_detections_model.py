"""The CPU model of a hypothesis bank's window of raw detections (k_hyp_associate; HypothesisBank.step_detections /
upload_detections / tags / unmatched_tags) and the judge the GPU tests use on what the device reports, plus the kidnapped-robot
case both sides share.  NumPy, the oracle and the package's host front end only; a plain module the CPU and GPU tests import.

`walk` is the device's rule written out: frontend.associate_known's sums and arithmetic (its `_averaged`), with what the device
adds to it -- ids outside [0, 1024) dropped with EKF_FLAG_ASSOC, at most EKF_AMAX distinct matched tags, the surplus dropped with
the flag -- and three planted mistakes (`mutant`) the judge must catch."""
from types import SimpleNamespace as NS

import numpy as np

from slam_duckietown_amd import frontend
from tests import hypotheses_model as hm
from tests import loc_det_world as ldw
from tests import localize_model as lm

AMAX, TAGMAX, EKF_FLAG_ASSOC = 32, 1024, 2
TOL = 1e-12                                                # the project's bar for the device's association against frontend.associate_known
MUTANTS = ("an unknown tag given a slot", "per-tag averaging dropped", "the 33rd tag not dropped")


def walk(window, index, n_landmarks, gate_range=1.5, ignore_tags=(), mutant=None):
    """One window against a frozen map: ({landmark: (tag_id, err, range, bearing)} in update order, the distinct unmatched ids
    in order of first appearance, the window's flag)."""
    gate2, flag = gate_range ** 2, 0
    seen, unmatched = {}, []
    for _stamp, tags in window:
        for tag in tags:
            tid = int(tag.tag_id)
            if not 0 <= tid < TAGMAX:
                flag |= EKF_FLAG_ASSOC
                continue
            if tid in ignore_tags:
                continue
            tx, tz = float(tag.pose_t[0][0]), float(tag.pose_t[2][0])
            if tz * tz + tx * tx > gate2:
                continue
            lmk = index.get(tid)
            if lmk is None or lmk < 0 or lmk >= n_landmarks:
                if mutant == MUTANTS[0]:
                    lmk = tid % n_landmarks
                else:
                    if tid not in unmatched:
                        unmatched.append(tid)
                    continue
            acc = seen.get(lmk)
            if acc is None:
                if len(seen) >= AMAX and mutant != MUTANTS[2]:
                    flag |= EKF_FLAG_ASSOC
                    continue
                seen[lmk] = [tx, tz, [tag.pose_err], tid]
            elif mutant != MUTANTS[1]:
                acc[0] += tx
                acc[1] += tz
                acc[2].append(tag.pose_err)
    out = frontend._averaged(seen, np.zeros(3))
    return {int(k): (int(v[3]), float(v[2]), float(v[4]), float(v[5])) for k, v in out.items()}, unmatched, flag


def judge(got, want, tol=TOL):
    """What the device (or a mutant) reports for a window -- (tags, unmatched, flag) -- against the model's: None, or what is
    wrong.  Landmarks, their order, tag ids, unmatched ids and the flag exactly; err, range and bearing within `tol`."""
    (gt, gu, gf), (wt, wu, wf) = got, want
    if list(gt) != list(wt):
        return f"matched landmarks {list(gt)} where the model has {list(wt)}"
    if list(gu) != list(wu):
        return f"unmatched ids {list(gu)} where the model has {list(wu)}"
    if gf != wf:
        return f"flag {gf} where the model has {wf}"
    for k in wt:
        if gt[k][0] != wt[k][0]:
            return f"landmark {k}: tag id {gt[k][0]} where the model has {wt[k][0]}"
        gap = max(abs(gt[k][i] - wt[k][i]) for i in (1, 2, 3))
        if not gap <= tol:
            return f"landmark {k}: err / range / bearing gap {gap:.3e} above {tol:g}"
    return None


# ---- the kidnapped robot from a log: the CPU condition on the model fleet and the GPU run share it ----
RELOC_K = 32                                               # seeds on the circle of one sighting: headings 2 pi / 32 = 0.196 rad apart
RELOC_SEED_COV = np.diag([0.05 ** 2, 0.05 ** 2, 0.1 ** 2])  # one sigma of heading = half the seeds' spacing
RELOC_SIGHTED = 0


def reloc_case():
    """ldw.recovery_stream()'s map (the oracle's, mapped with the tuned filter) and localisation windows, and RELOC_K seeds from
    ONE noise-free sighting of landmark RELOC_SIGHTED at the pose where the robot is put down, placed by the MAP's landmark."""
    world, wins, reset_truth, loc = ldw.recovery_stream()
    cfg = lm.with_noise(ldw.CFG, **ldw.RECOVERY_NOISE)
    mean, cov, index = ldw.oracle_map(world, wins, cfg, ldw.RECOVERY_P0)
    j = index[world.ids[RELOC_SIGHTED]]
    d = world.xy[RELOC_SIGHTED] - reset_truth[:2]
    zr, zb = float(np.hypot(d[0], d[1])), float(hm.wrap(np.arctan2(d[1], d[0]) - reset_truth[2]))
    seeds = frontend.poses_on_circle(mean[3 + 2 * j:5 + 2 * j], zr, zb, RELOC_K)
    return NS(world=world, wins=wins, cfg=cfg, map=(mean, cov, index), seeds=seeds, loc=loc,
              steps=[(ldw.LIN, ldw.ANG, win) for win, _truth in loc], truth=loc[-1][1])


def reloc_fleet(case):
    """The fleet on the dense model, no resampling: per seed (mean, covariance, log-likelihood) behind the last window."""
    mean0, cov0, index = case.map
    out = []
    for seed in case.seeds:
        mean, cov = hm.reset_state(mean0, cov0, seed, RELOC_SEED_COV)
        ll = 0.0
        for win, _truth in case.loc:
            log = []
            (mean, cov), _tags, _un = ldw.model_window(mean, cov, index, win, cfg=case.cfg, log=log)
            ll += hm.loglik_of(log)
        out.append((mean, cov, ll))
    return out
