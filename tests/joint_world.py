"""Shared by the joint-covariance tests (tests/test_joint_cpu.py, tests/test_gpu_joint.py): the scenario individual
compatibility gets wrong, built on the dense oracle, and the candidate lists joint compatibility starts from.

The scenario: ARC_N landmarks on an arc of radius ARC_R around the robot, ARC_S apart.  A tight, correlated map is built by
MAP_STEPS oracle steps that observe every landmark with small noise; then one prediction with a large motion noise makes the
pose loose (heading sigma LOOSE / 2 = 0.15 rad: at the landmarks' range about one spacing, ARC_S / ARC_R = 0.15 rad), while
the landmark and measurement sigmas (a few centimetres) stay small against ARC_S = 0.6.  The observations are of all ARC_N
landmarks, from a pose drawn from the predicted pose covariance.  Seen alone, every observation fits the neighbour of its
landmark as well as the landmark itself; jointly they cannot all be shifted, because the row ends.
"""
import numpy as np

from oracle import ekf_oracle as orc

ARC_N, ARC_R, ARC_S = 6, 4.0, 0.6
MAP_STEPS = 3
TIGHT, LOOSE, MEAS = 0.01, 0.3, 0.03      # motion sigma while mapping, motion sigma of the last prediction, measurement sigma
LIN, ANG = 0.004, 0.0
# Seeds of the pose draw / measurement noise.  Chosen on the CPU with the oracle so that for each of them greedy individual
# compatibility (frontend.resolve_associations on the reference scores) returns at least one wrong landmark AND
# joint_compatibility returns no wrong one and at least m - 1 right ones; a seed that does not satisfy both is replaced,
# never the assertion.
SEEDS = (0, 2, 3, 4, 9, 25)


def cfg_map():
    return orc.EkfConfig(motion_sigma=TIGHT, meas_sigma=MEAS)


def cfg_loose():
    return orc.EkfConfig(motion_sigma=LOOSE, meas_sigma=MEAS)


def observe(pose, lm, rng, sigma):
    d = lm - pose[:2]
    r = np.hypot(d[:, 0], d[:, 1]) + rng.normal(0.0, sigma, len(lm))
    b = orc.wrap_pi(np.arctan2(d[:, 1], d[:, 0]) - pose[2] + rng.normal(0.0, sigma, len(lm)))
    return r, b


def make_scenario(seed):
    """dict(mean0, P0: the state BEFORE the last prediction (tight pose, tight correlated map); lin, ang: that prediction's
    inputs; mean, P: the state after it (loose pose); zr, zb: the observations; truth (m,): the landmark of each)."""
    rng = np.random.default_rng(4000 + seed)
    ang = (np.arange(ARC_N) - (ARC_N - 1) / 2.0) * (ARC_S / ARC_R)
    lm = ARC_R * np.stack([np.cos(ang), np.sin(ang)], -1)
    n = 3 + 2 * ARC_N
    mean = np.concatenate([np.zeros(3), (lm + rng.normal(0.0, 0.03, lm.shape)).ravel()])
    P = np.diag(np.concatenate([np.full(3, 1e-4), np.full(n - 3, 0.05 ** 2)]))
    pose = np.zeros(3)
    for _ in range(MAP_STEPS):
        pose, _ = orc.motion_model(pose, LIN, ANG, cfg_map())
        zr, zb = observe(pose, lm, rng, MEAS)
        mean, P = orc.ekf_step_dense(mean, P, LIN, ANG, np.arange(ARC_N), zr, zb, cfg_map())
    mean0, P0 = mean.copy(), P.copy()
    mean, P = orc.predict_dense(mean0, P0, LIN, ANG, cfg_loose())
    P = (P + P.T) / 2
    pose, _ = orc.motion_model(pose, LIN, ANG, cfg_loose())
    pose = pose + np.linalg.cholesky(P[:3, :3]) @ rng.normal(size=3)      # a pose drawn from the predicted covariance
    zr, zb = observe(pose, lm, rng, MEAS)
    return dict(mean0=mean0, P0=(P0 + P0.T) / 2, lin=LIN, ang=ANG, mean=mean, P=P, zr=zr, zb=zb, truth=np.arange(ARC_N))


def candidate_lists(cand, cnis, accept):
    """Per observation its (at most two) candidates with NIS <= accept, in ascending order of NIS, and their sorted union."""
    lists = []
    for q in range(len(cand)):
        ok = [(float(cnis[q, c]), int(cand[q, c])) for c in range(2) if cand[q, c] >= 0 and cnis[q, c] <= accept]
        lists.append([j for _, j in sorted(ok)])
    return lists, sorted({j for c in lists for j in c})
