"""The kidnapped-robot scenario of the hypothesis bank and its CPU model: a fleet of pose hypotheses on one frozen map, each run
through tests/localize_model.literal_step, with the log-likelihood the device accumulates formed from the model's own
innovations.  NumPy and the oracle only; a plain module the CPU and GPU tests import.

The scenario (`kidnapped_case`): an N = 20 map from 30 SLAM steps (`streams.wandering`, one trajectory), a robot put down at a
pose the filter knows nothing about, ONE range/bearing sighting of a mapped landmark, K = 64 hypotheses on the circle that
sighting allows (`frontend.poses_on_circle`, headings 2 pi / 64 apart), then six steps of four landmarks each, the same
observations for every hypothesis.  Seed and noise were chosen here, on the CPU, with margin: the model fleet ends with the
hypothesis seeded next to the truth on top, its pose NEES <= 8 (the GPU test's bar is chi2_3(0.999) = 16.27) and the runner-up's
weight <= 1e-3 (the GPU test asks for a ratio below 1 - 0.99), so the device can only fail that test for its own reasons."""
import dataclasses
from types import SimpleNamespace as NS

import numpy as np

from oracle import ekf_oracle as orc
from slam_duckietown_amd import frontend
from tests import localize_model as lm
from tests import streams

N, SLAM_STEPS, K, STEPS, M = 20, 30, 64, 6, 4
MOTION_SIGMA, MEAS_SIGMA = 0.01, 0.05                      # the filter's constants, for the map's SLAM steps and for the fleet
OBS_NOISE = 0.02                                           # what the robot's sensor really has (range and bearing)
SEED_COV = np.diag([0.03 ** 2, 0.03 ** 2, 0.015 ** 2])      # a hypothesis's pose block at its seed
TRUE_POSE = np.array([0.35, -0.25, -np.pi + 2.0 * np.pi * 41 / K + 0.004])   # 0.004 rad off seed 41's heading
SIGHTED = 3                                                # the landmark of the first sighting
NEES_BAR, RUNNER_UP_BAR = 8.0, 1e-3
CHI2_3_999 = 16.27


def model_cfg():
    return dataclasses.replace(orc.EkfConfig(), motion_sigma=MOTION_SIGMA, meas_sigma=MEAS_SIGMA)


def wrap(a):
    return (a + np.pi) % (2.0 * np.pi) - np.pi


def sight(pose, landmarks_xy, rng, noise):
    d = np.atleast_2d(landmarks_xy) - pose[:2]
    zr = np.hypot(d[:, 0], d[:, 1]) + rng.normal(0.0, noise, len(d))
    zb = wrap(np.arctan2(d[:, 1], d[:, 0]) - pose[2] + rng.normal(0.0, noise, len(d)))
    return zr, zb


def slam_stream(seed=11):
    """The mapping run: (world landmarks (N, 2), mean0, diag0, lin, ang, idx, zr, zb, m) for one trajectory."""
    mean0, lin, ang, idx, zr, zb, m = streams.wandering(N, 1, SLAM_STEPS, 8, seed)
    world = orc.synthetic_world(N, seed + 1)
    diag0 = world[3].copy()
    diag0[:3] = 1e-6                                       # the mapping run starts at a known pose: the map's frame is pinned
    return world[1], mean0[0], diag0, lin, ang, idx, zr, zb, m


def kidnapped_case(map_mean):
    """Everything the scenario fixes beside the map's covariance: the seeds from one sighting of landmark SIGHTED as the MAP
    places it (`map_mean`: the filter's mean after the mapping run), and the six steps' motion and shared observations as the
    true robot sees the true landmarks."""
    world = slam_stream()[0]
    rng = np.random.default_rng(77)
    zr0, zb0 = sight(TRUE_POSE, world[SIGHTED], rng, OBS_NOISE)
    seeds = frontend.poses_on_circle(np.asarray(map_mean)[3 + 2 * SIGHTED:5 + 2 * SIGHTED], zr0[0], zb0[0], K)
    cfg = model_cfg()
    pose, steps = TRUE_POSE.copy(), []
    for k in range(STEPS):
        lin, ang = 0.004, 0.02
        pose, _ = orc.motion_model(pose, lin, ang, cfg)
        vis = (4 * k + np.arange(M) * 5) % N
        zr, zb = sight(pose, world[vis], rng, OBS_NOISE)
        steps.append((lin, ang, vis.astype(np.int32), zr, zb))
    return NS(seeds=seeds, steps=steps, truth=pose, spacing=2.0 * np.pi / K)


def model_map():
    """The map as the oracle's dense filter leaves it after the mapping run (the device's agrees to 1e-9)."""
    _, mean, diag0, lin, ang, idx, zr, zb, m = slam_stream()
    cfg = model_cfg()
    mean, cov = mean.copy(), np.diag(diag0)
    for k in range(SLAM_STEPS):
        mk = int(m[k, 0])
        mean, cov = orc.ekf_step_dense(mean, cov, lin[k, 0], ang[k, 0], idx[k, 0, :mk], zr[k, 0, :mk], zb[k, 0, :mk], cfg)
    return mean, 0.5 * (cov + cov.T)


def loglik_of(log):
    """The sum the device accumulates, from literal_step's log records (index, y, S, NIS, rejected)."""
    return float(sum(-0.5 * (nis + np.log(np.linalg.det(S)) + 2.0 * np.log(2.0 * np.pi)) for _, _, S, nis, _ in log))


def reset_state(mean, cov, pose, block):
    """`reset_pose` on a dense state: the pose and its block replaced, every pose-landmark cross term dropped."""
    mean, cov = np.array(mean, dtype=float), np.array(cov, dtype=float)
    mean[:3] = pose
    cov[:3, :] = 0.0
    cov[:, :3] = 0.0
    cov[:3, :3] = block
    return mean, cov


def run_fleet(map_mean, map_cov, case, gate=None):
    """The fleet through the dense model: (poses (K, 3), blocks (K, 3, 3), loglik (K,))."""
    cfg = model_cfg()
    poses, blocks, ll = np.empty((K, 3)), np.empty((K, 3, 3)), np.zeros(K)
    for k in range(K):
        mean, cov = reset_state(map_mean, map_cov, case.seeds[k], SEED_COV)
        for lin, ang, idx, zr, zb in case.steps:
            log = []
            mean, cov = lm.literal_step(mean, cov, lin, ang, idx, zr, zb, cfg, gate=gate, log=log)
            ll[k] += loglik_of(log)
        poses[k], blocks[k] = mean[:3], cov[:3, :3]
    return poses, blocks, ll


def pose_nees(pose, block, truth):
    e = np.asarray(pose) - np.asarray(truth)
    e[2] = wrap(e[2])
    return float(e @ np.linalg.solve(block, e))


def heading_gap(seed_heading, truth_heading_at_seed=TRUE_POSE[2]):
    return abs(float(wrap(seed_heading - truth_heading_at_seed)))
