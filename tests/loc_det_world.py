"""A small world for localisation from raw detections (ekf_localize_detections; EkfSlam.localize_detections): tags on a ring
around the origin, all inside the 1.5 m gate of a robot that drives a slow arc near it, the windows a camera would hand over,
and the model of one localisation window -- frontend.associate_known on the window, then tests/localize_model.literal_step on
what it matched.  NumPy, the oracle and the package's host front end only; a plain module the CPU and GPU tests import."""
from types import SimpleNamespace as NS

import numpy as np

from oracle import ekf_oracle as orc
from slam_duckietown_amd import frontend
from tests import localize_model as lm

CFG = orc.EkfConfig()
LIN, ANG = 0.004, 0.02
CHI2_3_0999 = 16.266236196238129                       # the chi-square quantile of 3 degrees of freedom at 0.999


def det(i, x, z, err=1e-3):
    """A detection of tag i at (x, z) in the camera frame, as step_detections / localize_detections take them."""
    return NS(tag_id=int(i), pose_R=np.eye(3), pose_t=np.array([[float(x)], [0.0], [float(z)]]), pose_err=float(err))


class World:
    """N tags at distance 0.5 .. 1.1 m around the origin (ids distinct in [0, 1024), not in index order), a true pose that
    follows the reference's motion model."""

    def __init__(self, N, seed):
        self.rng = np.random.default_rng(seed)
        phi = 2 * np.pi * (np.arange(N) + self.rng.uniform(-0.3, 0.3, N)) / N
        r = self.rng.uniform(0.5, 1.1, N)
        self.xy = np.stack([r * np.cos(phi), r * np.sin(phi)], axis=1)
        self.ids = [int(t) for t in self.rng.permutation(900)[:N] + 10]
        self.pose = np.zeros(3)
        self.N = N

    def move(self, lin=LIN, ang=ANG):
        self.pose, _ = orc.motion_model(self.pose, lin, ang, CFG)

    def camera(self, j, noise=0.004):
        """(x, z) of landmark j in the camera frame at the true pose: x = -y_robot, z = x_robot (:321)."""
        d = self.xy[j] - self.pose[:2]
        c, s = np.cos(self.pose[2]), np.sin(self.pose[2])
        xr, yr = c * d[0] + s * d[1], -s * d[0] + c * d[1]
        return -yr + self.rng.normal(0.0, noise), xr + self.rng.normal(0.0, noise)

    def window(self, which, frames=1, noise=0.004):
        """The landmarks `which` seen in `frames` camera frames: the reference's [(timestamp, [tag, ...])] list."""
        return [(float(fr), [det(self.ids[j], *self.camera(j, noise)) for j in which]) for fr in range(frames)]


def mapping_windows(world, count=4, frames=2):
    """`count` windows that together show every tag at least twice (window k: every tag but those with j % count == k)."""
    wins = []
    for k in range(count):
        world.move()
        wins.append(world.window([j for j in range(world.N) if count == 1 or j % count != k], frames))
    return wins


def oracle_map(world, wins, cfg=CFG, p0=CFG.motion_sigma):
    """The map the oracle builds from the mapping windows, from the origin with the pose block p0 * I (the reference's start:
    :69-70): (mean, covariance, tag_index)."""
    mean, cov, index = np.zeros(3), np.eye(3) * p0, {}
    for w in wins:
        mean, cov, _ = orc.ekf_pose_estimation_dense(ANG, LIN, mean, cov, 0.7, w, index, cfg)
    return mean, 0.5 * (cov + cov.T), index


def model_window(mean, cov, index, win, lin=LIN, ang=ANG, cfg=CFG, gate=None, log=None):
    """One localisation window on the dense model: ((mean, covariance), tags, unmatched)."""
    tags, unmatched = frontend.associate_known(win, index, mean[:3], cfg.gate_range, cfg.ignore_tags, n_landmarks=(len(mean) - 3) // 2)
    idx = list(tags)
    state = lm.literal_step(mean, cov, lin, ang, idx, [tags[k][4] for k in idx], [tags[k][5] for k in idx], cfg, gate=gate, log=log)
    return state, tags, unmatched


def mahalanobis(mean, cov, truth):
    d = np.asarray(mean[:3], dtype=float) - truth
    d[2] = orc.wrap_pi(d[2])
    return float(d @ np.linalg.solve(cov[:3, :3], d))


# ---- the recovery case (kidnapped robot): shared by the CPU condition on the model and the GPU run ----
RECOVERY_N, RECOVERY_SEED, RECOVERY_WINDOWS = 6, 41, 8
RECOVERY_OFFSET = np.array([0.3 * np.cos(0.7), 0.3 * np.sin(0.7), 0.2])      # 0.3 m and 0.2 rad away from the truth
RECOVERY_COV = np.diag([0.3 ** 2, 0.3 ** 2, 0.2 ** 2])                       # one sigma = the offset, per axis
RECOVERY_NOISE = dict(motion_sigma=0.01, meas_sigma=0.05)                    # a tuned filter: the defaults' sigma of 0.1 m per step
                                                                             # would cover any offset by itself
RECOVERY_P0 = 1e-4                                                           # the mapping run's start: the map's frame is known to 1 cm
                                                                             # (a pose can be found in a map no better than its frame is)


def recovery_stream():
    """(world, mapping windows, the true pose where the mapping ends and the pose is reset, localisation windows with the true
    pose behind each)."""
    world = World(RECOVERY_N, RECOVERY_SEED)
    wins = mapping_windows(world)
    reset_truth = world.pose.copy()
    loc = []
    for k in range(RECOVERY_WINDOWS):
        world.move()
        loc.append((world.window([(2 * k + i) % world.N for i in range(4)], frames=2), world.pose.copy()))
    return world, wins, reset_truth, loc
