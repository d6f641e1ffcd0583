"""Starts and observation streams the tests share, built from the oracle's synthetic worlds.  NumPy and the oracle only."""
import numpy as np

from oracle import ekf_oracle as orc

FRAME = (np.array([0.7, -0.4, 2.1]), np.array([[0.04, 0.01, -0.002], [0.01, 0.09, 0.003], [-0.002, 0.003, 0.002]]))


def dense_start(n, seed, rank=6):
    """A dense, well-conditioned covariance: rank `rank` plus a diagonal in [0.5, 2)."""
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(n, rank)) * 0.3
    P = A @ A.T
    P[np.arange(n), np.arange(n)] += rng.uniform(0.5, 2.0, n)
    return P


def steps_of(streams, k):
    """Step k of one synthetic_stream per trajectory, stacked as step() takes it: lin, ang, idx, zr, zb."""
    return tuple(np.stack([s[i][k] for s in streams]) if i >= 4 else np.array([s[i][k] for s in streams]) for i in (2, 3, 4, 5, 6))


def wandering(N, B, steps, hi, seed):
    """Per trajectory and step m ~ uniform{0..hi} landmarks at scattered indices (tests/test_gpu_cadence.py's stream)."""
    rng = np.random.default_rng(seed)
    world = [orc.synthetic_world(N, seed + 1 + t) for t in range(B)]
    cfg = orc.EkfConfig()
    lin = np.full((steps, B), 0.004)
    ang = np.where(np.arange(steps)[:, None] % 7 == 6, 0.005, 0.02) * np.ones((1, B))
    idx = np.zeros((steps, B, 16), dtype=np.int32)
    zr = np.zeros((steps, B, 16))
    zb = np.zeros((steps, B, 16))
    m = np.zeros((steps, B), dtype=np.int32)
    pose = [np.zeros(3) for _ in range(B)]
    for k in range(steps):
        for b in range(B):
            pose[b], _ = orc.motion_model(pose[b], lin[k, b], ang[k, b], cfg)
            mb = int(rng.integers(0, hi + 1))
            vis = rng.choice(N, size=mb, replace=False)
            d = world[b][1][vis] - pose[b][0:2]
            c, s = np.cos(pose[b][2]), np.sin(pose[b][2])
            xr = c * d[:, 0] + s * d[:, 1] + rng.normal(0, 0.01, mb)
            yr = -s * d[:, 0] + c * d[:, 1] + rng.normal(0, 0.01, mb)
            m[k, b] = mb
            idx[k, b, :mb] = vis
            zr[k, b, :mb] = np.hypot(xr, yr)
            zb[k, b, :mb] = np.arctan2(yr, xr)
    return [w[2] for w in world], lin, ang, idx, zr, zb, m


def stream_from(mean, steps, m, seed):
    """A synthetic stream consistent with a filter's own estimate: the robot starts at the mean's pose and observes the mean's
    landmarks in turn (the construction of oracle.synthetic_stream).  Ranges, bearings and increments only -- the same stream
    in every frame."""
    cfg, rng = orc.EkfConfig(), np.random.default_rng(seed)
    lm, pose, N = mean[3:].reshape(-1, 2), mean[:3].copy(), (len(mean) - 3) // 2
    lin, ang = np.full(steps, 0.004), np.full(steps, 0.02)
    idx, zr, zb = np.zeros((steps, m), dtype=np.int32), np.zeros((steps, m)), np.zeros((steps, m))
    for k in range(steps):
        pose, _ = orc.motion_model(pose, lin[k], ang[k], cfg)
        vis = (m * k + np.arange(m)) % N
        d = lm[vis] - pose[:2]
        c, s = np.cos(pose[2]), np.sin(pose[2])
        xr = c * d[:, 0] + s * d[:, 1] + rng.normal(0.0, 0.01, m)
        yr = -s * d[:, 0] + c * d[:, 1] + rng.normal(0.0, 0.01, m)
        idx[k], zr[k], zb[k] = vis, np.sqrt(xr ** 2 + yr ** 2), np.arctan2(yr, xr)
    return lin, ang, idx, zr, zb


def inject(zr, zb, where):
    """Outliers at (step, [trajectory,] landmark) positions: range + 20 m."""
    zr = np.array(zr, dtype=float)
    for pos in where:
        zr[pos] += 20.0
    return zr, np.array(zb, dtype=float)


def observed_start(N, seed):
    """A start whose landmarks have been observed before: means at synthetic_stream's true positions (its world `seed`),
    variance 0.01 (a first observation, with its prior variance of 1e4, is never an outlier)."""
    _, lm, mean0, diag0 = orc.synthetic_world(N, seed)
    mean0 = mean0.copy()
    mean0[3:] = lm.ravel()
    diag0 = diag0.copy()
    diag0[3:] = 0.01
    return mean0, diag0
