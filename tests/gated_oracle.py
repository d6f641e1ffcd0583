"""The oracle's sequential update, restated so that it also returns what the innovation log and the NIS gate are judged by:
every update's y and S, and -- gated -- its NIS and the decision.  NumPy and the oracle only: the CPU models and the GPU
tests both read them here."""
import numpy as np

from oracle import ekf_oracle as orc

AMAX = 32               # entries of one logged step the library keeps
G = 25.0                # threshold of the gated runs


# ---- the oracle, restated with the innovations -------------------------------------------------------------------------
def update_log(mean, cov, idx, ranges, bearings, cfg):
    """orc.update_dense (src/replay_no_ros.py:436-480) that also returns every update's y and S.  (The covariance down-date
    as cov - K (H cov): the same matrix as (I - K H) cov, in O(n^2).)"""
    n = len(mean)
    mean = np.array(mean, dtype=float)
    Q = np.diag(cfg.meas_noise_diag())
    ys, Ss = [], []
    for j, zr, zb in zip(idx, ranges, bearings):
        t = 3 + 2 * int(j)
        y, h5 = orc.innovation_and_h5(mean[0:3], mean[t:t + 2], zr, zb)
        H = np.zeros((2, n))
        H[:, 0:3] = h5[:, 0:3]
        H[:, t:t + 2] = h5[:, 3:5]
        HP = H @ cov
        S = HP @ H.T + Q
        K = HP.T @ np.linalg.inv(S)
        mean = mean + K @ y
        cov = cov - K @ HP
        ys.append(np.asarray(y, dtype=float).ravel())
        Ss.append(S)
    return mean, cov, np.array(ys).reshape(-1, 2), np.array(Ss).reshape(-1, 2, 2)


def step_log(mean, cov, lin, ang, idx, ranges, bearings, cfg, predict=True):
    if predict:
        mean, cov = orc.predict_dense(mean, cov, lin, ang, cfg)
    return update_log(mean, cov, idx, ranges, bearings, cfg)


def block_err(got, want):
    """Largest relative (Frobenius) error of a stack of 2 x 2 blocks: S's off-diagonal entries are small differences of large
    products, so each block is compared as a matrix."""
    got, want = np.asarray(got).reshape(-1, 4), np.asarray(want).reshape(-1, 4)
    return float(np.max(np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1))) if len(want) else 0.0


# ---- the oracle, gated -------------------------------------------------------------------------------------------------------
def gated_update(mean, cov, idx, ranges, bearings, cfg, g):
    """orc.update_dense (src/replay_no_ros.py:436-480) with the gate: an update whose NIS exceeds g leaves mean and covariance
    as they are.  Returns the state and, per update, y, S, NIS and the decision."""
    n = len(mean)
    mean = np.array(mean, dtype=float)
    Q = np.diag(cfg.meas_noise_diag())
    ys, Ss, nis, rej = [], [], [], []
    for j, zr, zb in zip(idx, ranges, bearings):
        t = 3 + 2 * int(j)
        y, h5 = orc.innovation_and_h5(mean[0:3], mean[t:t + 2], zr, zb)
        y = np.asarray(y, dtype=float).ravel()
        H = np.zeros((2, n))
        H[:, 0:3] = h5[:, 0:3]
        H[:, t:t + 2] = h5[:, 3:5]
        HP = H @ cov
        S = HP @ H.T + Q
        v = float(y @ np.linalg.solve(S, y))
        ys.append(y)
        Ss.append(S)
        nis.append(v)
        rej.append(v > g)
        if v > g:
            continue
        K = HP.T @ np.linalg.inv(S)
        mean = mean + K @ y
        cov = cov - K @ HP
    return mean, cov, np.array(ys).reshape(-1, 2), np.array(Ss).reshape(-1, 2, 2), np.array(nis), np.array(rej, dtype=bool)


def gated_step(mean, cov, lin, ang, idx, ranges, bearings, cfg, g, predict=True):
    """gated_update behind a prediction in O(n^2); returns gated_update's log.  (tests/test_gpu_pose_trace.py's
    gated_step_count predicts with orc.predict_dense and returns the number of rejections instead.)"""
    if predict:
        # orc.predict_dense (:368-430) in O(n^2): G only mixes the pose's rows and columns
        pose, Gm = orc.motion_model(mean[0:3], lin, ang, cfg)
        mean, cov = np.array(mean, dtype=float), np.array(cov, dtype=float)
        if not cfg.disable_motion_model:
            mean[0:3] = pose
        cov[0:3, :] = Gm @ cov[0:3, :]
        cov[:, 0:3] = cov[:, 0:3] @ Gm.T
        cov[0:3, 0:3] += np.diag(cfg.motion_noise_diag())
    return gated_update(mean, cov, idx, ranges, bearings, cfg, g)


def margin(nis, rej, injected, g=G):
    """The test's own margin: injected updates at >= 2 g, the others at <= g / 2."""
    nis, injected = np.asarray(nis), np.asarray(injected, dtype=bool)
    assert injected.any() and (nis[injected] >= 2 * g).all(), nis[injected]
    assert (nis[~injected] <= g / 2).all(), nis[~injected].max()
    assert (np.asarray(rej) == injected).all()


def check_gated_entries(innov, k, b, idx, ys, Ss, nis, rej):
    """Row k, trajectory b of a log against the gated oracle: rejected entries carry the true y, S and NIS."""
    m = len(idx)
    assert innov.m[k, b] == m
    kept = min(m, AMAX)
    assert list(innov.idx[k, b, :kept]) == [int(i) for i in idx[:kept]]
    np.testing.assert_allclose(innov.y[k, b, :kept], ys[:kept], rtol=0, atol=1e-9)
    assert block_err(innov.S[k, b, :kept], Ss[:kept]) < 1e-9
    np.testing.assert_allclose(innov.nis[k, b, :kept], nis[:kept], rtol=1e-9, atol=0)
    assert innov.rejected[k, b, :kept].tolist() == [int(r) for r in rej[:kept]]
    assert (innov.rejected[k, b, kept:] == -1).all()
