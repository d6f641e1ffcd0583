"""The dense model of localisation on a frozen map (ekf_localize_step / _update / _run): the Schmidt-Kalman ("consider") update,
in which the landmarks' gain is zero while their uncertainty and correlations still enter S and the pose rows.  NumPy and the
oracle only; a plain module the CPU and GPU tests import.

Two forms of one step for one trajectory, both with the NIS gate (`gate`: a threshold or None) and per-trajectory noise (the
`cfg` handed in: `with_noise`), both returning (mean, covariance) and appending one (index, y, S, NIS, rejected) per
observation to `log` where given:

`literal_step`  oracle.predict_dense, then per observation oracle.innovation_and_h5 at the current pose and the frozen landmark
                mean, the full S = H P H^T + Q, K = P H^T S^-1 with its rows >= 3 zeroed, and the Joseph form
                (I - K H) P (I - K H)^T + K Q K^T on the whole matrix.
`rows_step`     the same step on rows and columns 0..2 alone -- P[0:3, c] <- P[0:3, c] - K_p (H P)[:, c], the pose block
                P_pp - K_p S K_p^T -- for states where the Joseph products (O(n^3)) are too slow.  The landmark block is never
                read into a product that is written back, so it is unchanged by construction.
"""
import dataclasses

import numpy as np

from oracle import ekf_oracle as orc


def with_noise(cfg, motion_sigma=None, meas_sigma=None):
    """`cfg` with one trajectory's noise constants (set_noise's row)."""
    return dataclasses.replace(cfg, motion_sigma=cfg.motion_sigma if motion_sigma is None else float(motion_sigma),
                               meas_sigma=cfg.meas_sigma if meas_sigma is None else float(meas_sigma))


def _observations(cfg, idx, zr, zb):
    if not cfg.enable_measurement_model:
        return []
    return list(zip([int(j) for j in idx], [float(r) for r in zr], [float(b) for b in zb]))


def literal_step(mean, cov, lin, ang, idx, zr, zb, cfg, gate=None, predict=True, log=None):
    mean, cov = np.array(mean, dtype=float), np.array(cov, dtype=float)
    n = len(mean)
    if predict:
        mean, cov = orc.predict_dense(mean, cov, lin, ang, cfg)
    Q = np.diag(cfg.meas_noise_diag())
    for j, r, b in _observations(cfg, idx, zr, zb):
        t = 3 + 2 * j
        y, h5 = orc.innovation_and_h5(mean[0:3], mean[t:t + 2], r, b)
        H = np.zeros((2, n))
        H[:, 0:3] = h5[:, 0:3]
        H[:, t:t + 2] = h5[:, 3:5]
        S = H @ cov @ H.T + Q
        Si = np.linalg.inv(S)
        nis = float(y @ Si @ y)
        rejected = gate is not None and nis > gate
        if log is not None:
            log.append((j, y.copy(), S.copy(), nis, bool(rejected)))
        if rejected:
            continue
        K = cov @ H.T @ Si
        K[3:] = 0.0                                                # the landmarks' gain: the map is frozen
        mean = mean + K @ y
        IKH = np.eye(n) - K @ H
        cov = IKH @ cov @ IKH.T + K @ Q @ K.T
    return mean, cov


def rows_step(mean, cov, lin, ang, idx, zr, zb, cfg, gate=None, predict=True, log=None):
    mean, cov = np.array(mean, dtype=float), np.array(cov, dtype=float)
    if predict:
        pose, G = orc.motion_model(mean[0:3], lin, ang, cfg)
        if not cfg.disable_motion_model:
            mean[0:3] = pose
        X = G @ cov[0:3, :]
        X[:, 0:3] = G @ cov[0:3, 0:3] @ G.T + np.diag(cfg.motion_noise_diag())
        X[:, 0:3] = 0.5 * (X[:, 0:3] + X[:, 0:3].T)
        cov[0:3, :] = X
        cov[:, 0:3] = X.T
    Q = np.diag(cfg.meas_noise_diag())
    for j, r, b in _observations(cfg, idx, zr, zb):
        t = 3 + 2 * j
        sel = [0, 1, 2, t, t + 1]
        y, h5 = orc.innovation_and_h5(mean[0:3], mean[t:t + 2], r, b)
        HP = h5 @ cov[sel, :]                                      # (2, n): H P
        S = HP[:, sel] @ h5.T + Q
        Si = np.linalg.inv(S)
        nis = float(y @ Si @ y)
        rejected = gate is not None and nis > gate
        if log is not None:
            log.append((j, y.copy(), S.copy(), nis, bool(rejected)))
        if rejected:
            continue
        Kp = HP[:, 0:3].T @ Si                                     # (3, 2): (P H^T)[0:3] S^-1
        mean[0:3] = mean[0:3] + Kp @ y
        X = cov[0:3, :] - Kp @ HP
        Ppp = cov[0:3, 0:3] - Kp @ S @ Kp.T
        X[:, 0:3] = 0.5 * (Ppp + Ppp.T)
        cov[0:3, :] = X
        cov[:, 0:3] = X.T
    return mean, cov


def run(step, mean, cov, lin, ang, idx, zr, zb, cfg, m=None, gate=None, logs=None):
    """`step` (literal_step or rows_step) over the steps of one trajectory's stream: lin, ang [K]; idx, zr, zb [K, stride]; m [K]
    valid entries per step (default: all).  `logs`: a list that gets one list of observation records per step."""
    for k in range(len(lin)):
        mk = idx.shape[1] if m is None else int(m[k])
        log = [] if logs is not None else None
        mean, cov = step(mean, cov, lin[k], ang[k], idx[k][:mk], zr[k][:mk], zb[k][:mk], cfg, gate=gate, log=log)
        if logs is not None:
            logs.append(log)
    return mean, cov


def rel(a, b):
    den = np.linalg.norm(b)
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / den) if den > 0 else float(np.linalg.norm(np.asarray(a) - np.asarray(b)))
