"""Accuracy and consistency evaluation.  Host-side NumPy; the filters run on the GPU.

* Vicon alignment of the reference's ground truth (scripts/decode_bag_file.py:107-109, :167-181, :241-246):
  rotate the Vicon points about the robot's first pose by its first heading, subtract that pose, mm -> m.
* ATE / RMSE of an estimated path against ground truth (what the reference only eyeballs in its plots,
  src/replay_no_ros.py:520-529).
* NIS of every landmark update from the innovation log (`nis_consistency`): consistency without ground truth.
* A tuning sweep of the motion and measurement noise (`tune_noise`): a grid of noise pairs as the trajectories of one
  bank (``EkfSlam.set_noise``), each scored by the log-likelihood of its innovations.
* NEES of the pose over a batch of Monte-Carlo trajectories with chi-square consistency bounds: the
  batched filter bank (`EkfSlam(batch=B)`) is exactly the Monte-Carlo tool this needs.  `marginal_nees` takes the
  pose and landmark blocks of the whole bank from one `marginals()` call (no covariance pass): cheap enough for
  every step of a run.
* `association_check`: labelled observations judged by the likelihood query (``EkfSlam.associate``) -- the misread-tag
  detector.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np


def rotate_around(a, b, x, y, theta):
    """Rotate (x, y) about (a, b) by theta (scripts/decode_bag_file.py:107-109)."""
    return (a + (x - a) * math.cos(theta) - (y - b) * math.sin(theta),
            b + (x - a) * math.sin(theta) + (y - b) * math.cos(theta))


def align_vicon(points_mm, init_x: float, init_y: float, init_theta: float) -> np.ndarray:
    """Vicon points (mm, Vicon frame) -> metres in the frame the reference plots them in (:176-178, :242-244)."""
    pts = np.asarray(points_mm, dtype=float).reshape(-1, 2)
    c, s = math.cos(init_theta), math.sin(init_theta)
    dx, dy = pts[:, 0] - init_x, pts[:, 1] - init_y
    x = init_x + dx * c - dy * s
    y = init_y + dx * s + dy * c
    return np.stack([(x - init_x) / 1000.0, (y - init_y) / 1000.0], axis=1)


def load_vicon_csv(path: str):
    """Rows of a Vicon export the way the reference reads them (scripts/decode_bag_file.py:139-146, :187-195):
    five header lines skipped, the rest split on commas.  Returns (fields, lengths): `fields` is (rows, width)
    float64 with NaN where a field is empty or absent, `lengths` the number of fields of every row."""
    with open(path, "r") as fh:
        for _ in range(5):
            fh.readline()
        rows = [ln.split(",") for ln in fh.read().strip().splitlines()]
    width = max(len(r) for r in rows)
    out = np.full((len(rows), width), np.nan)
    for i, r in enumerate(rows):
        for j, f in enumerate(r):
            if f != "":
                out[i, j] = float(f)
    return out, np.array([len(r) for r in rows])


def vicon_ground_truth(robot, markers, start_capture_time: float, end_capture_time: float, first_timestamp: float,
                       delay: float = 0.0, robot_len=None, marker_len=None) -> dict:
    """Ground truth of a Vicon recording in the frame the filter starts in: what the reference's
    ``get_ground_truth`` (scripts/decode_bag_file.py:111-253) turns into ``ground_truth`` / ``landmarks`` events.

    robot:   (rows, 8)  Frame, Sub Frame, RX, RY, RZ [rad], TX, TY, TZ [mm]            (:139-151)
    markers: (rows, 2 + 3 k)  Frame, Sub Frame, then X, Y, Z [mm] per marker, NaN = not seen   (:187-195)
    Times: frame / framerate + start_capture_time + delay with framerate = round(rows / capture length) (:149, :154).
    The Vicon frame closest to `first_timestamp` (the first event of the bag) defines the origin: every point is
    rotated about that position by that heading, the position is subtracted, mm -> m (:167-181, :241-246).  A marker's
    position is the middle of its x and y ranges over the recording (:201-222).  Kept from the reference so that its
    outputs are reproduced exactly: a coordinate equal to 0.0 counts as missing (`!= False`, :206, :214); a marker
    is dropped as a duplicate when its RAW position (mm) lies within 10 of an already accepted NORMALISED landmark
    (m), i.e. practically never (:231-239); a marker never seen sits at raw (0, 0); the "moved too much" test compares
    min - max (:225-228, the names are swapped at the unpacking) and so never fires.
    Raises ValueError where the reference prints and exits (:157-164).
    Returns dict(times, xy (rows, 2) [m], landmarks (k', 2) [m], landmarks_time, origin=(x, y, theta), framerate)."""
    robot = np.asarray(robot, dtype=float)
    markers = np.asarray(markers, dtype=float)
    n_rows = robot.shape[0]
    framerate = round(n_rows / (end_capture_time - start_capture_time))                      # :149
    ok = np.ones(n_rows, dtype=bool) if robot_len is None else np.asarray(robot_len) == 8    # :148
    rob = robot[ok]
    times = rob[:, 0].astype(np.int64) / framerate + start_capture_time + delay             # :154
    k = int(np.argmin(np.abs(times - first_timestamp)))                                      # :157 (stable: first minimum)
    if abs(times[k] - first_timestamp) > 2:                                                  # :158
        raise ValueError("cannot find a matching time between the ground truth and the bag data "
                         f"(closest differs by {times[k] - first_timestamp:.3f} s); use `delay`")
    init_theta, init_x, init_y = float(rob[k, 4]), float(rob[k, 5]), float(rob[k, 6])      # :168
    c, s = math.cos(init_theta), math.sin(init_theta)

    def normalise(x, y):                                                                     # rotate_around + :177-178
        rx = init_x + (x - init_x) * c - (y - init_y) * s
        ry = init_y + (x - init_x) * s + (y - init_y) * c
        return (rx - init_x) / 1000, (ry - init_y) / 1000

    gx, gy = normalise(rob[:, 5], rob[:, 6])
    mok = np.ones(markers.shape[0], dtype=bool) if marker_len is None else np.asarray(marker_len) > 4    # :192
    mk = markers[mok]
    count = mk.shape[1] // 3                                                                 # :196
    landmarks = []
    for q in range(count):
        xs, ys = mk[:, 3 * q + 2], mk[:, 3 * q + 3]
        xs, ys = xs[~np.isnan(xs) & (xs != 0.0)], ys[~np.isnan(ys) & (ys != 0.0)]          # `!= False`
        hi_x, lo_x = (xs.max(), xs.min()) if xs.size else (0.0, 0.0)
        hi_y, lo_y = (ys.max(), ys.min()) if ys.size else (0.0, 0.0)
        if lo_x - hi_x > 20 or lo_y - hi_y > 20:                                             # :225-228 as written
            raise ValueError("landmarks have moved too much")
        pos_x, pos_y = (hi_x + lo_x) / 2, (hi_y + lo_y) / 2                                  # :230
        if any((pos_x - lx) ** 2 + (pos_y - ly) ** 2 < 10 ** 2 for lx, ly in landmarks):    # :233-239
            continue
        nx, ny = normalise(pos_x, pos_y)
        landmarks.append((float(nx), float(ny)))
    return dict(times=times, xy=np.stack([gx, gy], axis=1), landmarks=np.array(landmarks, dtype=float).reshape(-1, 2),
                landmarks_time=first_timestamp, origin=(init_x, init_y, init_theta), framerate=framerate)


def wrap_angle(a):
    return (np.asarray(a) + np.pi) % (2 * np.pi) - np.pi


def ate_rmse(estimate_xy, truth_xy, align: bool = False) -> float:
    """Absolute trajectory error (RMSE of the position difference).  align=True first removes the best
    rigid transform (rotation + translation, Kabsch) -- use it when the two frames are not registered."""
    e = np.asarray(estimate_xy, dtype=float).reshape(-1, 2)
    t = np.asarray(truth_xy, dtype=float).reshape(-1, 2)
    if e.shape != t.shape:
        raise ValueError("estimate and truth must have the same number of points")
    if align:
        ec, tc = e.mean(axis=0), t.mean(axis=0)
        H = (e - ec).T @ (t - tc)
        U, _, Vt = np.linalg.svd(H)
        d = np.sign(np.linalg.det(Vt.T @ U.T))
        R = Vt.T @ np.diag([1.0, d]) @ U.T
        e = (e - ec) @ R.T + tc
    return float(np.sqrt(np.mean(np.sum((e - t) ** 2, axis=1))))


def resample_truth(truth_t, truth_xy, query_t) -> np.ndarray:
    """Ground-truth positions linearly interpolated at the estimate's time stamps."""
    truth_t = np.asarray(truth_t, dtype=float)
    truth_xy = np.asarray(truth_xy, dtype=float).reshape(-1, 2)
    return np.stack([np.interp(query_t, truth_t, truth_xy[:, 0]), np.interp(query_t, truth_t, truth_xy[:, 1])], axis=1)


def nees(errors, covariances) -> np.ndarray:
    """e^T P^-1 e per sample; errors (B, d), covariances (B, d, d)."""
    e = np.asarray(errors, dtype=float)
    P = np.asarray(covariances, dtype=float)
    return np.einsum("bi,bi->b", e, np.linalg.solve(P, e[..., None])[..., 0])


def chi2_bounds(dof: int, runs: int, confidence: float = 0.95) -> Tuple[float, float]:
    """Two-sided bounds for the AVERAGE NEES of `runs` independent runs (Bar-Shalom's ANEES test)."""
    from scipy.stats import chi2
    a = (1.0 - confidence) / 2.0
    return chi2.ppf(a, dof * runs) / runs, chi2.ppf(1.0 - a, dof * runs) / runs


def pose_nees(filter_bank, true_poses: Sequence[Sequence[float]]):
    """NEES of [x, y, theta] for every trajectory of an ``EkfSlam`` bank; downloads only the 3x3 pose blocks.

    Returns (nees per trajectory (B,), average NEES, (lower, upper) 95 % bounds for a consistent filter).
    An average above the upper bound means the filter is over-confident, below the lower one conservative.
    """
    true_poses = np.asarray(true_poses, dtype=float).reshape(filter_bank.batch, 3)
    errs, covs = [], []
    for b in range(filter_bank.batch):
        mu = filter_bank.mean(b)[:3]
        e = mu - true_poses[b]
        e[2] = wrap_angle(e[2])
        errs.append(e)
        covs.append(filter_bank.covariance_block(0, 0, 3, 3, b))
    vals = nees(np.array(errs), np.array(covs))
    return vals, float(vals.mean()), chi2_bounds(3, filter_bank.batch)


def trajectory_ate(trace, truth_xy, align: bool = False) -> np.ndarray:
    """``ate_rmse`` of every trajectory of a pose trace (``EkfSlam.poses()``) over its logged steps: (B,).

    `truth_xy` is (T, 2) -- one ground-truth path shared by the bank -- or (T, B, 2), row k the truth at the time of the
    trace's row k.  A hypothesis bank's trace (``HypothesisBank.trace()``: one mixture mean per step, (T, 3)) counts as a bank
    of one."""
    mean = np.asarray(trace.mean, dtype=float)
    if mean.ndim == 2:
        mean = mean[:, None, :]
    T, B = mean.shape[0], mean.shape[1]
    truth = np.asarray(truth_xy, dtype=float)
    if truth.shape == (T, 2):
        truth = np.broadcast_to(truth[:, None, :], (T, B, 2))
    if truth.shape != (T, B, 2):
        raise ValueError("truth_xy must be (T, 2) or (T, B, 2) for a trace of T steps and B trajectories")
    return np.array([ate_rmse(mean[:, b, :2], truth[:, b], align=align) for b in range(B)])


class PoseNeesSeries(NamedTuple):
    nees: np.ndarray      # (T, B)  e^T P^-1 e of [x, y, theta] per step and trajectory
    anees: np.ndarray     # (T,)    its mean over the bank
    lower: float          # two-sided bounds of the bank average for a consistent filter (chi2_bounds(3, B, confidence))
    upper: float
    inside: float         # share of the steps with lower <= anees <= upper


def pose_nees_series(trace, true_poses, confidence: float = 0.95) -> PoseNeesSeries:
    """Pose NEES at every logged step of a pose trace (``EkfSlam.poses()``) against ground truth.

    `true_poses` is (T, 3) -- shared by the bank -- or (T, B, 3): [x, y, theta] at the time of the trace's row k; the
    theta error is wrapped (``wrap_angle``).  ``anees`` averages over the B trajectories of the bank, which are independent
    runs: a consistent filter keeps it within ``chi2_bounds(3, B, confidence)`` at about `confidence` of the steps
    (Bar-Shalom's ANEES test); above the upper bound the filter is over-confident, below the lower one conservative.
    Only the bank average per step is tested against bounds.  The NEES values along ONE trajectory are correlated in
    time (every step's error carries the errors before it), so their time average is not chi-square with T x 3 degrees
    of freedom and no time-averaged bound is offered."""
    mean = np.asarray(trace.mean, dtype=float)
    cov = np.asarray(trace.cov, dtype=float)
    T, B = mean.shape[0], mean.shape[1]
    truth = np.asarray(true_poses, dtype=float)
    if truth.shape == (T, 3):
        truth = np.broadcast_to(truth[:, None, :], (T, B, 3))
    if truth.shape != (T, B, 3):
        raise ValueError("true_poses must be (T, 3) or (T, B, 3) for a trace of T steps and B trajectories")
    e = mean - truth
    e[..., 2] = wrap_angle(e[..., 2])
    vals = nees(e.reshape(T * B, 3), cov.reshape(T * B, 3, 3)).reshape(T, B)
    anees = vals.mean(axis=1) if B else np.zeros(T)
    lower, upper = chi2_bounds(3, B, confidence)
    inside = float(np.mean((anees >= lower) & (anees <= upper))) if T else float("nan")
    return PoseNeesSeries(vals, anees, float(lower), float(upper), inside)


class MarginalNees(NamedTuple):
    pose: np.ndarray                          # (B,) pose NEES per trajectory
    pose_anees: float                         # their average
    pose_bounds: Tuple[float, float]          # 95 % ANEES bounds, chi2_bounds(3, B)
    landmarks: Optional[np.ndarray]           # (B, N) 2-dof NEES per landmark (NaN where a trajectory has fewer), or None
    landmark_bounds: Optional[Tuple[float, float]]   # chi2_bounds(2, B), or None


def marginal_nees(filter_bank, true_poses, true_landmarks=None) -> MarginalNees:
    """Pose NEES of every trajectory of a bank and, given `true_landmarks` (B, N, 2), every landmark's 2-dof NEES -- from
    ONE ``filter_bank.marginals()`` call (the diagonal blocks of the current covariance, no covariance pass) plus one mean
    download per trajectory (which never flushes).  Unlike `pose_nees` it leaves the filter's pass cadence alone, so it
    can be sampled at every step."""
    B = filter_bank.batch
    true_poses = np.asarray(true_poses, dtype=float).reshape(B, 3)
    pose, lms, counts = filter_bank.marginals()
    means = [np.asarray(filter_bank.mean(b), dtype=float) for b in range(B)]
    errs = np.array([m[:3] for m in means]) - true_poses
    errs[:, 2] = wrap_angle(errs[:, 2])
    vals = nees(errs, pose)
    lm_vals, lm_bounds = None, None
    if true_landmarks is not None:
        truth = np.asarray(true_landmarks, dtype=float)
        truth = truth.reshape(B, -1, 2)
        lm_vals = np.full(truth.shape[:2], np.nan)
        for b in range(B):
            k = min(int(counts[b]), truth.shape[1])
            if k:
                e = means[b][3:3 + 2 * k].reshape(k, 2) - truth[b, :k]
                lm_vals[b, :k] = nees(e, lms[b, :k])
        lm_bounds = chi2_bounds(2, B)
    return MarginalNees(vals, float(vals.mean()), chi2_bounds(3, B), lm_vals, lm_bounds)


class MapNees(NamedTuple):
    nees: np.ndarray                          # (B,) full-state NEES e^T P^-1 e per trajectory (NaN where info != 0)
    dof: np.ndarray                           # (B,) its degrees of freedom: the state size n
    info: np.ndarray                          # (B,) 0, or the order of the first leading minor of P that is not positive definite
    anees: Optional[float]                    # average over the bank where every trajectory has the same n, else None
    bounds: Optional[Tuple[float, float]]     # chi2_bounds(n, B, confidence) for that average, else None


def map_nees(filter_bank, true_poses, true_landmarks, confidence: float = 0.95) -> MapNees:
    """Full-state NEES of every trajectory of a bank: e^T P^-1 e with the WHOLE covariance -- pose, every landmark and all
    their cross-covariances, where EKF-SLAM's over-confidence lives -- through one ``filter_bank.factor()`` (the Cholesky
    factor formed on the device) and one ``mahalanobis``.  `true_poses` (B, 3), `true_landmarks` (B, N, 2) with N at least
    each trajectory's landmark count; the theta error is wrapped.  ``dof`` is n per trajectory; the bank average and its
    ``chi2_bounds(n, B, confidence)`` are given where all sizes agree.  ``info`` reports an indefinite P (LAPACK dpotrf's
    convention) instead of folding it into a NaN: that trajectory's NEES is NaN and ``anees`` with it."""
    B = filter_bank.batch
    true_poses = np.asarray(true_poses, dtype=float).reshape(B, 3)
    truth = np.asarray(true_landmarks, dtype=float).reshape(B, -1, 2)
    fac = filter_bank.factor()
    n = np.asarray(fac.n)
    e = np.zeros((B, int(n.max())))
    for b in range(B):
        k = (int(n[b]) - 3) // 2
        if truth.shape[1] < k:
            raise ValueError(f"true_landmarks holds {truth.shape[1]} landmarks, trajectory {b} has {k}")
        e[b, :3] = fac.means[b][:3] - true_poses[b]
        e[b, 2] = wrap_angle(e[b, 2])
        e[b, 3:n[b]] = fac.means[b][3:] - truth[b, :k].reshape(-1)
    vals = np.asarray(fac.mahalanobis(e), dtype=float)
    same = bool((n == n[0]).all())
    return MapNees(vals, n.copy(), np.asarray(fac.info).copy(), float(vals.mean()) if same else None,
                   chi2_bounds(int(n[0]), B, confidence) if same else None)


def map_entropy(factor) -> np.ndarray:
    """Differential entropy of N(mean, P) per trajectory of a ``CovFactor``, in nats: (n ln 2 pi e + ln det P) / 2."""
    return 0.5 * (np.asarray(factor.n) * math.log(2.0 * math.pi * math.e) + np.asarray(factor.logdet))


def information_gain(before, after) -> np.ndarray:
    """Entropy lost between two ``CovFactor``s of the same trajectories, in nats (positive: the map knows more)."""
    return map_entropy(before) - map_entropy(after)


class NisConsistency(NamedTuple):
    step_anis: np.ndarray            # (K,) per step: the bank's NIS summed over its updates, divided by B (NaN: no update)
    step_bounds: np.ndarray          # (K, 2) two-sided bounds of step_anis: chi2(2 sum m) / B
    traj_anis: np.ndarray            # (B,) per trajectory: its NIS summed over the run, divided by K (NaN: no update)
    traj_bounds: np.ndarray          # (B, 2) two-sided bounds of traj_anis: chi2(2 sum m) / K
    gate: float                      # the chi2_2 quantile at `confidence`
    above_gate: float                # share of all updates whose NIS exceeds it (about 1 - confidence when consistent)
    loglik: np.ndarray               # (B,) per trajectory: sum of -(NIS + log det(2 pi S)) / 2 over its updates
    updates: int                     # updates counted (NaN padding excluded)


def nis_consistency(innov, confidence: float = 0.95) -> NisConsistency:
    """Consistency statistics of an innovation log (``EkfSlam.innovations()``: ``nis`` (K, B, W), ``S`` (K, B, W, 2, 2),
    NaN-padded) -- the check that needs no ground truth.  Each update's NIS = y^T S^-1 y is chi2 with 2 dof for a consistent
    filter, so a sum over u updates is chi2 with 2u dof: the per-step bank average and the per-trajectory time average come
    with two-sided bounds at `confidence` for their own update counts (an average above its upper bound: the filter is
    over-confident; below the lower one: conservative).  ``loglik`` is each trajectory's Gaussian log-likelihood of its
    innovations, the quantity to maximise when tuning the motion and measurement variances."""
    from scipy.stats import chi2
    nis = np.asarray(innov.nis, dtype=float)
    S = np.asarray(innov.S, dtype=float)
    K, B = nis.shape[:2]
    ok = np.isfinite(nis)
    v = np.where(ok, nis, 0.0)
    a = (1.0 - confidence) / 2.0

    def bounds(n_updates, runs):
        dof = 2.0 * np.asarray(n_updates, dtype=float)
        with np.errstate(invalid="ignore", divide="ignore"):
            lo = np.where(dof > 0, chi2.ppf(a, np.maximum(dof, 1.0)), np.nan) / runs
            hi = np.where(dof > 0, chi2.ppf(1.0 - a, np.maximum(dof, 1.0)), np.nan) / runs
        return np.stack([lo, hi], axis=-1)

    per_step = ok.reshape(K, -1).sum(axis=1)
    per_traj = ok.sum(axis=(0, 2)) if K else np.zeros(B, dtype=int)
    step_anis = np.where(per_step > 0, v.reshape(K, -1).sum(axis=1) / max(B, 1), np.nan)
    traj_anis = np.where(per_traj > 0, v.sum(axis=(0, 2)) / max(K, 1), np.nan) if K else np.full(B, np.nan)
    gate = float(chi2.ppf(confidence, 2))
    total = int(ok.sum())
    above = float((v[ok] > gate).sum()) / total if total else float("nan")
    Sg = np.where(ok[..., None, None], S, np.eye(2) / (2.0 * np.pi))    # (padding: det(2 pi S) = 1, contributes 0)
    _sign, logdet = np.linalg.slogdet(2.0 * np.pi * Sg)
    loglik = -0.5 * np.where(ok, v + logdet, 0.0).sum(axis=(0, 2)) if K else np.zeros(B)
    return NisConsistency(step_anis, bounds(per_step, max(B, 1)), traj_anis, bounds(per_traj, max(K, 1)), gate, above,
                          loglik, total)


class HypothesisResolution(NamedTuple):
    best: int                        # the hypothesis with the largest log-likelihood (the first of equals)
    weight: float                    # its normalised weight exp(loglik - max) / sum
    separated: bool                  # the runner-up's weight is below (1 - confidence) x the best's
    runner_up: int                   # the second-best hypothesis (-1 in a bank of one)
    ratio: float                     # runner-up weight / best weight (0 in a bank of one)


def resolve_hypotheses(bank, confidence: float = 0.99) -> HypothesisResolution:
    """Has a hypothesis bank (``EkfSlam.hypotheses``; or an array of log-likelihoods) settled on one pose?  The best hypothesis,
    its posterior weight under equal priors, and whether it is SEPARATED: the runner-up's weight, relative to the best's, is
    below ``1 - confidence``.  Hypotheses without a finite log-likelihood weigh nothing; equal log-likelihoods are never
    separated."""
    from .ekf_bindings import HypothesisBank
    if not 0.0 < float(confidence) < 1.0:
        raise ValueError(f"resolve_hypotheses: confidence must lie in (0, 1), got {confidence!r}")
    w = HypothesisBank.weights_of(bank.loglik if hasattr(bank, "loglik") else bank)
    if w.size == 0:
        raise ValueError("resolve_hypotheses: an empty bank")
    best = int(np.argmax(w))
    if w.size == 1:
        return HypothesisResolution(best, float(w[best]), True, -1, 0.0)
    rest = w.copy()
    rest[best] = -1.0
    second = int(np.argmax(rest))
    ratio = float(w[second] / w[best])
    return HypothesisResolution(best, float(w[best]), ratio < 1.0 - float(confidence), second, ratio)


def clutter_loglik(accept: float, meas_sigma: float) -> float:
    """A default for ``HypothesisBank.step_unlabelled``'s ``miss``: the log-likelihood of an observation sitting exactly on the
    acceptance boundary under the measurement noise R = meas_sigma^2 I alone, ``-1/2 (accept + ln det R + 2 ln 2 pi)``.  An
    observation a hypothesis cannot match then costs it what the worst match it would still have accepted costs under the
    tightest S a landmark can have; without such a term a hypothesis that matches nothing is never penalised."""
    accept, meas_sigma = float(accept), float(meas_sigma)
    if not (accept >= 0.0 and math.isfinite(accept)):
        raise ValueError(f"clutter_loglik: accept must be finite and >= 0, got {accept!r}")
    if not (meas_sigma > 0.0 and math.isfinite(meas_sigma)):
        raise ValueError(f"clutter_loglik: meas_sigma must be finite and > 0, got {meas_sigma!r}")
    return -0.5 * (accept + 4.0 * math.log(meas_sigma) + 2.0 * math.log(2.0 * math.pi))


class MixturePose(NamedTuple):
    mean: np.ndarray                 # (3,) the weighted mean pose, the heading averaged on the circle
    cov: np.ndarray                  # (3, 3) sum w (P_k + d_k d_k^T), d_k the deviation from the mean (heading wrapped)
    weights: np.ndarray              # (K,) the weights used


def mixture_pose(bank, weights=None) -> MixturePose:
    """The mean and covariance of a hypothesis bank's pose mixture sum_k w_k N(pose_k, P_k): what a Gaussian-sum localiser
    reports between resamplings.  ``bank``: a ``HypothesisBank`` (anything with ``poses()`` and ``loglik``; a hypothesis whose
    ``flags()`` are set weighs nothing, as on the device) or a pair (poses (K, 3), blocks (K, 3, 3)) with ``weights``.  The heading
    is averaged on the circle -- atan2 of the weighted sine and cosine -- and deviations from it are wrapped to [-pi, pi)."""
    from .ekf_bindings import HypothesisBank
    if hasattr(bank, "poses"):
        poses, blocks = bank.poses()
        if weights is None:
            ll = np.array(bank.loglik, dtype=np.float64)
            if hasattr(bank, "flags"):
                ll = np.where(np.asarray(bank.flags()) != 0, -np.inf, ll)
            weights = HypothesisBank.weights_of(ll)
    else:
        poses, blocks = bank
    poses, blocks = np.asarray(poses, dtype=np.float64).reshape(-1, 3), np.asarray(blocks, dtype=np.float64).reshape(-1, 3, 3)
    w = np.full(len(poses), 1.0 / max(len(poses), 1)) if weights is None else np.asarray(weights, dtype=np.float64)
    if len(poses) == 0 or w.shape != (len(poses),) or not w.sum() > 0.0:
        raise ValueError("mixture_pose: an empty bank, or weights that do not match it or sum to nothing")
    w = w / w.sum()
    use = w > 0.0                                                              # (a dead hypothesis may hold NaN: 0 * NaN)
    p, P, w = poses[use], blocks[use], w[use]
    mean = np.array([w @ p[:, 0], w @ p[:, 1], np.arctan2(w @ np.sin(p[:, 2]), w @ np.cos(p[:, 2]))])
    d = p - mean
    d[:, 2] = wrap_angle(d[:, 2])
    cov = np.einsum("k,kij->ij", w, P) + np.einsum("k,ki,kj->ij", w, d, d)
    out = np.zeros(len(poses))
    out[use] = w
    return MixturePose(mean, 0.5 * (cov + cov.T), out)


class LandmarkRejections(NamedTuple):
    applied: np.ndarray              # (B, L) int64: updates of landmark l that trajectory b applied
    rejected: np.ndarray             # (B, L) int64: ... that the NIS gate rejected (L = largest logged index + 1)


def landmark_rejections(innov) -> LandmarkRejections:
    """Per trajectory and landmark, how many of its logged updates were applied and how many the NIS gate rejected, from an
    innovation log (``EkfSlam.innovations()``).  A landmark whose later sightings are all rejected was most likely initialised
    from a bad first detection (a new landmark's first update never reaches the gate): the evidence for
    ``EkfSlam.remove_landmarks``.  Entries beyond a step's m (index -1) are not counted; a log without rejection data counts
    every update as applied.  Indices are as they were when each step was logged."""
    idx = np.asarray(innov.idx)
    K, B = idx.shape[:2]
    W = idx.shape[2] if idx.ndim == 3 else 0
    m = np.minimum(np.asarray(innov.m).reshape(K, B), W)
    valid = (np.arange(W)[None, None, :] < m[..., None]) & (idx >= 0)
    rej = np.zeros(idx.shape, dtype=bool) if innov.rejected is None else np.asarray(innov.rejected) == 1
    L = int(idx[valid].max()) + 1 if valid.any() else 0
    applied = np.zeros((B, L), dtype=np.int64)
    rejected = np.zeros((B, L), dtype=np.int64)
    bb = np.broadcast_to(np.arange(B)[None, :, None], idx.shape)
    np.add.at(applied, (bb[valid & ~rej], idx[valid & ~rej]), 1)
    np.add.at(rejected, (bb[valid & rej], idx[valid & rej]), 1)
    return LandmarkRejections(applied, rejected)


class NoiseTuning(NamedTuple):
    motion_sigmas: np.ndarray        # (Gm,) the grid's motion sigmas (rows)
    meas_sigmas: np.ndarray          # (Gq,) the grid's measurement sigmas (columns)
    loglik: np.ndarray               # (Gm, Gq) nis_consistency's loglik of each grid point's run
    traj_anis: np.ndarray            # (Gm, Gq) its time-averaged NIS ...
    traj_bounds: np.ndarray          # (Gm, Gq, 2) ... with the two-sided bounds at `confidence`
    best: Tuple[float, float]        # (motion sigma, measurement sigma) of the largest loglik
    bank_sizes: Tuple[int, ...]      # trajectories of each bank that ran


_TUNE_BANK_BYTES = 2 << 30           # (one bank holds the whole grid while its covariances and pending factors fit this)


def tune_noise(stream, motion_sigmas, meas_sigmas, mean0, diag0, *, n_max: Optional[int] = None,
               bank_size: Optional[int] = None, confidence: float = 0.95, device: int = 0, config=None,
               filter_factory=None, start=None) -> NoiseTuning:
    """Tune the motion and measurement noise (the reference's MOTION_MODEL_VARIANCE / MEASUREMENT_MODEL_VARIANCE,
    src/replay_no_ros.py:15-16) on one recorded stream by maximum likelihood of the innovations.

    `stream` is ONE trajectory's input as ``EkfSlam.stream_upload`` takes it, (lin, ang, idx, ranges, bearings[, m]) with
    lin, ang, m of shape (steps,) and idx, ranges, bearings (steps, stride).  The grid is every pair of `motion_sigmas` x
    `meas_sigmas` (G points); each point is one trajectory of a bank (``set_noise``), all running the same stream from the
    same mean `mean0`, with the diagonal covariance `diag0` -- (n,), or (G, n) in grid order (row-major: motion, then
    measurement), e.g. for a pose block tied to the motion sigma.  Banks hold at most `bank_size` trajectories (default: the
    whole grid in one bank where it fits, else ``sharding.split_banks``' size).  Every bank logs the innovations of the whole
    run and is scored by ``nis_consistency`` once.  `config` is the handles' EkfConfig (its sigmas are replaced by the grid);
    `filter_factory(n_max, batch, device, config)` makes the banks (default ``EkfSlam``).

    `start` = ``(filter, b)`` or ``filter`` (b = 0) starts every grid point from trajectory b of a RUNNING filter on the same
    device instead -- tune the localisation phase of a run from the dense map its mapping phase built: every bank takes the
    state into its slot 0 with ``copy_from(filter, b, 0)`` and forks it to the rest (``fork(0)``), on the device.  `mean0`
    and `diag0` may then be None (they are not used), and `n_max` defaults to the start filter's."""
    from . import sharding
    from .ekf_bindings import EkfConfig, EkfSlam
    if isinstance(stream, dict):
        stream = tuple(stream[k] for k in ("lin", "ang", "idx", "ranges", "bearings")) + (stream.get("m"),)
    if len(stream) not in (5, 6):
        raise ValueError("tune_noise: stream is (lin, ang, idx, ranges, bearings[, m])")
    lin, ang = np.asarray(stream[0], dtype=float).reshape(-1), np.asarray(stream[1], dtype=float).reshape(-1)
    steps = lin.shape[0]
    idx = np.asarray(stream[2], dtype=np.int32).reshape(steps, -1)
    zr = np.asarray(stream[3], dtype=float).reshape(idx.shape)
    zb = np.asarray(stream[4], dtype=float).reshape(idx.shape)
    m = None if len(stream) < 6 or stream[5] is None else np.asarray(stream[5], dtype=np.int32).reshape(steps)
    ms_grid = np.asarray(motion_sigmas, dtype=float).reshape(-1)
    qs_grid = np.asarray(meas_sigmas, dtype=float).reshape(-1)
    Gm, Gq = len(ms_grid), len(qs_grid)
    G = Gm * Gq
    if G == 0 or steps == 0:
        raise ValueError("tune_noise: an empty grid or stream")
    start_f = start_b = None
    if start is not None:
        start_f, start_b = start if isinstance(start, tuple) else (start, 0)
        start_b = int(start_b)
        n = int(start_f.n_max)
    else:
        mean0 = np.asarray(mean0, dtype=float).reshape(-1)
        n = mean0.shape[0]
        diag0 = np.asarray(diag0, dtype=float)
        if diag0.shape == (n,):
            diag0 = np.broadcast_to(diag0, (G, n))
        elif diag0.shape != (G, n):
            raise ValueError(f"tune_noise: diag0 must be shaped ({n},) or ({G}, {n}), got {diag0.shape}")
    n_max = n if n_max is None else int(n_max)
    pm = np.repeat(ms_grid, Gq)                          # grid point g = (motion index g // Gq, measurement index g % Gq)
    pq = np.tile(qs_grid, Gm)
    if bank_size is None:
        per = 8 * (n_max * n_max + 2 * 160 * n_max)      # a trajectory's covariance and pending factors, roughly
        bank_size = G if G * per <= _TUNE_BANK_BYTES else 32
    banks = sharding.split_banks(list(range(G)), int(bank_size))
    cfg = config if config is not None else EkfConfig()
    make = filter_factory or (lambda n_max_, batch, dev, c: EkfSlam(n_max_, batch=batch, device=dev, config=c))
    loglik, anis = np.empty(G), np.empty(G)
    bounds = np.empty((G, 2))
    for ids in banks:
        B = len(ids)
        f = make(n_max, B, device, cfg)
        try:
            f.set_noise(pm[ids], pq[ids])
            if start_f is not None:
                f.copy_from(start_f, start_b, 0)
                f.fork(0)
            else:
                for k, g in enumerate(ids):
                    f.set_state_diag(mean0, diag0[g], k)
            f.log_innovations(steps)
            f.stream_upload(np.repeat(lin[:, None], B, 1), np.repeat(ang[:, None], B, 1),
                            np.repeat(idx[:, None, :], B, 1), np.repeat(zr[:, None, :], B, 1), np.repeat(zb[:, None, :], B, 1),
                            None if m is None else np.repeat(m[:, None], B, 1))
            f.stream_run(0, steps)
            nc = nis_consistency(f.innovations(0, steps), confidence)
        finally:
            f.close()
        loglik[ids], anis[ids], bounds[ids] = nc.loglik, nc.traj_anis, nc.traj_bounds
    g_best = int(np.nanargmax(loglik))
    return NoiseTuning(ms_grid, qs_grid, loglik.reshape(Gm, Gq), anis.reshape(Gm, Gq), bounds.reshape(Gm, Gq, 2),
                       (float(pm[g_best]), float(pq[g_best])), tuple(len(b) for b in banks))


class AssociationFlag(NamedTuple):
    """One labelled observation `association_check` reports."""
    b: int                # trajectory
    q: int                # observation number in its list
    labelled: int         # the landmark its label names
    best: int             # the landmark of the smallest score d = NIS + ln det S (-1: none)
    d_labelled: float     # the labelled landmark's score
    d_other: float        # the smallest score of any OTHER landmark (inf: there is none)


def association_check(f, idx, ranges, bearings, margin: float = 0.0):
    """Labelled observations against the filter's own likelihood (``f.associate(..., full=True)``: one device query, no
    covariance pass, nothing of the filter changes): reports every observation whose labelled landmark is not the best
    candidate, or whose lead in d = NIS + ln det S over the best OTHER landmark is below ``margin`` -- a misread tag id, or a
    label that the geometry cannot tell from its neighbour.  ``idx`` / ``ranges`` / ``bearings``: as ``EkfSlam.update``
    takes them (one list per trajectory, a flat list for a single trajectory, or (B, m) arrays).  Returns a list of
    ``AssociationFlag`` in (trajectory, observation) order; empty: every label is the clear best."""
    B = f.batch
    if isinstance(idx, np.ndarray) and idx.ndim == 2:
        idx, ranges, bearings = list(idx), list(np.asarray(ranges)), list(np.asarray(bearings))
    elif B == 1 and (len(idx) == 0 or np.ndim(idx[0]) == 0):
        idx, ranges, bearings = [idx], [ranges], [bearings]
    if len(idx) != B:
        raise ValueError("association_check: one list per trajectory expected")
    a = f.associate([list(r) for r in ranges], [list(z) for z in bearings], full=True)
    d = a.all_nis + a.all_logdet
    flags = []
    for b in range(B):
        n_lm = d.shape[2]
        for q, j in enumerate(idx[b]):
            j = int(j)
            if not 0 <= j < n_lm or np.isnan(d[b, q, j]):
                raise ValueError(f"association_check: trajectory {b}: label {j} names no landmark of the map")
            others = np.delete(d[b, q], j)
            others = others[~np.isnan(others)]
            d_other = float(others.min()) if others.size else math.inf
            best = int(a.cand[b, q, 0])
            if best != j or d_other - d[b, q, j] < margin:
                flags.append(AssociationFlag(b, q, j, best, float(d[b, q, j]), d_other))
    return flags


def landmark_separation(f, pairs, b: int = 0):
    """How far apart are landmarks i and j of trajectory b, and is that significant?  For index pairs ``(i, j)`` returns
    ``(distance (K,), sigma (K,), mahalanobis (K,))``: the Euclidean distance of the two means, its first-order standard
    deviation from the 4 x 4 joint covariance of the two landmarks (the cross-covariance included -- two landmarks mapped
    from the same poses are far better known relative to each other than their marginals say), and the Mahalanobis
    separation  d^T (P_ii + P_jj - P_ij - P_ji)^-1 d,  d = l_i - l_j  (chi-square with 2 degrees of freedom if both were
    the same landmark: the test a duplicate-landmark detector needs).  Read-only: ``EkfSlam.joint`` calls over the distinct
    landmarks, EKF_JMAX // 2 pairs at a time; no covariance pass."""
    from .ekf_bindings import EKF_JMAX
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    K = pairs.shape[0]
    dist, sigma, maha = np.empty(K), np.empty(K), np.empty(K)
    per = EKF_JMAX // 2
    for k0 in range(0, K, per):
        chunk = pairs[k0:k0 + per]
        lms = sorted({int(x) for x in chunk.ravel()})
        place = {j: 3 + 2 * p for p, j in enumerate(lms)}
        mean, cov = f.joint(lms, b)
        for t, (i, j) in enumerate(chunk):
            if i == j:
                raise ValueError(f"landmark_separation: pair ({i}, {j}) names one landmark twice")
            a, c = place[int(i)], place[int(j)]
            s = [a, a + 1, c, c + 1]
            P4 = cov[np.ix_(s, s)]
            d = mean[a:a + 2] - mean[c:c + 2]
            r = float(np.hypot(d[0], d[1]))
            D = np.array([[1.0, 0.0, -1.0, 0.0], [0.0, 1.0, 0.0, -1.0]])
            Pd = D @ P4 @ D.T                                  # P_ii + P_jj - P_ij - P_ji
            with np.errstate(divide="ignore", invalid="ignore"):
                g = d / r                                      # gradient of |d| by d
            dist[k0 + t] = r
            sigma[k0 + t] = math.sqrt(max(float(g @ Pd @ g), 0.0)) if r > 0.0 else float("nan")
            maha[k0 + t] = float(d @ np.linalg.solve(Pd, d))
    return dist, sigma, maha
