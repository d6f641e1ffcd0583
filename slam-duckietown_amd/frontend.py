"""Host-side front end of one EKF step: what stays on the CPU.

Association / range gate / averaging of the AprilTag detections of one window, and the wheel
odometry scalars.  O(#detections) Python, mirrors the reference's semantics exactly:

  associate      src/replay_no_ros.py:280-337
  delta_phi      src/replay_no_ros.py:250-266
  displacement   src/replay_no_ros.py:484-497

`associate_known` is `associate` against a frozen map (localisation mode: unknown tags are reported, never added).
`resolve_associations` has no counterpart in the reference (which trusts tag ids): it turns the candidates the device's
likelihood query (``EkfSlam.associate``) returns for one trajectory's unlabelled observations into an assignment.
"""
from __future__ import annotations

import math
from typing import Dict, List, Sequence, Tuple

import numpy as np


def delta_phi(ticks: int, prev_ticks: int, resolution: int) -> float:
    """Wheel rotation in radians for an encoder tick difference (replay_no_ros.py:262-264)."""
    return (ticks - prev_ticks) * (2 * np.pi / resolution)


def displacement(R: float, baseline: float, delta_phi_left: float, delta_phi_right: float) -> Tuple[float, float]:
    """(angular, linear) displacement of a differential drive (replay_no_ros.py:491-497)."""
    right = R * delta_phi_right
    left = R * delta_phi_left
    return (right - left) / baseline, (left + right) / 2


def associate(detections, tag_index: Dict[int, int], pose, gate_range: float = 1.5,
              ignore_tags: Sequence[int] = ()):
    """Tag id -> landmark index, 1.5 m gate, per-tag averaging over the window's frames.

    ``detections`` is the reference's ``[(timestamp, [tag, ...])]`` list; a tag needs ``tag_id``,
    ``pose_t`` (3,1) and ``pose_err``.  ``tag_index`` is mutated (new ids get the next index,
    :294-295).  Returns ``{landmark_index: [xw, yw, err, tag_id, range, bearing]}`` in order of
    first appearance -- which is the order the update processes them in (:436).
    The world-frame guess uses ``pose`` BEFORE the prediction (:331-332).
    """
    # Sums instead of lists of arrays: `np.mean(list_of_(3,1)_arrays, axis=0)` (:315) adds the frames in order and divides by
    # their number -- the same additions, in the same order, on Python floats (only pose_t[0] and pose_t[2] are ever used,
    # :321); the errors are averaged the same way up to 7 detections (NumPy sums short 1-D arrays sequentially; from 8 on it
    # sums pairwise, and np.mean itself is called to stay bit-identical).  What costs time here is Python, not arithmetic:
    # this function is a third of a drop-in call at the reference's map size.
    gate2 = gate_range ** 2
    seen: Dict[int, List] = {}
    for _stamp, tags in detections:
        for tag in tags:
            tid = tag.tag_id
            if tid in ignore_tags:
                continue
            t = tag.pose_t
            tx, tz = float(t[0][0]), float(t[2][0])
            if tz * tz + tx * tx > gate2:
                continue
            lm = tag_index.get(tid)
            if lm is None:
                lm = tag_index[tid] = len(tag_index)
            acc = seen.get(lm)
            if acc is None:
                seen[lm] = [tx, tz, [tag.pose_err], tid]
            else:
                acc[0] += tx
                acc[1] += tz
                acc[2].append(tag.pose_err)
    return _averaged(seen, pose)


def _averaged(seen, pose):
    """What ``associate`` and ``associate_known`` return for the window's sums ``{landmark: [sum tx, sum tz, errs, tag id]}``."""
    x0, y0, th = float(pose[0]), float(pose[1]), float(pose[2])
    result = {}
    for lm, (sx, sz, errs, tid) in seen.items():
        k = len(errs)
        if k < 8:
            e = errs[0]
            for v in errs[1:]:
                e = e + v
            err = np.float64(e) / k
        else:
            err = np.mean(errs, axis=0)
        x_r, y_r = np.float64(sz / k), np.float64(-(sx / k))
        rng = np.sqrt(x_r ** 2 + y_r ** 2)
        brg = np.arctan2(y_r, x_r)
        result[lm] = [x0 + rng * np.cos(brg + th), y0 + rng * np.sin(brg + th), err, tid, rng, brg]
    return result


def associate_known(detections, tag_index: Dict[int, int], pose, gate_range: float = 1.5,
                    ignore_tags: Sequence[int] = (), n_landmarks=None):
    """``associate`` against a FROZEN map (localisation): ``tag_index`` is read, never written.  A tag it does not hold -- or,
    with ``n_landmarks`` given, one whose index lies at or beyond it -- is unmatched: it takes no part and its id is recorded.
    Ignored tags and tags beyond the gate are dropped before that, as in ``associate`` (:286-289).

    Returns ``(tags, unmatched)``: ``tags`` as ``associate`` returns them, with the same numbers (the same sums in the same
    order), and the distinct unmatched ids in order of first appearance."""
    gate2 = gate_range ** 2
    seen: Dict[int, List] = {}
    unmatched: List[int] = []
    for _stamp, tags in detections:
        for tag in tags:
            tid = tag.tag_id
            if tid in ignore_tags:
                continue
            t = tag.pose_t
            tx, tz = float(t[0][0]), float(t[2][0])
            if tz * tz + tx * tx > gate2:
                continue
            lm = tag_index.get(tid)
            if lm is None or (n_landmarks is not None and lm >= n_landmarks):
                if tid not in unmatched:
                    unmatched.append(tid)
                continue
            acc = seen.get(lm)
            if acc is None:
                seen[lm] = [tx, tz, [tag.pose_err], tid]
            else:
                acc[0] += tx
                acc[1] += tz
                acc[2].append(tag.pose_err)
    return _averaged(seen, pose), unmatched


def remap_tag_index(tag_index: Dict[int, int], old_to_new) -> Dict[int, int]:
    """TAG_INDEX after ``EkfSlam.remove_landmarks``: the tags of removed landmarks (``old_to_new[j] == -1``) dropped, every
    other tag renumbered -- values stay 0..len-1 in first-sighting order.  For callers that keep their own TAG_INDEX with
    ``associate``; a removed tag seen again gets the next index, a new landmark."""
    o2n = np.asarray(old_to_new)
    out = {}
    for tag, j in tag_index.items():
        if not 0 <= j < len(o2n):
            raise ValueError(f"remap_tag_index: landmark index {j} of tag {tag} outside old_to_new ({len(o2n)} landmarks)")
        if o2n[j] >= 0:
            out[tag] = int(o2n[j])
    return out


def resolve_associations(cand, nis, min_nis, accept: float, create: float):
    """One trajectory's unlabelled observations -> landmarks, from what ``EkfSlam.associate`` returns for it: ``cand``
    (m, 2) the two best landmarks of every observation (best first, -1: none), ``nis`` (m, 2) their NIS, ``min_nis`` (m,) the
    smallest NIS over all landmarks.

    Greedy, one landmark per observation: the observations are taken in ascending order of their best candidate's NIS
    (stable sort; NaN last) and each takes its first candidate that no earlier one took.  It is ACCEPTED when that
    candidate's NIS <= ``accept``.  Otherwise -- also when both its candidates are taken -- it is a NEW landmark when it
    fits nothing at all (``min_nis > create``, or the map is empty), else it is DROPPED as ambiguous: too far from its
    candidate to update with, too close to some landmark to start another.

    Returns ``(assign, new_obs, dropped_obs)``: ``assign`` (m,) int64, the landmark of every accepted observation and -1 for
    the others; the observation numbers of the new and of the dropped ones, ascending."""
    cand = np.asarray(cand, dtype=np.int64).reshape(-1, 2)
    nis = np.asarray(nis, dtype=np.float64).reshape(-1, 2)
    min_nis = np.asarray(min_nis, dtype=np.float64).reshape(-1)
    m = cand.shape[0]
    assign = np.full(m, -1, dtype=np.int64)
    new_obs: List[int] = []
    dropped: List[int] = []
    taken = set()
    for q in np.argsort(nis[:, 0], kind="stable"):
        q = int(q)
        pick = next((c for c in range(2) if cand[q, c] >= 0 and int(cand[q, c]) not in taken), None)
        if pick is not None and nis[q, pick] <= accept:
            assign[q] = cand[q, pick]
            taken.add(int(cand[q, pick]))
        elif cand[q, 0] < 0 or min_nis[q] > create:
            new_obs.append(q)
        else:
            dropped.append(q)
    return assign, sorted(new_obs), sorted(dropped)


def fit_transform(src_xy, dst_xy, weights=None):
    """The rigid transform without scale ``T = (x, y, phi)`` that minimises ``sum_i w_i |dst_i - (t + R(phi) src_i)|^2``, and
    its covariance: ``(T (3,), cov (3, 3))``.  ``T`` is the frame of ``src`` expressed in the frame of ``dst`` -- what
    ``EkfSlam.transform`` and ``EkfSlam.join(transform=)`` take.  Closed form: weighted centroids c_s, c_d, then on the centred
    points a_i, b_i ``phi = atan2(sum w a x b, sum w a . b)``, then ``t = c_d - R c_s``.  ``cov = (sum_i w_i A_i^T A_i)^-1``
    with ``A_i = [I2 | J2 R src_i]``: the estimate's covariance when ``dst_i`` carries noise ``I / w_i``.  ``weights`` None:
    all one.  ``ValueError`` for unequal lengths, non-finite input, negative weights, or fewer than two distinct points of
    positive weight (the rotation is then undetermined)."""
    src = np.asarray(src_xy, dtype=np.float64)
    dst = np.asarray(dst_xy, dtype=np.float64)
    if src.ndim != 2 or src.shape[1] != 2 or dst.ndim != 2 or dst.shape[1] != 2:
        raise ValueError("fit_transform: (k, 2) arrays expected")
    if src.shape[0] != dst.shape[0]:
        raise ValueError(f"fit_transform: src and dst must have the same length, got {src.shape[0]} and {dst.shape[0]}")
    w = np.ones(src.shape[0]) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    if w.shape[0] != src.shape[0]:
        raise ValueError("fit_transform: one weight per point expected")
    if not (np.isfinite(src).all() and np.isfinite(dst).all() and np.isfinite(w).all()):
        raise ValueError("fit_transform: non-finite input")
    if (w < 0).any():
        raise ValueError("fit_transform: negative weight")
    used = w > 0
    if len({(float(p[0]), float(p[1])) for p in src[used]}) < 2 or len({(float(p[0]), float(p[1])) for p in dst[used]}) < 2:
        raise ValueError("fit_transform: at least two distinct points are needed")
    W = w.sum()
    cs, cd = (w[:, None] * src).sum(0) / W, (w[:, None] * dst).sum(0) / W
    a, b = src - cs, dst - cd
    phi = math.atan2(float((w * (a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0])).sum()), float((w * (a * b).sum(1)).sum()))
    c, s = math.cos(phi), math.sin(phi)
    R = np.array([[c, -s], [s, c]])
    t = cd - R @ cs
    rs = src @ R.T                                                 # R src_i
    g = np.stack([-rs[:, 1], rs[:, 0]], axis=1)                    # J2 R src_i
    info = np.zeros((3, 3))
    info[0, 0] = info[1, 1] = W
    info[:2, 2] = info[2, :2] = (w[:, None] * g).sum(0)
    info[2, 2] = (w * (g * g).sum(1)).sum()
    cov = np.linalg.inv(info)
    return np.array([t[0], t[1], phi]), (cov + cov.T) / 2          # (exactly symmetric)


def wrap_pi(a):
    """(a + pi) % 2 pi - pi with NumPy remainder semantics, [-pi, pi): how the device wraps a bearing residual."""
    return (a + np.pi) % (2.0 * np.pi) - np.pi


def poses_on_circle(landmark_xy, range_, bearing, count: int) -> np.ndarray:
    """The ``count`` poses (count, 3) consistent with ONE range/bearing sighting of a landmark at a known position: positions on
    the circle of radius ``range_`` around it, headings evenly spaced over [-pi, pi) -- heading theta puts the robot at
    landmark - range (cos(theta + bearing), sin(theta + bearing)).  The seeding of a kidnapped robot's hypotheses
    (``HypothesisBank.reset``); neighbours are 2 pi / count apart in heading."""
    count = int(count)
    if count < 1:
        raise ValueError("poses_on_circle: count must be >= 1")
    lm = np.asarray(landmark_xy, dtype=np.float64).reshape(2)
    th = -np.pi + 2.0 * np.pi * np.arange(count) / count
    a = th + float(bearing)
    return np.stack([lm[0] - float(range_) * np.cos(a), lm[1] - float(range_) * np.sin(a), th], axis=1)


def measurement_h(pose, landmark_xy):
    """Range/bearing model of one landmark seen from ``pose`` (x, y, theta): ``(zhat (2,), H5 (2, 5))``, the predicted
    observation and its Jacobian on (x, y, theta, lx, ly) -- src/replay_no_ros.py:443-469 as the device evaluates them
    (a landmark at the pose's position gives NaN / inf like the reference's 0/0)."""
    pose = np.asarray(pose, dtype=np.float64)
    lm = np.asarray(landmark_xy, dtype=np.float64)
    dx, dy = lm[0] - pose[0], lm[1] - pose[1]                      # :443
    q = dx * dx + dy * dy                                          # :446
    sq = np.sqrt(q)
    zhat = np.array([sq, np.arctan2(dy, dx) - pose[2]])            # :451-454
    with np.errstate(divide="ignore", invalid="ignore"):
        h5 = np.array([[-sq * dx, -sq * dy, 0.0, sq * dx, sq * dy],
                       [dy, -dx, -q, -dy, dx]], dtype=np.float64) / q    # :466-469
    return zhat, h5


def joint_compatibility(ranges, bearings, candidates, sel, mean, cov, meas_var, confidence: float = 0.99,
                        max_nodes: int = 20000):
    """Joint-compatibility branch and bound (Neira & Tardos) for one trajectory's unlabelled observations.

    ``candidates[q]`` lists the landmarks individually plausible for observation q, best first; all are members of ``sel``,
    the landmark list ``EkfSlam.joint(sel, b)`` returned ``mean`` and ``cov`` for (sub-state [x, y, theta, l_sel0, ...]).
    ``meas_var`` (2,) is the diagonal of the trajectory's Q: ``noise()[1][b] ** 2`` twice.

    Depth first over the observations in order; each tries its candidates that no earlier one holds, in the given order,
    then "unmatched".  A hypothesis with p pairings is feasible when its joint NIS  y^T (H cov H^T + I_p (x) Q)^-1 y  --
    all innovations stacked, bearings wrapped, H the rows of ``measurement_h`` scattered to the sub-state's columns -- is
    <= the chi-square quantile of 2p degrees of freedom at ``confidence``; individually plausible pairings that share one
    pose error the wrong way fail it.  Two cuts, both exact: a branch whose pairings plus the observations left stay below
    the best count of pairings, and a branch whose joint NIS already exceeds the quantile of the most pairings it can still
    reach (adding pairings never lowers a joint NIS).  The best hypothesis has the most pairings, then the smaller joint
    NIS, then is the first found.

    Returns ``(assign (m,) int64 landmark or -1, joint_nis, exhausted)``; ``exhausted`` is False when ``max_nodes`` -- a
    guard against 3^16 worst cases -- ended the search, the best hypothesis so far is still returned."""
    from scipy.stats import chi2
    ranges = np.asarray(ranges, dtype=np.float64).reshape(-1)
    bearings = np.asarray(bearings, dtype=np.float64).reshape(-1)
    sel = [int(j) for j in np.asarray(sel).reshape(-1)]
    mean = np.asarray(mean, dtype=np.float64)
    cov = np.asarray(cov, dtype=np.float64)
    meas_var = np.asarray(meas_var, dtype=np.float64).reshape(2)
    m = len(ranges)
    ns = 3 + 2 * len(sel)
    place = {j: p for p, j in enumerate(sel)}
    cands = [[int(j) for j in c] for c in candidates]
    if len(cands) != m or len(bearings) != m:
        raise ValueError("joint_compatibility: one candidate list and one bearing per observation expected")
    for c in cands:
        for j in c:
            if j not in place:
                raise ValueError(f"joint_compatibility: candidate {j} is not a member of sel")
    # every (observation, candidate) pairing once: its innovation and its two rows of H on the sub-state
    rows = {}
    for q, c in enumerate(cands):
        for j in c:
            t = 3 + 2 * place[j]
            zhat, h5 = measurement_h(mean[:3], mean[t:t + 2])
            H = np.zeros((2, ns))
            H[:, :3] = h5[:, :3]
            H[:, t:t + 2] = h5[:, 3:]
            rows[q, j] = (np.array([ranges[q] - zhat[0], wrap_pi(bearings[q] - zhat[1])]), H)
    limit = [0.0] + [float(chi2.ppf(confidence, 2 * p)) for p in range(1, m + 1)]
    P = cov[:ns, :ns]

    def joint_nis(pairs):
        if not pairs:
            return 0.0
        y = np.concatenate([rows[p][0] for p in pairs])
        H = np.vstack([rows[p][1] for p in pairs])
        S = H @ P @ H.T + np.diag(np.tile(meas_var, len(pairs)))
        return float(y @ np.linalg.solve(S, y))

    best = {"pairs": None, "nis": 0.0}
    nodes = [0]
    exhausted = [True]

    def descend(q, pairs, nis):
        if q == m:
            if not nis <= limit[len(pairs)]:                 # (a NaN is infeasible)
                return
            if best["pairs"] is None or len(pairs) > len(best["pairs"]) or (len(pairs) == len(best["pairs"]) and nis < best["nis"]):
                best["pairs"], best["nis"] = list(pairs), nis
            return
        if best["pairs"] is not None and len(pairs) + (m - q) < len(best["pairs"]):   # cannot reach the best count any more
            return
        used = {j for _, j in pairs}
        for j in cands[q] + [-1]:
            if j in used:
                continue
            if nodes[0] >= max_nodes:
                exhausted[0] = False
                return
            nodes[0] += 1
            if j < 0:
                descend(q + 1, pairs, nis)
            else:
                pairs.append((q, j))
                v = joint_nis(pairs)
                if v <= limit[len(pairs) + (m - q - 1)]:     # some completion may still be feasible
                    descend(q + 1, pairs, v)
                pairs.pop()
            if not exhausted[0]:
                return

    descend(0, [], 0.0)
    assign = np.full(m, -1, dtype=np.int64)
    for q, j in best["pairs"] or []:
        assign[q] = j
    return assign, best["nis"], exhausted[0]
