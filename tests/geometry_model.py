"""The scalar geometry of one filter step -- motion model, range/bearing linearisation, wrapped innovation -- and one dense
sequential step built on it, restated in np.longdouble (x87 extended: 64-bit significand, eps 1.1e-19), plus the judge the CPU and
GPU geometry tests share.  NumPy only; a plain module.

The restatement follows oracle.ekf_oracle line by line (motion_model, innovation_and_h5, predict_dense, update_dense) with three
differences: every operand is a longdouble, pi is a 36-digit literal rather than the float64 one, and the 2 x 2 inverse is written
out (np.linalg does not take longdouble).  The remainder keeps orc.wrap_pi's semantics: (a + pi) % 2 pi - pi with NumPy's floored
remainder, into [-pi, pi).  What a float64 implementation loses against it is therefore its own rounding plus k (2 pi_d - 2 pi)
for a wrap across k turns (2.4e-16 a turn: 3.9e-14 at theta = -1000).
"""
import numpy as np

LD = np.longdouble
PI = LD("3.14159265358979323846264338327950288")
TWO_PI = 2 * PI


def ld(a):
    return np.array(a, dtype=LD)


def wrap_pi(a):
    """orc.wrap_pi in longdouble: floored remainder, [-pi, pi)."""
    return (LD(a) + PI) % TWO_PI - PI


def motion_model(pose, lin, ang, cfg):
    """orc.motion_model (src/replay_no_ros.py:368-417): (new pose (3,), G (3, 3)), theta read before the update."""
    pose = ld(pose)
    lin, ang, thr = LD(lin), LD(ang), LD(cfg.arc_threshold)
    th = pose[2]
    G = np.eye(3, dtype=LD)
    new = pose[:3].copy()
    if cfg.disable_motion_model:                                   # :372-373
        return new, G
    if cfg.enable_circular_interpolation:
        if abs(ang) <= thr:                                        # :376 straight, theta NOT advanced
            new[0] += lin * np.cos(th)
            new[1] += lin * np.sin(th)
            G[0, 2] = -lin * np.sin(th)
            G[1, 2] = lin * np.cos(th)
        else:                                                      # :390 arc
            r = lin / ang
            new[0] += -r * np.sin(th) + r * np.sin(th + ang)
            new[1] += r * np.cos(th) - r * np.cos(th + ang)
            new[2] = wrap_pi(th + ang)                             # :397
            G[0, 2] = -r * np.cos(th) + r * np.cos(th + ang)       # :401
            G[1, 2] = -r * np.sin(th) + r * np.sin(th + ang)       # :402
    else:                                                          # :405-417 no wrap
        new[0] += lin * np.cos(th)
        new[1] += lin * np.sin(th)
        new[2] = th + ang
        G[0, 2] = -lin * np.sin(th)
        G[1, 2] = lin * np.cos(th)
    return new, G


def unwrapped_residual(pose3, lm2, z_bearing):
    """z_b - (atan2(d) - theta) before the wrap (:453-455): what must keep clear of the odd multiples of pi."""
    pose3, lm2 = ld(pose3), ld(lm2)
    d = lm2 - pose3[0:2]
    return LD(z_bearing) - (np.arctan2(d[1], d[0]) - pose3[2])


def innovation_and_h5(pose3, lm2, z_range, z_bearing):
    """orc.innovation_and_h5 (:443-469): (y (2,), h5 (2, 5)) on {x, y, theta, lx, ly}."""
    pose3, lm2 = ld(pose3), ld(lm2)
    d = lm2 - pose3[0:2]
    q = d[0] * d[0] + d[1] * d[1]
    sq = np.sqrt(q)
    y = ld([LD(z_range) - sq, wrap_pi(LD(z_bearing) - (np.arctan2(d[1], d[0]) - pose3[2]))])
    h5 = ld([[-sq * d[0], -sq * d[1], LD(0), sq * d[0], sq * d[1]], [d[1], -d[0], -q, -d[1], d[0]]]) / q
    return y, h5


def inv2(S):
    det = S[0, 0] * S[1, 1] - S[0, 1] * S[1, 0]
    return ld([[S[1, 1], -S[0, 1]], [-S[1, 0], S[0, 0]]]) / det


def predict(mean, cov, lin, ang, cfg):
    """orc.predict_dense (:420-430); G only mixes the pose's rows and columns."""
    mean, cov = ld(mean), ld(cov)
    pose, G = motion_model(mean[0:3], lin, ang, cfg)
    if not cfg.disable_motion_model:
        mean[0:3] = pose
    cov[0:3, :] = G @ cov[0:3, :]
    cov[:, 0:3] = cov[:, 0:3] @ G.T
    rd = ld(cfg.motion_noise_diag())
    for i in range(3):
        cov[i, i] += rd[i]
    return mean, cov


def scores(mean, cov, j, z_range, z_bearing, cfg):
    """One observation against landmark j at the state given: (y, S, NIS, h5, H P)."""
    t = 3 + 2 * int(j)
    sel = [0, 1, 2, t, t + 1]
    y, h5 = innovation_and_h5(mean[0:3], mean[t:t + 2], z_range, z_bearing)
    HP = h5 @ cov[sel, :]
    S = HP[:, sel] @ h5.T
    Qd = ld(cfg.meas_noise_diag())
    S[0, 0] += Qd[0]
    S[1, 1] += Qd[1]
    Si = inv2(S)
    return y, S, y @ Si @ y, h5, HP


def update(mean, cov, obs, cfg, log=None):
    """orc.update_dense (:436-480), sequential; appends (j, y, S, NIS, h5) per observation to `log`.  K = P H^T S^-1 from the columns,
    (I - K H) P from the rows, as the reference forms them."""
    mean, cov = ld(mean), ld(cov)
    for j, zr, zb in obs:
        t = 3 + 2 * int(j)
        sel = [0, 1, 2, t, t + 1]
        y, S, nis, h5, HP = scores(mean, cov, j, zr, zb, cfg)
        K = cov[:, sel] @ h5.T @ inv2(S)
        mean = mean + K @ y
        cov = cov - K @ HP
        if log is not None:
            log.append((int(j), y, S, nis, h5))
    return mean, cov


class StepRecord:
    """What one step leaves for the judge: the observations' (j, y, S, NIS, h5), the pose after the prediction, the pose and its
    block after the step, and the conditions' raw material (theta + ang where the arc branch wraps it, the unwrapped bearing
    residuals, the ranges sqrt(q) the updates saw)."""

    def __init__(self):
        self.obs, self.residuals, self.ranges = [], [], []
        self.predicted = self.predicted_block = self.pose = self.block = self.theta_sum = None


def wraps_theta(ang, cfg):
    """The step's theta goes through the wrap (:397): the arc branch."""
    return (not cfg.disable_motion_model) and cfg.enable_circular_interpolation and abs(ang) > cfg.arc_threshold


def step(mean, cov, lin, ang, obs, cfg, rec=None):
    """predict + update (orc.ekf_step_dense)."""
    th0 = LD(mean[2])
    mean, cov = predict(mean, cov, lin, ang, cfg)
    if rec is not None:
        rec.predicted, rec.predicted_block = mean[0:3].copy(), cov[0:3, 0:3].copy()
        rec.theta_sum = th0 + LD(ang) if wraps_theta(ang, cfg) else None
    if cfg.enable_measurement_model:
        for o in obs:
            if rec is not None:
                t = 3 + 2 * int(o[0])
                rec.residuals.append(unwrapped_residual(mean[0:3], mean[t:t + 2], o[2]))
                d = mean[t:t + 2] - mean[0:2]
                rec.ranges.append(np.sqrt(d[0] * d[0] + d[1] * d[1]))
            mean, cov = update(mean, cov, [o], cfg, rec.obs if rec is not None else None)
    if rec is not None:
        rec.pose, rec.block = mean[0:3].copy(), cov[0:3, 0:3].copy()
    return mean, cov


class Reference:
    """A script through the model: the final state, a StepRecord per step, and what the judge needs to know of the script."""

    def __init__(self, mean, cov, recs, exact, init_var):
        self.mean, self.cov, self.recs, self.exact, self.init_var = mean, cov, recs, exact, init_var


def run(script):
    """A whole script (tests/geometry_cases.py) -> Reference."""
    mean, cov, recs = ld(script.mean0), ld(script.cov0), []
    for lin, ang, obs in script.steps:
        rec = StepRecord()
        mean, cov = step(mean, cov, lin, ang, obs, script.cfg, rec)
        recs.append(rec)
    return Reference(mean, cov, recs, script.exact, script.cfg.landmark_init_var)


def localize_reference(script):
    """The script as localisation on its frozen start map, through tests/localize_model.py (float64, Joseph form) fed the script's
    inputs: a Reference the judge takes."""
    from tests import localize_model as lm
    mean, cov, recs = script.mean0.copy(), script.cov0.copy(), []
    for lin, ang, obs in script.steps:
        log, rec = [], StepRecord()
        mean, cov = lm.literal_step(mean, cov, lin, ang, [o[0] for o in obs], [o[1] for o in obs], [o[2] for o in obs], script.cfg,
                                    log=log)
        rec.obs = [(j, ld(y), ld(S), LD(nis), None) for j, y, S, nis, _ in log]
        rec.pose, rec.block = ld(mean[0:3]), ld(cov[0:3, 0:3])
        recs.append(rec)
    return Reference(mean, cov, recs, script.exact, script.cfg.landmark_init_var)


def associate_scores(mean, cov, ranges, bearings, cfg):
    """EkfSlam.associate(full=True) at the state given, every observation against every landmark: (NIS (S, N), ln det S (N,),
    wrapped bearing residual (S, N))."""
    mean, cov = ld(mean), ld(cov)
    N = (len(mean) - 3) // 2
    nis = np.zeros((len(ranges), N), dtype=LD)
    logdet = np.zeros(N, dtype=LD)
    res = np.zeros((len(ranges), N), dtype=LD)
    for l in range(N):
        for q, (zr, zb) in enumerate(zip(ranges, bearings)):
            y, S, v, _, _ = scores(mean, cov, l, zr, zb, cfg)
            nis[q, l] = v
            res[q, l] = y[1]
            logdet[l] = np.log(S[0, 0] * S[1, 1] - S[0, 1] * S[1, 0])
    return nis, logdet, res


def pi_margin(a):
    """Distance of an angle from the nearest odd multiple of pi."""
    return float(PI - abs(wrap_pi(a)))


# ---- the judge -------------------------------------------------------------------------------------------------------------------
class Run:
    """One script on one path, as the judge takes it: per step the list of (j, y (2,), S (2, 2), NIS[, h5 (2, 5)]) and the pose
    row (mean (3,), block (3, 3)); the final (mean, cov) and the flags."""

    def __init__(self, obs, poses, mean, cov, flags=0):
        self.obs, self.poses, self.mean, self.cov, self.flags = obs, poses, mean, cov, flags


FIGURES = ("y", "S", "nis", "H", "pose", "pose_block", "state", "state_entry")


def _relm(got, want):
    got, want = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD)
    den = np.sqrt(np.sum(want * want))
    num = np.sqrt(np.sum((got - want) ** 2))
    return float(num / den) if den > 0 else float(num)


def distances(run, ref, range_relative=False):
    """Worst distances of `run` from the model: ({figure: value}, [what cannot be compared at all]).

    y: absolute, both components (`range_relative`: the range component over the range the update saw -- the CPU conditions);
    S: relative Frobenius per 2 x 2 block; H: the same per 2 x 2 block of h5 (pose x, y; landmark x, y), its theta column exactly;
    NIS: relative; pose: absolute per entry; pose_block: relative Frobenius of the 3 x 3 block;
    state: the largest block piece of parity_blocks.state_errors on the final mean and covariance (pose block, cross rows, landmark
    block, pose mean, over the pose and the informed landmarks); state_entry: its per-entry maxima (corr_max, mean_landmarks and the
    loose landmarks' cross terms), which parity_blocks bounds apart from the blocks; the loose landmarks' own rules are asserted
    here.
    A script whose last observation is an exact-boundary one (`ref.exact`): that y_1 is compared modulo 2 pi and must lie in
    [-pi_d, pi_d); its S and NIS, the script's last pose row and the final state are not compared."""
    from tests.parity_blocks import PIECES, state_errors
    w = {k: 0.0 for k in FIGURES}
    bad = []
    K = len(ref.recs)
    if len(run.obs) != K or len(run.poses) != K:
        return w, [f"{len(run.obs)} logged steps and {len(run.poses)} pose rows where the script has {K} steps"]
    if run.flags != 0:
        bad.append(f"flags {run.flags:#x}")
    for k, rec in enumerate(ref.recs):
        last_step = ref.exact and k == K - 1
        if [int(o[0]) for o in run.obs[k]] != [o[0] for o in rec.obs]:
            bad.append(f"step {k}: landmarks {[int(o[0]) for o in run.obs[k]]} logged where the model applied {[o[0] for o in rec.obs]}")
            continue
        for i, (got, (_, my, mS, mnis, mh)) in enumerate(zip(run.obs[k], rec.obs)):
            y, S, nis = got[1], got[2], got[3]
            e0 = float(abs(LD(y[0]) - my[0]))
            if range_relative:
                e0 /= float(rec.ranges[i])
            if last_step and i == len(rec.obs) - 1:
                y1 = float(y[1])
                if not -np.pi <= y1 < np.pi:
                    bad.append(f"step {k} obs {i}: the exact-boundary y_1 = {y1!r} lies outside [-pi, pi)")
                w["y"] = max(w["y"], e0, float(abs(wrap_pi(LD(y1) - my[1]))))
                continue
            w["y"] = max(w["y"], e0, float(abs(LD(y[1]) - my[1])))
            w["S"] = max(w["S"], _relm(S, mS))
            w["nis"] = max(w["nis"], float(abs(LD(nis) - mnis) / mnis) if mnis > 0 else float(abs(LD(nis) - mnis)))
            if len(got) > 4:
                # h5's two 2 x 2 blocks, on the pose's x, y and on the landmark's (gated_oracle.block_err's measure; the theta
                # column is 0 and -1 exactly)
                w["H"] = max(w["H"], _relm(np.asarray(got[4])[:, 0:2], mh[:, 0:2]), _relm(np.asarray(got[4])[:, 3:5], mh[:, 3:5]),
                             float(np.max(np.abs(np.asarray(got[4], dtype=LD)[:, 2] - mh[:, 2]))))
        if last_step:
            continue
        mu3, P33 = run.poses[k]
        w["pose"] = max(w["pose"], float(np.max(np.abs(np.asarray(mu3, dtype=LD) - rec.pose))))
        w["pose_block"] = max(w["pose_block"], _relm(P33, rec.block))
    if not ref.exact:
        want = (np.asarray(ref.mean, dtype=np.float64), np.asarray(ref.cov, dtype=np.float64))
        got = (np.asarray(run.mean, dtype=np.float64), np.asarray(run.cov, dtype=np.float64))
        if got[0].shape != want[0].shape or got[1].shape != want[1].shape:
            return w, bad + [f"a final state of {got[0].shape} / {got[1].shape}"]
        err = state_errors(got, want, ref.init_var)
        entry = ("corr_max", "mean_landmarks")
        w["state"] = max(err[p] for p in PIECES if p in err and p not in entry)
        w["state_entry"] = max(err[p] for p in entry if p in err)
        if "loose_block" in err:
            eps_v = 32 * np.finfo(float).eps * ref.init_var
            if err["loose_block"] > eps_v or err["loose_mean"] > 1e-9 or err["loose_zeros"] != 0:
                bad.append(f"loose landmarks: block {err['loose_block']:.3e} (bound {eps_v:.3e}), mean {err['loose_mean']:.3e}, "
                           f"{err['loose_zeros']} non-zero entries where the model holds exact zeros")
            w["state_entry"] = max(w["state_entry"], err["loose_cross"])
    return w, bad


def judge(run, ref, bars, what="", range_relative=False, symmetric=False):
    """`run` against the model within `bars` ({figure: bound}); returns the distances.  `symmetric`: the covariance and every
    pose block must be exactly symmetric (the device's are)."""
    w, bad = distances(run, ref, range_relative)
    bad = list(bad)
    for k in FIGURES:
        if not w[k] <= bars[k]:
            bad.append(f"{k}: {w[k]:.3e} exceeds {bars[k]:g}")
    if symmetric:
        if not np.array_equal(run.cov, np.asarray(run.cov).T):
            bad.append("the final covariance is not exactly symmetric")
        if not all(np.array_equal(P, np.asarray(P).T) for _, P in run.poses):
            bad.append("a pose block of the trace is not exactly symmetric")
    assert not bad, what + "; ".join(bad)
    return w
