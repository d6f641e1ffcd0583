"""The CPU model of the hypothesis bank's weights, systematic resampling, copy and split (ekf_hypotheses_weigh /
ekf_hypotheses_resample), in float64 NumPy as include/ekfslam_hip.h states them, and the cases the CPU and GPU tests share.  A plain
module: nothing here needs a device.

A bank is a `Bank` of arrays: pose (K, 3), blk (K, 3, 3), rows (K, 3, n) -- P[0:3, :] with the block mirrored in its first three
columns, what `HypothesisBank.rows` returns --, loglik (K,), n_obs, n_rej (K,), flags (K,).

The plan's one delicate point is t_k = ceil(K C_k - u): a device that sums the weights in another order moves K C_k by at most
K^2 2^-53 (1.9e-9 at K = 4096), so wherever every K C_k - u keeps `MARGIN` = 1e-7 from the nearest integer, ancestors and
offspring must be EQUAL to the model's.  `margin` measures that distance; tests/test_hyp_resample_cpu.py asserts it for every
case of `PLAN_CASES` and for the kidnapped-robot run, so the GPU tests can only fail for the device's own reasons."""
import dataclasses
import typing

import numpy as np

NONFINITE = 1                                              # EKF_FLAG_NONFINITE
MARGIN = 1e-7
U_LAST = 1.0 - 2.0 ** -53                                  # the largest double below 1


@dataclasses.dataclass
class Bank:
    pose: np.ndarray
    blk: np.ndarray
    rows: np.ndarray
    loglik: np.ndarray
    n_obs: np.ndarray
    n_rej: np.ndarray
    flags: np.ndarray

    def copy(self):
        return Bank(*(np.array(getattr(self, f.name)) for f in dataclasses.fields(self)))

    @property
    def count(self):
        return len(self.loglik)


class Weights(typing.NamedTuple):
    w: np.ndarray                                          # exp(loglik - max) where the hypothesis weighs, else 0: not normalised
    ess: float
    logmean: float
    live: int
    last: int                                              # the last hypothesis with w > 0 (-1: none)


def weigh(loglik, flags=None):
    """w (not normalised: exp(loglik - max) over the hypotheses that weigh), ess, logmean, live, last live index (-1: none)."""
    ll = np.asarray(loglik, dtype=np.float64)
    K = len(ll)
    ok = np.isfinite(ll)
    if flags is not None:
        ok &= (np.asarray(flags) & NONFINITE) == 0
    w = np.zeros(K)
    if ok.any():
        top = ll[ok].max()
        w[ok] = np.exp(ll[ok] - top)
    pos = np.nonzero(w > 0.0)[0]
    if len(pos) == 0:
        return Weights(w, 0.0, -np.inf, 0, -1)
    s, s2 = w.sum(), (w * w).sum()
    return Weights(w, float(s * s / s2), float(top + np.log(s / K)), int(len(pos)), int(pos[-1]))


def _t_raw(w, u):
    """K C_k - u before ceil and clamp, C the inclusive cumulative sum of the normalised weights."""
    K = len(w)
    return K * (np.cumsum(w) / w.sum()) - u


def margin(loglik, flags, u):
    """The least distance of K C_k - u from an integer over the hypotheses that weigh, the last of them left out (its t is K by
    definition, not by rounding).  inf where there is nothing to round: a degenerate bank, or one live hypothesis."""
    W = weigh(loglik, flags)
    if W.live == 0:
        return np.inf
    x = _t_raw(W.w, u)[(W.w > 0.0) & (np.arange(len(W.w)) < W.last)]
    return float(np.abs(x - np.round(x)).min()) if len(x) else np.inf


def plan(loglik, flags, u):
    """(ancestors, offspring, Weights).  A degenerate bank: the identity."""
    W = weigh(loglik, flags)
    K = len(W.w)
    if W.live == 0:
        return np.arange(K, dtype=np.int32), np.ones(K, dtype=np.int32), W
    t = np.clip(np.ceil(_t_raw(W.w, u)), 0, K).astype(np.int64)
    t[W.last:] = K
    t = np.where(W.w > 0.0, t, 0)                          # a hypothesis that weighs nothing carries t on ...
    t = np.maximum.accumulate(t)                           # ... and t never falls
    off = np.diff(np.concatenate([[0], t])).astype(np.int32)
    anc = np.arange(K, dtype=np.int32)
    dead = np.nonzero(off == 0)[0]
    extras = np.repeat(np.arange(K), np.maximum(off - 1, 0))
    assert len(extras) == len(dead)
    anc[dead] = extras
    return anc, off, W


def chol3(P):
    """The lower factor with the device's rule: a pivot <= 0 or not finite zeroes its column."""
    L = np.zeros((3, 3))

    def ok(d):
        return d > 0.0 and np.isfinite(d)
    if ok(P[0, 0]):
        L[0, 0] = np.sqrt(P[0, 0])
        L[1, 0], L[2, 0] = P[0, 1] / L[0, 0], P[0, 2] / L[0, 0]
    d1 = P[1, 1] - L[1, 0] * L[1, 0]
    if ok(d1):
        L[1, 1] = np.sqrt(d1)
        L[2, 1] = (P[1, 2] - L[2, 0] * L[1, 0]) / L[1, 1]
    d2 = P[2, 2] - L[2, 0] * L[2, 0] - L[2, 1] * L[2, 1]
    if ok(d2):
        L[2, 2] = np.sqrt(d2)
    return L


def resample(bank, u, split=0.0, z=None, mutant=None):
    """The resampled bank (a new one) and (ancestors, offspring, Weights).  `mutant`: one of the three wrong implementations
    the CPU test shows the GPU test's judge to catch -- "loglik" (copies the ancestor's log-likelihood instead of setting the
    evidence), "block" (scales the block but not the rows), "single" (splits the slots of single-offspring ancestors too)."""
    anc, off, W = plan(bank.loglik, bank.flags, u)
    out = bank.copy()
    if W.live == 0:
        return out, (anc, off, W)
    for name in ("pose", "blk", "rows", "n_obs", "n_rej", "flags"):
        getattr(out, name)[:] = getattr(bank, name)[anc]
    out.loglik[:] = bank.loglik[anc] if mutant == "loglik" else W.logmean
    if split > 0.0:
        keep = 1.0 - split * split
        for k in range(bank.count):
            if off[anc[k]] < 2 and mutant != "single":
                continue
            out.pose[k] = out.pose[k] + split * (chol3(out.blk[k]) @ np.asarray(z, dtype=np.float64)[k])
            out.blk[k] = keep * out.blk[k]
            if mutant != "block":
                out.rows[k] = keep * out.rows[k]
            else:
                out.rows[k][:, :3] = out.blk[k]
    return out, (anc, off, W)


def bits_equal(a, b):
    """np.array_equal on the bits: NaN equals the same NaN (a flagged hypothesis holds them), -0.0 differs from 0.0."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return a.tobytes() == b.tobytes()


def judge(got, before, u, split, z, logmean=None, pose_tol=1e-9):
    """What the GPU test asks of a resampled bank `got` given the bank `before` it: None, or what is wrong.  Copies, counters,
    blocks and rows bit for bit (a split: keep * the value before, one multiply), every log-likelihood the evidence, poses of split
    slots within `pose_tol`, every other slot's pose bit for bit.  `logmean`: the evidence the device reported (default: the model's)."""
    want, (anc, off, W) = resample(before, u, split, z)
    if W.live and logmean is not None:                     # (the device's own evidence, itself within 1e-9 of the model's)
        if not abs(logmean - W.logmean) <= 1e-9 * max(1.0, abs(W.logmean)):
            return "the evidence is off"
        want.loglik[:] = logmean
    if not bits_equal(got.loglik, want.loglik):
        return "loglik is not the evidence everywhere"
    for name in ("n_obs", "n_rej", "flags", "blk", "rows"):
        if not bits_equal(getattr(got, name), getattr(want, name)):
            return f"{name} differs"
    moved = off[anc] >= 2 if split > 0.0 else np.zeros(before.count, dtype=bool)
    if not bits_equal(got.pose[~moved], want.pose[~moved]):
        return "the pose of a slot that was not split moved"
    if moved.any() and not np.abs(got.pose[moved] - want.pose[moved]).max() <= pose_tol:
        return "the pose of a split slot is off"
    return None


# ---- the plan cases the CPU test (margin) and the GPU test (device against model) share ---------------------------------------
# Log-likelihoods come from the device in the GPU test: K hypotheses seeded on the map's own pose, then ONE update with landmark
# PLAN_LM seen at its predicted range + d_k and its predicted bearing, so that loglik_k = -1/2 (d_k^2 (S^-1)_rr + ln det S +
# 2 ln 2 pi): d shapes the weights.  An offset of DEAD metres underflows exp: the hypothesis weighs exactly nothing.  A flagged
# hypothesis is given a NaN range, which sets its sticky flag.  A case: (name, K, d (K,), u, flagged indices, the indices whose offset is DEAD).
PLAN_LM, DEAD, PLAN_KS = 0, 40.0, (1, 2, 65, 1025)


def plan_cases(K):
    d = np.random.default_rng(100 + K).normal(0.0, 1.9, K)             # 2.5 sigma of the range innovation: ESS about K / 2
    cases = [("typical", K, d, 0.37, (), ()), ("u = 0", K, d, 0.0, (), ()), ("u = 1 - 2^-53", K, d, U_LAST, (), ()),
             ("uniform, the identity", K, np.zeros(K), 0.5, (), ())]
    onehot = np.full(K, DEAD)
    onehot[K // 3] = 0.0
    cases.append(("one-hot", K, onehot, 0.61, (), tuple(k for k in range(K) if k != K // 3)))
    if K >= 2:
        for dead in ((0, K - 1),) if K >= 3 else ((0,), (K - 1,)):           # (a bank of two keeps one alive)
            ends = d.copy()
            ends[list(dead)] = DEAD
            cases.append((f"nothing weighs at {dead}", K, ends, 0.23, (), dead))
        cases.append(("a flagged hypothesis", K, d, 0.81, (K // 2,), ()))
    cases.append(("degenerate: all flagged", K, d, 0.4, tuple(range(K)), ()))
    return cases


def plan_map(N=20, seed=11, steps=30):
    """The dense model of tests/hyp_support.mapped_handle(sd, 1): (mean, cov) after the mapping run."""
    from oracle import ekf_oracle as orc
    from tests import streams
    _, lin, ang, idx, zr, zb, m = streams.wandering(N, 1, steps, 8, seed)
    world = orc.synthetic_world(N, seed + 1)
    mean, cov, cfg = world[2].copy(), np.diag(world[3]), orc.EkfConfig()
    for k in range(steps):
        mk = int(m[k, 0])
        mean, cov = orc.ekf_step_dense(mean, cov, lin[k, 0], ang[k, 0], idx[k, 0, :mk], zr[k, 0, :mk], zb[k, 0, :mk], cfg)
    return mean, 0.5 * (cov + cov.T)


def plan_case_logliks(mean, cov, d):
    """The log-likelihoods the device's update leaves for the offsets d, from the dense model: one literal_step gives S, the
    innovation is (d_k, 0)."""
    from oracle import ekf_oracle as orc
    from tests import localize_model as lm
    t = 3 + 2 * PLAN_LM
    dx = mean[t:t + 2] - mean[:2]
    r0, b0 = float(np.hypot(*dx)), float(np.arctan2(dx[1], dx[0]) - mean[2])
    log = []
    lm.literal_step(mean, cov, 0.0, 0.0, [PLAN_LM], [r0], [b0], orc.EkfConfig(), predict=False, log=log)
    S = log[0][2]
    Si = np.linalg.inv(S)
    return -0.5 * (np.asarray(d) ** 2 * Si[0, 0] + np.log(np.linalg.det(S)) + 2.0 * np.log(2.0 * np.pi))


# ---- the kidnapped robot with resampling: tests/hypotheses_model.py's scenario, resample_if(0.5, split = SPLIT) behind every step --
SPLIT, FRACTION = 0.5, 0.5


def kidnapped_draws(K, steps, seed=5):
    """The fixed offsets u (steps,) and draws z (steps, K, 3) of the run."""
    rng = np.random.default_rng(seed)
    return rng.random(steps), rng.standard_normal((steps, K, 3))


def split_dense(mean, cov, s, z):
    """The split on a dense state: pose += s L z, the pose block and the pose rows and columns keep 1 - s^2."""
    mean, cov = np.array(mean), np.array(cov)
    keep = 1.0 - s * s
    mean[:3] = mean[:3] + s * (chol3(cov[:3, :3]) @ z)
    blk = keep * cov[:3, :3]
    cov[:3, :] = keep * cov[:3, :]
    cov[:, :3] = keep * cov[:, :3]
    cov[:3, :3] = blk
    return mean, cov


def run_fleet_resampling(map_mean, map_cov, case, us, zs):
    """hypotheses_model.run_fleet with the policy: (poses, blocks, loglik, events), events = [(step, ancestors, offspring,
    margin)] for every resampling that took place."""
    from tests import hypotheses_model as hm
    from tests import localize_model as lm
    cfg = hm.model_cfg()
    K = len(case.seeds)
    states = [hm.reset_state(map_mean, map_cov, case.seeds[k], hm.SEED_COV) for k in range(K)]
    ll, events = np.zeros(K), []
    for i, (lin, ang, idx, zr, zb) in enumerate(case.steps):
        for k in range(K):
            log = []
            states[k] = lm.literal_step(*states[k], lin, ang, idx, zr, zb, cfg, log=log)
            ll[k] += hm.loglik_of(log)
        flags = np.zeros(K, dtype=np.uint32)
        if weigh(ll, flags).ess < FRACTION * K:
            anc, off, W = plan(ll, flags, us[i])
            events.append((i, anc, off, margin(ll, flags, us[i])))
            states = [states[a] for a in anc]
            states = [split_dense(*states[k], SPLIT, zs[i][k]) if off[anc[k]] >= 2 else states[k] for k in range(K)]
            ll[:] = W.logmean
    return np.array([s[0][:3] for s in states]), np.array([s[1][:3, :3] for s in states]), ll, events
