"""Shared by the tests of a hypothesis bank's unlabelled observations (tests/test_hyp_assoc_cpu.py,
tests/test_gpu_hyp_associate.py): the table of worlds, a hypothesis's dense state, the reference and the judge.  The reference is
tests/assoc_world.py's -- ref_scores / ref_candidates on the dense state of one hypothesis -- and the judge is its check_query,
tolerances and excuses unchanged: NIS within 1e-9 cond(S) relative, ln det S within 2e-9 cond(S) absolute, the candidate order
compared where the reference's own order is clear of those tolerances.  The resolve is frontend.resolve_associations with
create = inf: the map is frozen, "new" means dropped.  A plain module."""
import functools
from types import SimpleNamespace as NS

import numpy as np

from oracle import ekf_oracle as orc
from slam_duckietown_amd import frontend
from tests import assoc_world as aw
from tests import hyp_support as hs
from tests import streams

CASES = ((20, 3, 5), (20, 65, 16), (70, 65, 8), (130, 33, 8))      # (N, K, m)
RESET_BLOCK = np.diag([0.05 ** 2, 0.05 ** 2, 0.1 ** 2])
MAP_SEED, OBS_SEED, OBS_NOISE = 11, 5, 0.01


def slam_inputs(N):
    """(mean0, diag0, lin, ang, idx, zr, zb, m) of the mapping run: hs.mapped_handle's, for one trajectory."""
    _, lin, ang, idx, zr, zb, m = streams.wandering(N, 1, hs.SLAM_STEPS, 8, MAP_SEED)
    world = orc.synthetic_world(N, MAP_SEED + 1)
    return world[2], world[3], lin, ang, idx, zr, zb, m


def first_sighting(N):
    """(landmark, range, bearing) of the first observation of the mapping run."""
    _, _, _, _, idx, zr, zb, m = slam_inputs(N)
    k = int(np.flatnonzero(m[:, 0] > 0)[0])
    return int(idx[k, 0, 0]), float(zr[k, 0, 0]), float(zb[k, 0, 0])


def seeds(mean, N, K):
    """K poses on the circle of the first sighting around that landmark as the map places it; hypothesis 0 at the slot's own pose."""
    lm, r, b = first_sighting(N)
    poses = frontend.poses_on_circle(mean[3 + 2 * lm:5 + 2 * lm], r, b, K)
    poses[0] = mean[:3]
    return poses


def observations(mean, N, m):
    """m landmarks of rng(5).choice(N, m) as the slot's mean sees them, with 0.01 noise: (labels, ranges, bearings)."""
    rng = np.random.default_rng(OBS_SEED)
    return hs.observe(mean, rng.choice(N, m), rng, OBS_NOISE)


def dense_state(mean, cov, pose, rows):
    """Hypothesis k's dense (mu_k, P_k): the slot's state with the pose, the pose block and the pose rows replaced."""
    mu, P = np.array(mean, dtype=float), np.array(cov, dtype=float)
    mu[:3] = pose
    P[:3, :] = rows
    P[:, :3] = rows.T
    return mu, P


def bank_states(f, bank):
    """Every hypothesis's dense state from the slot's downloaded state, bank.poses() and bank.rows(k)."""
    mean, cov = f.state(0)
    poses, _ = bank.poses()
    return [dense_state(mean, cov, poses[k], bank.rows(k)) for k in range(bank.count)]


@functools.lru_cache(maxsize=None)
def model_map(N):
    """The map as the oracle's dense filter leaves it after the mapping run."""
    mean, diag0, lin, ang, idx, zr, zb, m = slam_inputs(N)
    cfg = orc.EkfConfig()
    mu, P = mean.copy(), np.diag(diag0)
    for k in range(hs.SLAM_STEPS):
        mk = int(m[k, 0])
        mu, P = orc.ekf_step_dense(mu, P, lin[k, 0], ang[k, 0], idx[k, 0, :mk], zr[k, 0, :mk], zb[k, 0, :mk], cfg)
    return mu, P


def model_states(N, K):
    """The table's hypotheses on the model map: reset to the seeds with RESET_BLOCK, every cross term dropped."""
    mu, P = model_map(N)
    rows = np.zeros((3, len(mu)))
    rows[:, :3] = RESET_BLOCK
    return [dense_state(mu, P, p, rows) for p in seeds(mu, N, K)]


def model_query(states, zr, zb, qd, cross=True, by_nis=False):
    """The reference's answer in the query's shape (a HypothesisAssociations look-alike), one row per dense state.  The planted
    mistakes: cross=False forms the scores without the pose-landmark cross terms, by_nis=True ranks by NIS alone."""
    K, m = len(states), len(zr)
    N = (len(states[0][0]) - 3) // 2
    out = NS(cand=np.full((K, m, 2), -1, dtype=np.int32), nis=np.full((K, m, 2), np.nan), logdet=np.full((K, m, 2), np.nan),
             min_nis=np.full((K, m), np.nan), all_nis=np.full((K, m, N), np.nan), all_logdet=np.full((K, m, N), np.nan))
    for k, (mu, P) in enumerate(states):
        if not cross:
            P = P.copy()
            P[:3, 3:] = 0.0
            P[3:, :3] = 0.0
        nis, logdet, _, _ = aw.ref_scores(mu, P, zr, zb, qd)
        cand, cnis, mn, _ = aw.ref_candidates(nis, np.zeros_like(logdet) if by_nis else logdet)
        out.all_nis[k], out.all_logdet[k] = nis, np.broadcast_to(logdet, (m, N))
        out.cand[k], out.nis[k], out.min_nis[k] = cand, cnis, mn
        for q in range(m):
            for c in range(2):
                if cand[q, c] >= 0:
                    out.logdet[k, q, c] = logdet[cand[q, c]]
    return out


class _Shape:
    """What aw.check_query asks of a filter beside the query's result: the observations as (K, m) arrays."""

    def __init__(self, K):
        self.K = K

    def _unlabelled(self, zr, zb, m):
        zr, zb = np.asarray(zr, dtype=float), np.asarray(zb, dtype=float)
        return (np.broadcast_to(zr, (self.K, len(zr))), np.broadcast_to(zb, (self.K, len(zb))),
                np.full(self.K, len(zr), dtype=np.int32))


def new_totals():
    return {"entries": 0, "left_out": 0, "obs": 0, "excused": 0}


def judge(res, states, zr, zb, meas_sigma, totals, what=""):
    """aw.check_query on a query of len(states) hypotheses -- raises AssertionError where it fails -- counting what it leaves out
    (entries within 1e-9 of the wrap) and excuses (observations whose candidate order is not clear) into `totals`."""
    aw.check_query(_Shape(len(states)), lambda k: states[k], zr, zb, meas_sigma=meas_sigma, what=what, res=res, totals=totals)


def resolve(cand, nis, min_nis, accept):
    """frontend.resolve_associations on a frozen map: (assign (m,), dropped count); new -> dropped."""
    assign, new_obs, dropped = frontend.resolve_associations(cand, nis, min_nis, accept, np.inf)
    assert not new_obs or (np.asarray(cand).reshape(-1, 2)[new_obs, 0] < 0).all()      # (create = inf: only an empty map makes "new")
    return assign, len(new_obs) + len(dropped)


def host_lists(res, zr, zb, accept):
    """The per-hypothesis lists the guarantee's host route hands to bank.update, and the assignment (K, m) they come from."""
    K, m = res.cand.shape[:2]
    assign = np.full((K, m), -1, dtype=np.int64)
    idx, rr, bb = [], [], []
    for k in range(K):
        assign[k], _ = resolve(res.cand[k], res.nis[k], res.min_nis[k], accept)
        keep = np.flatnonzero(assign[k] >= 0)
        idx.append(assign[k, keep].astype(np.int32))
        rr.append(np.asarray(zr, dtype=float)[keep])
        bb.append(np.asarray(zb, dtype=float)[keep])
    return idx, rr, bb, assign


def resolve_twice(cand, nis, min_nis, accept):
    """The planted mistake: a resolve that lets two observations take one landmark (every observation its best candidate)."""
    cand, nis = np.asarray(cand).reshape(-1, 2), np.asarray(nis).reshape(-1, 2)
    return np.where((cand[:, 0] >= 0) & (nis[:, 0] <= accept), cand[:, 0], -1)


def judge_assignment(got, res, accept):
    """None, or what is wrong with the assignment rows `got` (K, m) against the resolve of the query `res`."""
    for k in range(res.cand.shape[0]):
        want, _ = resolve(res.cand[k], res.nis[k], res.min_nis[k], accept)
        if not np.array_equal(np.asarray(got[k]), want):
            return f"hypothesis {k}: assignment {list(np.asarray(got[k]))} where the resolve gives {list(want)}"
        taken = [int(j) for j in got[k] if j >= 0]
        if len(set(taken)) != len(taken):
            return f"hypothesis {k}: a landmark taken twice"
    return None
