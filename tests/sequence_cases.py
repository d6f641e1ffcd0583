"""The table of tests/test_gpu_sequence_pairs.py and tests/test_sequence_cpu.py: every ORDERED PAIR of state-changing calls.

Each call of the handle is tested against its own dense model; what the calls share is the per-trajectory bookkeeping of
csrc/ekf_api.hip (size, the active bound and its mirrors, pending ranks and pose noise, the tag row, the stream, the tables of
copy / join / transform), and a mirror left stale by one call shows only in the NEXT call that trusts it.  So: a start with ranks
pending, operation A, operation B, then a continuation (a step and a stream) whose covariance pass reads whatever A and B left
-- judged after each of the three against ONE dense model of the whole sequence (tests/sequence_model.py), block by block
(parity_blocks.assert_state_close).  21 operations, 441 pairs, each with a name (225 until localisation joined the table, 324
until localisation from detections and the hypothesis bank did).

START: direct_model.small_stream at N = 30 -- synthetic_stream(26, 31, 4, seed) over landmarks 0 .. 25, landmarks 26 .. 29 never
observed at landmark_init_var: n = 63, one column short of the 64-column tile edge of the general kernels, so that growth
(add_landmarks, join, a window) crosses it.  n_max = 79 (38 landmarks; the largest pair, join + join, reaches 36): the
small-state path by default, the general kernels under `both_paths`.  Prelude: run_stream of 28 steps, then THREE single steps
-- all 31 of the stream.  (Two were planned, so that ranks are pending on the general kernels when A starts; but 28 stream steps
of m = 4 are cadences of 10, 10 and 8 steps, the last one's 64 ranks stay pending, and the second single step fills the 80 of
"rank_limit": the pass runs behind it and NOTHING is pending.  The third step's 8 ranks are.)

An operation is a function (driver, rng): it draws its arguments from the MODEL's current state -- so it stays valid after a
renumbering -- and issues the calls through the driver, which hands each to the model and to whatever runs beside it (a filter,
the model in another precision).  Every argument is therefore the same float64 value for all of them.

The same setup, prelude and operations serve tests/test_gpu_queries_after_calls.py and tests/test_queries_after_calls_cpu.py
(run_query_case, below): ONE operation, then the read-only queries -- no second operation, and no download in between."""
import functools

import numpy as np

from oracle import ekf_oracle as orc
from slam_duckietown_amd import frontend
from tests import direct_model as dm
from tests import fuzz_model as fz
from tests import linear_model as lm
from tests import localize_model as lcm
from tests import motion_model as mm
from tests import parity_blocks as pb
from tests import sequence_model as sm
from tests.streams import FRAME, stream_from

INIT_VAR = orc.EkfConfig().landmark_init_var
N_OBSERVED, N_LANDMARKS, N_MAX = 26, 30, 79
STREAM_STEPS, SINGLE_STEPS = 28, 3
SEED = 7
TOL = 1e-9              # every piece of the informed part against the model (parity_blocks' default against the oracle)
FLOOR_TOL = 1e-11       # admissibility: the model in float64 against itself in longdouble, every relative-Frobenius piece
# ENTRY_TOL: the bound of the loose landmarks' cross terms = 10 x the worst entrywise piece (corr_max, mean_landmarks,
# loose_cross) of the float64 model against the longdouble one over all 225 cases -- the margin update_cases.DENSE_NEVER
# takes over its own measurement.  tests/test_sequence_cpu.py repeats the measurement and holds this constant to it;
# profiles/sequence_pairs.txt has the figures.
ENTRY_FLOOR = 4.0e-11     # measured 3.78e-11: corr_max of "remove_landmarks then update_direct" after the continuation
#                           (the 99 pairs added with localisation reach 3.34e-11: the maximum, and the constant, stay)
ENTRY_TOL = 10 * ENTRY_FLOOR

TAG0 = 100              # landmark j of the start carries tag TAG0 + j
T_PLAIN = np.array([0.7, -0.4, -2.9])           # transform without a covariance
T_COV = np.array([-0.3, 0.5, 0.4])              # ... and with COV
COV = FRAME[1]


@functools.lru_cache(maxsize=None)
def start(seed=SEED):
    """(mean0, diag0, lin, ang, idx, zr, zb): dm.small_stream generalised to N = 30."""
    s = orc.synthetic_stream(N_OBSERVED, STREAM_STEPS + SINGLE_STEPS, 4, seed)
    rng = np.random.default_rng(300 + seed)
    extra = 2 * (N_LANDMARKS - N_OBSERVED)
    mean0 = np.concatenate([s[0], rng.uniform(-1.0, 1.0, extra)])
    diag0 = np.concatenate([s[1], np.full(extra, INIT_VAR)])
    return (mean0, diag0) + tuple(s[2:])


@functools.lru_cache(maxsize=None)
def sources():
    """The other handles a case reads, key -> (mean, covariance, tag index): "map3" a 3-landmark filter (join), "map12" a
    12-landmark one (copy_from); the dense oracle's states, which a handle takes verbatim through set_state."""
    out = {}
    for key, (N, steps, m, seed, tag0) in {"map3": (3, 10, 3, 61, 300), "map12": (12, 12, 4, 62, 400)}.items():
        _, om, oP = dm.run_dense(N, steps, m, seed)
        out[key] = (om, oP, {tag0 + j: j for j in range(N)})
    return out


class Driver:
    """Hands every call to the model and to the sinks beside it; operations read `model` for their arguments."""

    def __init__(self, model, *sinks):
        self.model, self.sinks = model, (model,) + sinks
        self.calls = []

    def __getattr__(self, name):
        def call(*args, **kw):
            self.calls.append(name)
            for s in self.sinks:
                getattr(s, name)(*args, **kw)
        return call


# ---- what the operations pick -------------------------------------------------------------------------------------------------
def pick(tr):
    """(an informed landmark, a loose one -- the last but one landmark where none is left --, the last landmark), distinct."""
    loose, informed = pb.loose_landmarks(tr.cov, INIT_VAR)
    last = tr.n_lm - 1
    a = int(next(l for l in informed if l != last)) if len(informed) else 0
    b = int(next((l for l in loose if l not in (a, last)), next(l for l in range(tr.n_lm - 2, -1, -1) if l != a)))
    return a, b, last


def observe(drv, rng, idx):
    """One step that observes `idx`, consistently with the model's mean (lm.follow_up_obs)."""
    zr, zb = lm.follow_up_obs(drv.model.tr.mean, idx, int(rng.integers(0, 50)))
    drv.step1(0.004, 0.02, [int(i) for i in idx], zr, zb)


def stream(drv, rng, steps, m):
    st = stream_from(drv.model.tr.mean, steps, m, int(rng.integers(1 << 30)))
    drv.run_stream(*st)


# ---- the 21 operations --------------------------------------------------------------------------------------------------------
def op_step(drv, rng):
    tr = drv.model.tr
    _, never, last = pick(tr)
    observe(drv, rng, list(dict.fromkeys([0, never, last])))


def op_run_stream(drv, rng):
    stream(drv, rng, 6, 4)


def op_step_detections(drv, rng):
    """One known tag (the tagged landmark nearest to the pose) and one new one, two frames."""
    tr = drv.model.tr
    d = {t: float(np.hypot(*(tr.mean[3 + 2 * j:5 + 2 * j] - tr.mean[:2]))) for t, j in tr.tags.items()}
    known = min(d, key=d.get)
    assert d[known] < 1.3
    new = next(i for i in range(600, 1024) if i not in tr.tags)
    win = fz.window_of(rng, tr, [known, new], {new: (0.2, 0.8)}, 2)
    drv.step_detections(0.004, 0.02, win)


def op_predict_linear(drv, rng):
    tr = drv.model.tr
    drv.predict_linear(*mm.draw(rng, tr.mean, tr.cov, "full"))


# predict_dense: F = I + DENSE_F * randn / sqrt(n), dense.  A loose landmark then carries 1e4 * F_ij ~ 0.04 against every other
# entry (correlation 2e-3 with an informed landmark: a skipped row shows at once), and DENSE_F is as large as admissibility
# allows: when a loose landmark correlated with another is observed, its 1e4 cancels inside the other's own block, and at
# DENSE_F = 2e-3 the float64 model itself is 5e-10 off there -- above the 32 eps init_var the judge allows that block -- and at
# 1e-4 a direct fix of such a landmark leaves the informed means 1.8e-10 sigma off, too near TOL.
DENSE_F = 3e-5


def op_predict_dense(drv, rng):
    n = len(drv.model.tr.mean)
    F = np.eye(n) + rng.normal(size=(n, n)) * (DENSE_F / np.sqrt(n))
    A = rng.normal(size=(n, 3)) * 0.02
    drv.predict_dense1(F, A @ A.T + np.diag(rng.uniform(1e-4, 1e-3, n)))


def op_update_direct(drv, rng):
    """A pose fix, an informed landmark and a loose one (surveyed within decimetres of its prior mean: dm.case_small).

    The loose landmark's survey has sigma 0.3 .. 0.6 m.  A fix forms v - v^2 / (v + R) with v = 1e4: whatever the code, the
    result carries up to 32 eps init_var = 7.1e-11 absolutely (assert_update_close's rule for a first-touched block).  Here the
    fixed landmark is INFORMED afterwards and judged relatively, at TOL = 1e-9 of its variance ~ R: that can hold only for
    R > 7.1e-11 / 1e-9 = 0.07 m^2.  (dm.make_fixes' sigma of 0.02 .. 0.1 m asks for 1e-9 of 4e-4 .. 1e-2.)"""
    tr = drv.model.tr
    a, never, _ = pick(tr)
    z, R = dm.make_fixes(rng, tr.mean, tr.cov, [dm.POSE, a])
    sig, rho = rng.uniform(0.3, 0.6, 2), rng.uniform(-0.4, 0.4)
    Rn, zn = np.zeros((3, 3)), np.zeros(3)
    Rn[:2, :2] = np.array([[sig[0] ** 2, rho * sig[0] * sig[1]], [rho * sig[0] * sig[1], sig[1] ** 2]])
    zn[:2] = tr.mean[3 + 2 * never:5 + 2 * never] + np.sqrt(0.01 + sig ** 2) * rng.normal(size=2)
    drv.update_direct([dm.POSE, a, never], z + [zn], R + [Rn])


def op_update_linear(drv, rng):
    """A relative constraint between an informed and a loose landmark (a dense H: the bound rises): lm.case_panel's."""
    tr = drv.model.tr
    a, never, _ = pick(tr)
    offset = tr.mean[3 + 2 * never:5 + 2 * never] - tr.mean[3 + 2 * a:5 + 2 * a] + np.array([0.1, -0.2])
    drv.update_linear(*lm.constraint_rows(a, never, offset, np.eye(2) * 0.05 ** 2))


def op_transform(drv, rng):
    drv.transform(T_PLAIN, None)


def op_transform_cov(drv, rng):
    drv.transform(T_COV, COV)


def op_join(drv, rng):
    drv.join("map3", None, None)


def op_join_explicit(drv, rng):
    drv.join("map3", FRAME[0], FRAME[1])


def op_remove(drv, rng):
    a, never, _ = pick(drv.model.tr)
    drv.remove_landmarks([never, a])


def op_add(drv, rng):
    drv.add_landmarks(rng.uniform(-1.0, 1.0, (2, 2)))


def op_copy(drv, rng):
    drv.copy_in("map12")


def op_bound_off(drv, rng):
    drv.set_option("active_bound", 0)
    op_step(drv, rng)
    drv.set_option("active_bound", 1)


# ---- localisation on a frozen map ---------------------------------------------------------------------------------------------
# k_loc_rows updates the pose rows only below the active bound, and no later pass repairs a column it skipped (localisation
# appends no rank).  Each operation is therefore TWO parts.  Part one names only informed landmarks far below the start's bound
# (`a`, and the tail's `mid`): its own bound is low, and it is right only if the bound A left reaches every column A correlated.
# Part two names a loose landmark: now the operation itself must raise every mirror, for B and the continuation.  (One call that
# names the last landmark sets its own bound to n and says nothing about A.)
def localize_obs(drv, rng, idx):
    return lm.follow_up_obs(drv.model.tr.mean, idx, int(rng.integers(0, 50)))


def op_localize(drv, rng):
    tr = drv.model.tr
    a, never, _ = pick(tr)
    idx = [a, tail_mid(tr), a]                             # (an index twice: legal for localisation only)
    drv.localize1(0.004, 0.02, idx, *localize_obs(drv, rng, idx))
    idx = [0, never]
    drv.localize1(0.004, 0.005, idx, *localize_obs(drv, rng, idx))


def op_localize_update(drv, rng):
    tr = drv.model.tr
    a, never, _ = pick(tr)
    idx = [a, tail_mid(tr)]
    drv.localize_update1(idx, *localize_obs(drv, rng, idx))
    idx = [never, a]
    drv.localize_update1(idx, *localize_obs(drv, rng, idx))


def op_run_localize(drv, rng):
    """Four stream steps of three landmarks each (landmarks 0 .. 11: informed, below the bound A left); the last observation of
    the last step names a loose landmark instead, seen from where the increments take the model's pose, a few centimetres and
    hundredths of a radian off.  Steps 0 .. 2 rely on the bound A left; the last raises it through the stream's own bound."""
    tr = drv.model.tr
    _, never, _ = pick(tr)
    lin, ang, idx, zr, zb = stream_from(tr.mean, 4, 3, int(rng.integers(1 << 30)))
    at = tr.mean.copy()
    for k in range(len(lin)):
        at[:3] = orc.motion_model(at[:3], lin[k], ang[k], orc.EkfConfig())[0]
    r, b = lm.follow_up_obs(at, [never], int(rng.integers(0, 50)))
    if never not in idx[-1]:                               # (behind copy_from the last step names it already, and an uploaded
        idx[-1, -1], zr[-1, -1], zb[-1, -1] = never, r[0], b[0]    # stream -- a SLAM stream too -- takes no index twice in a step)
    drv.run_localize_stream(lin, ang, idx, zr, zb)


# ---- localisation from raw detections ------------------------------------------------------------------------------------------
# ekf_localize_detections raises its bound ON THE DEVICE, from whatever the window matched, and the host follows through the
# `sizes_dirty` read-back.  Two windows, as the localisation operations above have two parts: window one shows the tags of `a` and
# the tail's `mid` and one tag the table does not hold (it must come back unmatched and add nothing); window two the tags of
# landmark 0 and of a loose landmark.  The operation asserts ON THE MODEL that each window matches exactly what it intends.
GATE = 1.39             # fz.window_of leaves a known tag out beyond 1.4 m from the pose; the device's gate is 1.5 m


def pose_distance(tr, j):
    return float(np.hypot(*(tr.mean[3 + 2 * j:5 + 2 * j] - tr.mean[:2])))


def tags_in_gate(tr):
    """The landmarks whose tag a camera at the model's pose has in front of the gate."""
    tagged = set(tr.tags.values())
    return [j for j in range(tr.n_lm) if j in tagged and pose_distance(tr, j) < GATE]


def informed_in_gate(tr):
    """(`a`, the tail's `mid`) for window one.  The start's landmark 12 lies 1.3 m from the pose: where a call has moved the
    pose away from it (a split does, by decimetres) the highest informed landmark BELOW it that is in range stands in -- its
    bound is lower still --, and likewise the lowest one in range for `a`."""
    informed = set(int(l) for l in pb.loose_landmarks(tr.cov, INIT_VAR)[1])
    near = [j for j in tags_in_gate(tr) if j in informed and j <= tail_mid(tr)]
    assert len(near) >= 2, near
    return near[0], near[-1]


def loose_in_gate(tr):
    """The landmark window two names beside landmark 0: `pick`'s loose landmark where it carries a tag in front of the gate;
    else the tagged loose landmark nearest to the pose; where no tagged loose landmark is in range (behind copy_from), the
    highest-indexed tagged landmark in range."""
    near = tags_in_gate(tr)
    never = pick(tr)[1]
    if never in near:
        return never
    loose = [j for j in near if j in pb.loose_landmarks(tr.cov, INIT_VAR)[0]]
    return min(loose, key=lambda j: pose_distance(tr, j)) if loose else max(near)


def detection_window(drv, rng, lms, unknown=()):
    """A two-frame window of the tags of landmarks `lms` and the ids `unknown`, and the assertion that the model's association
    matches exactly `lms` and reports exactly `unknown`.  -> (window, unmatched ids)."""
    tr = drv.model.tr
    tag_of = {j: t for t, j in tr.tags.items()}
    ids = [tag_of[j] for j in dict.fromkeys(lms)] + list(unknown)
    win = fz.window_of(rng, tr, ids, {t: (0.2, 0.8) for t in unknown}, 2)
    tags, unmatched = frontend.associate_known(win, tr.tags, tr.mean[:3], tr.cfg.gate_range, tr.cfg.ignore_tags,
                                               n_landmarks=tr.n_lm)
    assert sorted(tags) == sorted(set(lms)) and unmatched == list(unknown), (sorted(tags), lms, unmatched)
    assert all(t[4] < tr.cfg.gate_range - 0.05 for t in tags.values())             # (well inside the gate: no decision near it)
    return win, unmatched


def op_localize_detections(drv, rng):
    tr = drv.model.tr
    new = next(i for i in range(600, 1024) if i not in tr.tags)
    drv.localize_detections(0.004, 0.02, *detection_window(drv, rng, informed_in_gate(tr), [new]))
    tr = drv.model.tr
    low = 0 if 0 in tags_in_gate(tr) else informed_in_gate(tr)[0]
    drv.localize_detections(0.004, 0.005, *detection_window(drv, rng, [low, loose_in_gate(tr)]))


# ---- a hypothesis bank made behind A, stepped, and adopted back -----------------------------------------------------------------
# ekf_hyp_create takes the slot's bound from the host mirror after flush_pending, k_hyp_rows updates only below it, and
# ekf_hyp_adopt writes the bound's mirrors itself: the only way a pose part written OUTSIDE the handle comes back into it.  Three
# hypotheses on the target's map as A left it; step one shares the part-one observations (`a` and the tail's `mid`), step two
# names the loose landmark; then one hypothesis is adopted and the bank closed.  The model is two localize1 calls.
HYP_COUNT = 3
HYP_MOTION = ((0.004, 0.02), (0.004, 0.005))
HYP_OFF = (0.5, 1.0)                                                # the reset hypothesis: half a metre and one radian off
HYP_COV = np.diag([0.03 ** 2, 0.03 ** 2, 0.015 ** 2])               # the reset hypothesis' pose block
RESAMPLE_U, SPLIT = 0.5, 0.3
PLAN_MARGIN = 1e-6


def hyp_parts(drv, rng):
    """((idx, zr, zb) of part one, (idx, zr, zb) of part two), both as the model's mean sees them now."""
    tr = drv.model.tr
    a, never, _ = pick(tr)
    return tuple((idx,) + tuple(localize_obs(drv, rng, idx)) for idx in ([a, tail_mid(tr)], [0, never]))


def reset_offset(tr, one):
    """Half a metre and one radian off the model's pose, in the direction (of eight) and the sense (of two) in which the
    part-one observations weigh the reset hypothesis LEAST against one that stays.  The table's meas_sigma is 0.7 (metres and
    radians): two observations seen a radian off cost a hypothesis one to three units of log-likelihood, no more, and in an
    unlucky direction the bearing the half metre adds cancels the radian.  The plan needs its weight below 1 / 6 of the sum."""
    stay, log = (tr.mean, tr.cov), []
    lcm.literal_step(*stay, *HYP_MOTION[0], *one, tr.cfg, log=log)
    ll, offs = {}, {}
    for k in range(8):
        for sense in (1.0, -1.0):
            offs[k, sense] = np.array([HYP_OFF[0] * np.cos(k * np.pi / 4), HYP_OFF[0] * np.sin(k * np.pi / 4), sense * HYP_OFF[1]])
            mean, cov, log0 = tr.mean.copy(), tr.cov.copy(), []
            mean[:3] = mean[:3] + offs[k, sense]
            cov[:3, :], cov[:, :3] = 0.0, 0.0
            cov[:3, :3] = HYP_COV
            lcm.literal_step(mean, cov, *HYP_MOTION[0], *one, tr.cfg, log=log0)
            ll[k, sense] = sm.loglik(log0)
    return offs[min(ll, key=ll.get)]


def op_hyp_adopt(drv, rng):
    """Step two gives one list per hypothesis: hypothesis 1, the one adopted, the part-two observations; 0 and 2 two informed
    landmarks each, all four distinct, so that a list handed to the wrong hypothesis shows."""
    one, two = hyp_parts(drv, rng)
    informed = [int(l) for l in pb.loose_landmarks(drv.model.tr.cov, INIT_VAR)[1] if l not in two[0]]
    lists = [(idx,) + tuple(localize_obs(drv, rng, idx)) for idx in (informed[2:4], informed[4:6])]
    drv.hyp_adopt(HYP_MOTION, one, [lists[0], two, lists[1]], 1)


def op_hyp_resample_adopt(drv, rng):
    """Hypothesis 0 is reset half a metre and one radian off before step one: its rows are zero and its own bound is 3, where
    hypotheses 1 and 2 carry the slot's.  resample(u = 0.5, split = 0.3) leaves it no offspring, slot 0 takes hypothesis 1's
    bound, rows and record (k_hyp_copy) and is split (k_hyp_split); step two names the loose landmark, and slot 0 is adopted."""
    one, two = hyp_parts(drv, rng)
    pose0 = drv.model.tr.mean[:3] + reset_offset(drv.model.tr, one)
    drv.hyp_resample_adopt(HYP_MOTION, one, two, pose0, HYP_COV, RESAMPLE_U, SPLIT, rng.standard_normal((HYP_COUNT, 3)))


# (the localisation operations are APPENDED, three and then three more: the pairs before them keep their ids and their draws)
OPS = (("step", op_step), ("run_stream", op_run_stream), ("step_detections", op_step_detections),
       ("predict_linear", op_predict_linear), ("predict_dense", op_predict_dense), ("update_direct", op_update_direct),
       ("update_linear", op_update_linear), ("transform", op_transform), ("transform(cov)", op_transform_cov),
       ("join", op_join), ("join(explicit)", op_join_explicit), ("remove_landmarks", op_remove),
       ("add_landmarks", op_add), ("copy_from", op_copy), ("active_bound off/on", op_bound_off),
       ("localize", op_localize), ("localize_update", op_localize_update), ("run_localize", op_run_localize),
       ("localize_detections", op_localize_detections), ("hyp_adopt", op_hyp_adopt),
       ("hyp_resample_adopt", op_hyp_resample_adopt))
LOCALIZE_OPS = ("localize", "localize_update", "run_localize", "localize_detections", "hyp_adopt", "hyp_resample_adopt")
PAIRS = [(a, b) for a in range(len(OPS)) for b in range(len(OPS))]


def pair_name(a, b):
    return f"{OPS[a][0]} then {OPS[b][0]}"


def setup(drv):
    """What every case starts from: the block-diagonal start, the start's tags, the default active bound."""
    s = start()
    drv.set_option("active_bound", 1)
    drv.set_state_diag(s[0], s[1])
    drv.set_tag_index({TAG0 + j: j for j in range(N_LANDMARKS)})


def prelude(drv):
    s = start()
    k = STREAM_STEPS
    drv.run_stream(*[x[:k] for x in s[2:]])
    for k in range(STREAM_STEPS, STREAM_STEPS + SINGLE_STEPS):
        drv.step1(s[2][k], s[3][k], s[4][k], s[5][k], s[6][k])


def continuation(drv, rng):
    op_step(drv, rng)
    stream(drv, rng, 4, 3)


def run_case(drv, a, b, judge=None):
    """setup, prelude, A, B, continuation on the driver; `judge(stage)` after the prelude ("start": before A; a filter's judge
    must not read the state there, ranks are pending), after A, after B and after the continuation ("A", "B", "end")."""
    rng = np.random.default_rng([SEED, a, b])
    judge = judge or (lambda stage: None)
    setup(drv)
    prelude(drv)
    judge("start")
    OPS[a][1](drv, rng)
    judge("A")
    OPS[b][1](drv, rng)
    judge("B")
    continuation(drv, rng)
    judge("end")


def as_got(model):
    """A model's state as a `got`: NumPy's products leave the last bits of P_ij and P_ji apart, and the judge demands of `got`
    the exact symmetry the device gives."""
    mean, cov, tags = model.state()
    cov = np.asarray(cov, dtype=float)
    return np.asarray(mean, dtype=float), (cov + cov.T) / 2, tags, 0


def model_bound(tr):
    """The active bound the model's history implies: past the highest landmark correlated with anything."""
    seen = np.flatnonzero(tr.seen)
    return 3 + 2 * (int(seen[-1]) + 1) if len(seen) else 3


def keep_rows_beyond(before, after, bound):
    """What a pass -- or a query -- that skips every row at or beyond `bound` leaves: those rows and columns (and means) as
    they were.  `before`'s covariance is symmetrised first (a model's products leave the last bits of P_ij and P_ji apart)."""
    mean, cov = np.array(after[0]), np.array(after[1])
    was = (np.asarray(before[1]) + np.asarray(before[1]).T) / 2
    mean[bound:], cov[bound:, :], cov[:, bound:] = before[0][bound:], was[bound:, :], was[:, bound:]
    return mean, cov


# ---- one operation, then the read-only queries (tests/test_gpu_queries_after_calls.py) -----------------------------------------
# The tail: single steps that each see landmark 0 and ONE mid-map informed landmark, mid = min(12, n_lm - 3) (copy_from leaves
# 12 landmarks).  Their own bound, 3 + 2 (mid + 1), lies far below the bound A left: a query behind them is right only if the
# bound A established reaches it.  TAIL_STEPS: two, and one more where the second would land exactly on the rank limit and
# leave nothing pending on the general kernels (the prelude's story) -- no case needs it with these draws.
TAIL_STEPS = {}


def tail_mid(tr):
    return min(12, tr.n_lm - 3)


def tail_bound(tr):
    return 3 + 2 * (tail_mid(tr) + 1)


def query_name(a):
    return OPS[a][0]


def run_query_case(drv, a, judge=None):
    """setup, prelude, A, the tail; `judge(stage)` after the prelude ("start": ranks are pending), after A ("A") and after the
    tail ("tail": the last, and the only one that may download).  Draws from its own generator: the 225 pairs stay what they
    are."""
    rng = np.random.default_rng([SEED, a, 99])
    judge = judge or (lambda stage: None)
    setup(drv)
    prelude(drv)
    judge("start")
    OPS[a][1](drv, rng)
    judge("A")
    for _ in range(TAIL_STEPS.get(OPS[a][0], 2)):
        observe(drv, rng, [0, tail_mid(drv.model.tr)])
    judge("tail")


QUERY_OBS = 4           # observations per associate() query


def query_rngs(a):
    """(the generator of the associate() observations, the generator of joint()'s permutations) of case a."""
    return np.random.default_rng([11, a]), np.random.default_rng([12, a])


def query_obs(rng, mean):
    """QUERY_OBS unlabelled observations: range and bearing of a random landmark from `mean`, the landmark moved by 0.05 m per
    axis and the bearing by 0.02 rad (test_gpu_associate's obs_around, for one trajectory)."""
    N = (len(mean) - 3) // 2
    zr, zb = np.zeros(QUERY_OBS), np.zeros(QUERY_OBS)
    for q in range(QUERY_OBS):
        l = int(rng.integers(N))
        d = mean[3 + 2 * l:5 + 2 * l] - mean[:2] + rng.normal(0, 0.05, 2)
        zr[q] = np.hypot(*d)
        zb[q] = orc.wrap_pi(np.arctan2(d[1], d[0]) - mean[2] + rng.normal(0, 0.02))
    return zr, zb


def query_selection(tr):
    """The three landmarks of the second joint(): the highest one under the model's bound, a loose one and the tail's `mid` --
    distinct; where the map has no (other) loose landmark, or two of them coincide, the lowest landmarks not yet named."""
    top = (model_bound(tr) - 3) // 2 - 1
    loose = [int(l) for l in pb.loose_landmarks(tr.cov, INIT_VAR)[0] if l != top]
    sel = list(dict.fromkeys([max(top, 0)] + loose[:1] + [tail_mid(tr)]))
    return sel + [l for l in range(tr.n_lm) if l not in sel][:3 - len(sel)]


def sub_idx(sel):
    """State indices of joint(sel)'s sub-state: the pose, then the landmarks in the order given."""
    return [0, 1, 2] + [3 + 2 * int(j) + d for j in sel for d in range(2)]


def unpermute(sel, mean, cov):
    """joint(sel) of ALL landmarks in some order, as the whole state: (mean, covariance) in the state's own order."""
    ix = np.array(sub_idx(sel))
    m, P = np.empty(len(ix)), np.empty((len(ix), len(ix)))
    m[ix], P[np.ix_(ix, ix)] = mean, cov
    return m, P


def new_model(dtype=np.float64):
    s = start()
    return sm.bank(s[0], s[1], sources(), dtype)
