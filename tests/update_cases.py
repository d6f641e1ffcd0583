"""The inputs of tests/test_gpu_update_rows.py and the block-wise reference of ONE direct or linear update (no GPU imports:
tests/test_update_blocks_cpu.py reads the same table and shows on the oracle's states that every case is admissible -- the
simple and the Joseph form of the reference agree on every active-part piece to 1e-11, so that TIGHT on the GPU is a statement
about device code).

Bases (BASES): a bank of streams from a block-diagonal start whose first `steps` steps run before the call; the landmarks at
and beyond `nobs` are never observed (variance landmark_init_var).  Cases are drawn around the ORACLE's state after those steps
(`oracle_state`); the GPU tests apply the model to the device's own state() just before the call, which differs from the
oracle's by rounding.
"""
import functools

import numpy as np

from oracle import ekf_oracle as orc
from tests import direct_model as dm
from tests import linear_model as lm
from tests import parity_blocks as pb

INIT_VAR = orc.EkfConfig().landmark_init_var
TIGHT = 1e-9
FORMS_TOL = 1e-11       # the two forms of the reference on every active-part piece (admissibility of a case's inputs)
POSE, POSITION = dm.POSE, dm.POSITION

# name: (N, landmarks the stream observes, steps before the call, further steps of the uploaded stream, m, trajectories, seed)
BASES = {
    # N = 40 (n = 83: the general kernels), 25 steps of m = 4 over landmarks 0 .. 33 (every one observed about three times:
    # P is dense), landmarks 34 .. 39 never observed; 11 further steps for the life after the call
    "n40": (40, 34, 25, 11, 4, 1, 700),
    "n40x4": (40, 34, 25, 0, 4, 4, 710),
    # N = 150: landmarks 0 .. 119 observed (active bound 243: two slabs of 128 rows), 120 .. 149 never
    "n150x3": (150, 120, 30, 0, 4, 3, 720),
    "n150x8": (150, 120, 30, 0, 4, 8, 730),
    # 208 x N = 190 (n = 383, three slabs): the smallest bank plan_pass sends to the row-slab pass by itself
    # (tests/test_gpu_fuzz_features.py); 25 steps of m = 8 = 5 whole cadences of 40 landmark updates, nothing pending behind them;
    # 24 steps leave 32 updates pending
    "n190x208": (190, 190, 25, 0, 8, 208, 740),
}


@functools.lru_cache(maxsize=None)
def stream(base, b):
    """Trajectory b's stream of the base: synthetic_stream over the observed landmarks, the state extended by the
    never-observed ones (dm.small_stream's pattern)."""
    N, nobs, steps, more, m, B, seed = BASES[base]
    assert 0 <= b < B
    s = orc.synthetic_stream(nobs, steps + more, m, seed + b)
    rng = np.random.default_rng(seed + 5000 + b)
    mean0 = np.concatenate([s[0], rng.uniform(-1.0, 1.0, 2 * (N - nobs))])
    diag0 = np.concatenate([s[1], np.full(2 * (N - nobs), INIT_VAR)])
    return (mean0, diag0) + tuple(s[2:])


def steps_of(base):
    return BASES[base][2]


@functools.lru_cache(maxsize=None)
def oracle_state(base, b, steps=None):
    """The dense oracle's state of trajectory b after the base's steps (the active part run alone: the never-observed
    landmarks are a closed system of their own and stay at the start)."""
    N, nobs, st, more, m, B, seed = BASES[base]
    s = stream(base, b)
    top = 3 + 2 * nobs
    om, oP = dm.dense_of((s[0][:top], s[1][:top]) + tuple(s[2:]), st if steps is None else steps)
    mean, cov = s[0].copy(), np.diag(s[1])
    mean[:top], cov[:top, :top] = om, oP
    return mean, cov


# ---- the reference of one update on the closed system the call touches ----
def closed_rows(before_P, touched):
    """State indices of the pose, every landmark active in `before_P` and every landmark of `touched`, and the landmark
    renumbering onto them.  A never-observed landmark nobody names is correlated with nothing: the update of the rest does
    not know it (assert_update_close checks that its rows hold exact zeros and come back bit for bit)."""
    active, first, _ = pb.landmark_classes(before_P, touched, INIT_VAR)
    lms = np.sort(np.concatenate([active, first]))
    rows = np.concatenate([np.arange(3), pb.landmark_rows(lms)]).astype(np.int64)
    return rows, {int(l): i for i, l in enumerate(lms)}


def embed(before, rows, sub):
    mean, cov = np.array(before[0], dtype=float), np.array(before[1], dtype=float)
    mean[rows] = sub[0]
    cov[np.ix_(rows, rows)] = sub[1]
    return (mean, cov) + tuple(sub[2:])


def linear_reference(before, meas, innovation=False, gate=np.inf, joseph=True):
    """lm.linear_update_joseph (or the simple form) of `meas` = (landmarks, H, R, r) on the closed system, embedded in
    `before`: (mean, cov, nis, dof, applied).  Equal to the form on the whole state; affordable at N = 2050."""
    lms, H, R, r = meas
    rows, place = closed_rows(before[1], lms)
    fn = lm.linear_update_joseph if joseph else lm.linear_update
    sub = fn(before[0][rows], before[1][np.ix_(rows, rows)], [place[int(l)] for l in lms], H, R, r, innovation, gate)
    return embed(before, rows, sub)


def direct_reference(before, fix, gate=np.inf, joseph=True):
    """dm.direct_update_joseph (or the simple form) of `fix` = (targets, z, R) on the closed system, embedded in `before`."""
    t, z, R = fix
    rows, place = closed_rows(before[1], [x for x in t if x >= 0])
    fn = dm.direct_update_joseph if joseph else dm.direct_update
    sub = fn(before[0][rows], before[1][np.ix_(rows, rows)], [place[int(x)] if x >= 0 else x for x in t], z, R, gate)
    return embed(before, rows, sub)


def forms_disagreement(before, a, j, touched):
    """The block-wise pieces of the simple form `a` against the Joseph form `j` of one update of `before`: the active part
    (pb.PIECES) and, where the call first touches never-observed landmarks, their pieces (pb.UPDATE_PIECES)."""
    active, first, _ = pb.landmark_classes(before[1], touched, INIT_VAR)
    act = np.concatenate([np.arange(3), pb.landmark_rows(active)]).astype(np.int64)
    err = pb.active_errors(a[0][act], a[1][np.ix_(act, act)], j[0][act], j[1][np.ix_(act, act)])
    if len(first):
        fr = pb.landmark_rows(first)
        err["touched_block"] = max(float(np.abs(a[1][r:r + 2, r:r + 2] - j[1][r:r + 2, r:r + 2]).max()) for r in 3 + 2 * first)
        err["touched_mean"] = max(float(np.abs(a[0][r:r + 2] - j[0][r:r + 2]).max() / max(1.0, np.abs(j[0][r:r + 2]).max()))
                                  for r in 3 + 2 * first)
        cols = np.concatenate([act, fr])
        dev = np.abs(a[1][np.ix_(fr, cols)] - j[1][np.ix_(fr, cols)]) / np.sqrt(np.outer(np.diag(j[1])[fr], np.diag(j[1])[cols]))
        for i, r in enumerate(fr):
            own = 3 + 2 * ((r - 3) // 2)
            dev[i, (cols == own) | (cols == own + 1)] = 0.0
        err["touched_cross"] = float(dev.max())
    return err


# ---- a dense H over a never-observed landmark: the entrywise bound ----
# An update whose dense rows tie a never-observed landmark to others cancels landmark_init_var = 1e4 inside entries of the
# active part and of that landmark's cross terms, and the two forms of the reference themselves differ there by ~2e-10
# (correlation-scaled).  No bound has been derived; the GPU is held to TEN times what tests/test_update_blocks_cpu.py measures
# between the two forms on the oracle's state of the same case (one decade: the device sums in another order than either
# form), and below parity_blocks.REL_TOL in any event.  The CPU test repeats the measurement and asserts that the stored
# figures are still its own (within a factor 3: a rounding-level quantity moves with the BLAS's order of summation).
# At most two such cases; every other case takes TIGHT on every piece, a first-touched landmark's cross terms included
# (a constraint between ONE never-observed landmark and an observed one, lm.case_panel, cancels nothing: its forms agree to 4e-16).
# name: (entry_tol -- corr_max and mean_landmarks --, first_cross_tol -- touched_cross)
DENSE_NEVER = {
    # lm.case_bank trajectory 1, D = 32 over 16 landmarks, two of them never observed.  Measured between the forms on the
    # oracle's state: corr_max 2.18e-10, mean_landmarks 9.09e-11, touched_cross 2.14e-10 (the relative Frobenius pieces: pose
    # 5.9e-11, cross 5.8e-11, landmarks 1.1e-11, mean_pose 9.5e-12 -- they stay at TIGHT; touched_block 3.5e-12 against the
    # 7.1e-11 of 32 eps init_var, touched_mean 1.2e-11 against 1e-9).
    "lm.case_bank[1]": (2.2e-9, 2.2e-9),
}


@functools.lru_cache(maxsize=None)
def dense_never_landmarks():
    """name -> the landmark list of each DENSE_NEVER case, in the order its call names them (built once)."""
    _, meas, _ = lm.case_bank()
    return {"lm.case_bank[1]": tuple(int(l) for l in meas[1][0])}


def dense_never_key(landmarks, before_P):
    """The DENSE_NEVER case a call over `landmarks` on a state of covariance `before_P` is (how check_against_model recognises
    it), or None.  Both must hold: the call names the case's very landmarks in the case's order, AND some of them are never
    observed in `before_P` -- what the loosened bound exists for; a call over the same landmarks on a state that has observed
    them all cancels nothing and takes TIGHT."""
    lms = tuple(int(l) for l in landmarks)
    if not len(pb.landmark_classes(before_P, lms, INIT_VAR)[1]):
        return None
    return next((key for key, want in dense_never_landmarks().items() if lms == want), None)


def dense_never_bounds(landmarks, before_P):
    """(entry_tol, first_cross_tol) of a linear call over `landmarks` on a state of covariance `before_P`: the DENSE_NEVER
    case's, (None, TIGHT) for every other."""
    key = dense_never_key(landmarks, before_P)
    return DENSE_NEVER[key] if key else (None, TIGHT)


# ---- linear cases on the base "n40": (D, k, mode) ----
LINEAR_ROWS = [(1, 0, "z"), (3, 1, "innovation"), (4, 0, "z"), (5, 2, "innovation"), (8, 1, "z"), (9, 8, "innovation"),
               (12, 2, "z"), (16, 16, "z"), (17, 8, "innovation"), (31, 16, "innovation"), (32, 8, "z"), (12, 5, "z")]


def rows_cap(D, direct):
    """The instantiation a bank whose largest D this is runs in (csrc/ekf_host_plan.h: front_rows_cap of kpad = D padded
    to 4)."""
    kpad = (D + 3) & ~3
    return 4 if kpad <= 4 else 8 if kpad <= 8 else 16 if kpad <= 16 else (36 if direct else 32)


def linear_case(base, b, D, k, mode, salt=0):
    """D dense rows over the pose and k OBSERVED landmarks in no order: H uniform in [-1, 1], a dense correlated R
    (lm.dense_noise), and a measurement the filter could have expected -- z = H (mean[s] + dx) + v with dx ~ N(0, P[s, s]) and
    v ~ N(0, R), so that the NIS is about D also where D > 3 + 2 k (rows drawn one sigma off independently of each other, as
    lm.dense_rows draws them, contradict one another there: NIS 6000 at D = 32 over 8 landmarks, and the mean then moves by so
    many sigma that the reference's two forms differ by 1.1e-11).  -> (landmarks, H, R, r), r the measurement z or, mode
    "innovation", y = z - H mean[s]."""
    om, oP = oracle_state(base, b)
    nobs = BASES[base][1]
    rng = np.random.default_rng(1000 * D + 10 * k + 7919 * b + salt + BASES[base][6])
    lms = [int(l) for l in rng.permutation(nobs)[:k]]
    if k > 1 and lms == sorted(lms):
        lms = lms[::-1]
    s = lm.sub_indices(lms)
    H = rng.uniform(-1.0, 1.0, (D, len(s)))
    R = lm.dense_noise(rng, D)
    dx = np.linalg.cholesky(oP[np.ix_(s, s)]) @ rng.normal(size=len(s))
    y = H @ dx + np.linalg.cholesky(R) @ rng.normal(size=D)
    return lms, H, R, (H @ om[s] + y if mode == "z" else y)


# ---- direct cases on the base "n40": D -> (head, landmarks, of which never observed) ----
DIRECT_FIXES = {2: (POSITION, 0, 0), 3: (POSE, 0, 0), 4: (POSITION, 1, 1), 5: (POSE, 1, 0), 7: (POSE, 2, 0), 8: (None, 4, 1),
                9: (POSE, 3, 0), 15: (POSE, 6, 0), 16: (POSITION, 7, 1), 17: (POSE, 7, 0), 31: (POSE, 14, 0), 32: (None, 16, 0),
                33: (POSE, 15, 1)}


def direct_case(base, b, D, salt=0, offset_sigmas=1.0):
    """Fixes of D rows: a pose or position fix (or none) in the middle of a list of landmarks in no order, `never` of them
    never observed (surveyed within decimetres of the prior mean, as dm.case_small's): (targets, z, R)."""
    head, nl, never = DIRECT_FIXES[D]
    om, oP = oracle_state(base, b)
    N, nobs = BASES[base][0], BASES[base][1]
    never = min(never, N - nobs)                       # (a base without never-observed landmarks: an observed one instead)
    rng = np.random.default_rng(2000 * D + 7919 * b + salt + BASES[base][6])
    t = [int(l) for l in rng.permutation(nobs)[:nl - never]] + [int(l) for l in nobs + rng.permutation(N - nobs)[:never]]
    t = [t[i] for i in rng.permutation(len(t))]
    if head is not None:
        t.insert(len(t) // 2, head)
    assert len(dm.rows_of(t)) == D
    loose = np.diag(np.where(np.diag(oP) >= INIT_VAR, 0.01, np.diag(oP)))
    z, R = [], []
    for x in t:
        zi, Ri = dm.make_fixes(rng, om, oP if x < 0 or x < nobs else loose, [x], offset_sigmas)
        z, R = z + zi, R + Ri
    return t, z, R


def outlier_linear(base, b, sigmas=10.0):
    """A 2-row pose measurement (x and theta) `sigmas` sigma off on both rows: what a gate rejects."""
    om, oP = oracle_state(base, b)
    H = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    R = lm.dense_noise(np.random.default_rng(31 + b), 2)
    y = sigmas * np.sqrt(np.diag(H @ oP[:3, :3] @ H.T + R))
    return [], H, R, y


def outlier_direct(base, b, sigmas=10.0):
    om, oP = oracle_state(base, b)
    z, R = dm.make_fixes(np.random.default_rng(37 + b), om, oP, [POSITION])
    z[0][:2] = om[:2] + sigmas * np.sqrt(np.diag(oP)[:2] + np.diag(R[0])[:2])
    return [POSITION], z, R


# ---- ragged banks on "n40x4": per trajectory D (linear: and k); trajectory 2 of (b) is the outlier ----
RAGGED_LINEAR = {"a": [(1, 0, "innovation"), (32, 16, "innovation"), (0, 0, "innovation"), (9, 3, "innovation")],
                 "b": [(5, 1, "innovation"), (8, 3, "innovation"), (2, 0, "innovation"), (7, 2, "innovation")]}
RAGGED_DIRECT = {"a": [2, 33, 0, 9], "b": [5, 8, 2, 7]}
LONE = 2                # (c): the one trajectory that brings rows, the others with ranks pending


def ragged_linear(which):
    """-> per trajectory (landmarks, H, R, y) in innovation mode; D = 0 brings ([], (0, 3), (0, 0), ())."""
    out = []
    for b, (D, k, mode) in enumerate(RAGGED_LINEAR[which]):
        if D == 0:
            out.append(([], np.zeros((0, 3)), np.zeros((0, 0)), np.zeros(0)))
        elif which == "b" and b == 2:
            out.append(outlier_linear("n40x4", b))
        else:
            out.append(linear_case("n40x4", b, D, k, mode))
    return out


def ragged_direct(which):
    out = []
    for b, D in enumerate(RAGGED_DIRECT[which]):
        if D == 0:
            out.append(([], [], []))
        elif which == "b" and b == 2:
            out.append(outlier_direct("n40x4", b))
        else:
            out.append(direct_case("n40x4", b, D))
    return out


PASS_LINEAR = (12, 5, "z")      # the linear call of the pass-form cases
PASS_DIRECT = 33                # ... and the direct one


def all_cases():
    """Every (name, kind, base, b, payload, innovation) of tests/test_gpu_update_rows.py, for the admissibility check: the
    rejected outliers are left out (nothing is applied)."""
    out = []
    for D, k, mode in LINEAR_ROWS:
        out.append((f"linear D={D} k={k} {mode}", "linear", "n40", 0, linear_case("n40", 0, D, k, mode), mode == "innovation"))
    for D in DIRECT_FIXES:
        out.append((f"direct D={D}", "direct", "n40", 0, direct_case("n40", 0, D), False))
    for which in ("a", "b"):
        for b, meas in enumerate(ragged_linear(which)):
            if len(meas[3]) and not (which == "b" and b == 2):
                out.append((f"ragged linear ({which}) b={b} D={len(meas[3])}", "linear", "n40x4", b, meas, True))
        for b, fix in enumerate(ragged_direct(which)):
            if len(fix[0]) and not (which == "b" and b == 2):
                out.append((f"ragged direct ({which}) b={b} D={RAGGED_DIRECT[which][b]}", "direct", "n40x4", b, fix, False))
    out.append(("lone linear b=2", "linear", "n40x4", LONE, linear_case("n40x4", LONE, *PASS_LINEAR), False))
    out.append(("lone direct b=2", "direct", "n40x4", LONE, direct_case("n40x4", LONE, PASS_DIRECT), False))
    for base, bs in (("n150x3", range(3)), ("n150x8", range(8)), ("n190x208", range(4))):
        for b in bs:
            out.append((f"{base} linear b={b}", "linear", base, b, linear_case(base, b, *PASS_LINEAR), False))
            out.append((f"{base} direct b={b}", "direct", base, b, direct_case(base, b, PASS_DIRECT), False))
    return out
