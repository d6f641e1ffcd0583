"""CPU: the geometry case table (tests/geometry_cases.py) against its longdouble model (tests/geometry_model.py).

Conditions, asserted for every script -- they make the table fit to judge a device by, they are not measurements of one:
  * outside the exact-boundary group every unwrapped bearing residual, and theta + ang wherever the arc branch wraps it, keeps
    1e-6 or more from every odd multiple of pi (so no implementation within 1e-9 of the model can land on the other side);
    the same for the scripts run as localisation (frozen map: the filter moves otherwise, so do its residuals) and for every
    (observation, landmark) pair the association test scores;
  * the float64 oracle agrees with the model: bearing innovation 1e-12 absolute, range innovation 1e-12 of the range, S, NIS and H
    1e-12 relative per block, pose 1e-12, pose block and final state 1e-11 per block (parity_blocks' blocks; its two per-entry
    maxima, which a 1e4 prior collapsing to 0.5 leaves at 1e4 eps / 0.5 in float64, at parity_blocks.PATH_CORR_TOL).
Mutants of the float64 oracle -- the slips the device copies could carry -- must each FAIL the judge the GPU module uses
(geometry_model.judge at geometry_cases.DEVICE_BARS) on a named script.
"""
import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests import geometry_cases as gc
from tests import geometry_model as gm
from tests.gated_oracle import block_err
from tests.parity_blocks import PATH_CORR_TOL

CPU_BARS = dict(y=1e-12, S=1e-12, nis=1e-12, H=1e-12, pose=1e-12, pose_block=1e-11, state=1e-11, state_entry=PATH_CORR_TOL)
MARGIN = 1e-6
SCRIPTS = {s.name: s for s in gc.all_scripts()}


# ---- the float64 oracle as a Run, with the two scalar pieces replaceable ---------------------------------------------------------
def oracle_run(script, motion_model=orc.motion_model, innovation_and_h5=orc.innovation_and_h5):
    """orc.ekf_step_dense over the script, restated so that it keeps every update's y, S, NIS and h5 and every step's pose row
    (tests/gated_oracle.py's form), the motion model and the linearisation handed in."""
    cfg = script.cfg
    mean, cov = script.mean0.copy(), script.cov0.copy()
    n = len(mean)
    Q = np.diag(cfg.meas_noise_diag())
    obs_log, poses = [], []
    for lin, ang, obs in script.steps:
        pose, G = motion_model(mean[0:3], lin, ang, cfg)
        if not cfg.disable_motion_model:
            mean[0:3] = pose
        GF = np.eye(n)
        GF[0:3, 0:3] = G
        cov = GF @ cov @ GF.T
        cov[0:3, 0:3] += np.diag(cfg.motion_noise_diag())
        row = []
        for j, zr, zb in (obs if cfg.enable_measurement_model else ()):
            t = 3 + 2 * j
            y, h5 = innovation_and_h5(mean[0:3], mean[t:t + 2], zr, zb)
            H = np.zeros((2, n))
            H[:, 0:3] = h5[:, 0:3]
            H[:, t:t + 2] = h5[:, 3:5]
            S = H @ cov @ H.T + Q
            K = cov @ H.T @ np.linalg.inv(S)
            row.append((j, y.copy(), S, float(y @ np.linalg.solve(S, y)), h5))
            mean = mean + K @ y
            cov = (np.eye(n) - K @ H) @ cov
        obs_log.append(row)
        poses.append((mean[0:3].copy(), cov[0:3, 0:3].copy()))
    return gm.Run(obs_log, poses, mean, cov)


_REFS = {}


def reference(name):
    if name not in _REFS:
        _REFS[name] = gm.run(SCRIPTS[name])
    return _REFS[name]


# ---- the table's shape -----------------------------------------------------------------------------------------------------------
def test_table_shape():
    """Banks of at most 16 under one config, twelve steps of at most four observations over twelve landmarks, stream scripts
    with more than 40 updates, at most 8 exact-boundary observations, every range / direction / bearing edge somewhere at
    position 0 and at a later one, at a cadence's head (steps 0 and 10) and inside one -- but the millimetre ranges, which float64
    itself holds to the conditions only in a script's first update."""
    names = [s.name for s in gc.all_scripts()]
    assert len(set(names)) == len(names) and [b for b, _ in gc.banks()] == list(gc.BANK_NAMES)
    exact = 0
    for _, scripts in gc.banks():
        assert len(scripts) <= 16
        for s in scripts:
            assert len(s.steps) == gc.K and len(s.mean0) == gc.NS and s.cov0.shape == (gc.NS, gc.NS)
            assert all(len(o) <= 4 and all(0 <= j < gc.N for j, _, _ in o) for _, _, o in s.steps)
            if s.exact:
                exact += 1
                assert s.updates == 1 and len(s.steps[-1][2]) == 1
            elif "unobserved" not in s.name:
                assert s.updates > 40, (s.name, s.updates)
    assert 0 < exact <= 8
    where = {}
    for s in gc.all_scripts():
        for k, i, what in s.edges:
            key = what.split(",")[0] if what.startswith("first") else what
            where.setdefault(key, set()).add((k in (0, 10), i == 0))
    for r in gc.RANGES[2:]:
        got = where[f"first observation at {r:g} m"]
        assert {h for h, _ in got} == {True, False} and {p for _, p in got} == {True, False}, (r, got)
    for r in gc.RANGES[:2]:                                    # millimetres: a script's first update only (geometry_cases.NEAR)
        assert where[f"first observation at {r:g} m"] == {(True, True)}
    seen = {(r, round(phi, 6)) for s in gc.all_scripts() for r, phi in [gc.first_place(w) for _, _, w in s.edges if w.startswith("first")]}
    assert {(r, round(phi, 6)) for r, phi in gc.COMBOS} <= seen    # every range in every world direction
    for cfg_thr, edges in ((gc.THR, (gc.THR, gc.NX, gc.UNDER)), (gc.THR_WIDE, (gc.THR_WIDE, gc.NX_WIDE, gc.UNDER_WIDE))):
        for e in edges:                                        # every threshold edge of ang, either sign, with lin of both signs
            for sign in (1.0, -1.0):
                lins = {np.sign(lin) for s in gc.all_scripts() if s.cfg.arc_threshold == cfg_thr and s.cfg.enable_circular_interpolation
                        and not s.cfg.disable_motion_model for lin, ang, _ in s.steps if ang == sign * e}
                assert {1.0, -1.0} <= lins or (e in (gc.UNDER, gc.UNDER_WIDE) and sign < 0), (e, sign, lins)   # (-UNDER: not in the table)
    for e in gc.EXTRAS:
        got = where[f"bearing {e:+.6f} on the true one"]
        assert got == {(True, True), (True, False), (False, True), (False, False)}, (e, got)


def test_wraps_happen_where_the_table_says():
    """theta + ang leaves [-pi, pi) upwards and downwards, at a cadence's head (steps 0 and 10) and inside one; in linear mode
    |theta| exceeds 30 before the first observed step of the runaway script, and theta stays beyond 30 under set_state(40)."""
    seen = set()
    for s in gc.all_scripts():
        for k, rec in enumerate(reference(s.name).recs):
            if rec.theta_sum is not None and abs(rec.theta_sum) > gm.PI:
                seen.add((rec.theta_sum > 0, k in (0, 10)))
    assert seen == {(True, True), (True, False), (False, True), (False, False)}, seen
    recs = reference("linear mode: theta runs away to -38 unobserved").recs
    assert abs(recs[4].pose[2]) > 30 and not recs[4].obs and recs[5].obs
    assert all(abs(r.pose[2]) > 30 for r in reference("linear mode: theta 40, ranges and directions").recs)
    assert all(abs(r.pose[2]) > 30 for r in reference("theta 40 set through set_state").recs[:3])


# ---- conditions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCRIPTS))
def test_conditions(name):
    s, ref = SCRIPTS[name], reference(name)
    if not s.exact:
        for k, rec in enumerate(ref.recs):
            assert rec.theta_sum is None or gm.pi_margin(rec.theta_sum) >= MARGIN, (k, rec.theta_sum)
            for i, r in enumerate(rec.residuals):
                assert gm.pi_margin(r) >= MARGIN, (k, i, r)
    w = gm.judge(oracle_run(s), ref, CPU_BARS, what=name + ": ", range_relative=True)
    print(name + ": " + " ".join(f"{k}={v:.1e}" for k, v in w.items()))


@pytest.mark.parametrize("name", list(SCRIPTS))
def test_conditions_as_localisation(name):
    """On a frozen map the pose takes every correction alone and the residuals are others: they too keep clear of +-pi."""
    s = SCRIPTS[name]
    for k, rec in enumerate(gm.localize_reference(s).recs):
        for i, o in enumerate(rec.obs):
            assert s.exact or np.pi - abs(float(o[1][1])) >= MARGIN, (k, i, o[1][1])


NIS_FLOOR = 1e-4           # y within ~1e-14 of an innovation of >= 1e-2: a NIS of 1e-4 can be held to 1e-10 relatively
SEPARATION = 1e-6          # of max(1, |d|): a thousand times what the association bars let a score move


@pytest.mark.parametrize("name", [n for n, s in SCRIPTS.items() if not s.exact and s.cfg.enable_measurement_model])
def test_conditions_of_the_association_scores(name):
    """geometry_cases.association_observations against every landmark at the oracle's final state: every pair's residual clear of
    +-pi, every NIS large enough to be held relatively, and per observation the three smallest d = NIS + ln det S apart by more than
    the bars can move them -- so that the GPU module asserts the two best candidates of every observation, unconditionally."""
    s = SCRIPTS[name]
    run = oracle_run(s)
    zr, zb = gc.association_observations(s)
    nis, logdet, res = gm.associate_scores(run.mean, run.cov, zr, zb, s.cfg)
    assert (np.abs(res.astype(float)) <= np.pi - MARGIN).all()
    assert np.isfinite(logdet.astype(float)).all() and float(nis.min()) >= NIS_FLOOR, float(nis.min())
    d = (nis + logdet[None, :]).astype(float)
    for q in range(len(zr)):
        best = np.sort(d[q])[:3]
        assert (np.diff(best) > SEPARATION * np.maximum(1.0, np.abs(best[:2]))).all(), (q, best)


# ---- the bare formulas -----------------------------------------------------------------------------------------------------------
def test_bare_formulas():
    """orc.motion_model and orc.innovation_and_h5 alone against the model, from identical float64 inputs, over the table's edges.
    Bounds from the formats, not from a run: the bearing innovation takes three roundings at the magnitude of theta (atan2 - theta,
    z_b - that, + pi) and loses 2 pi_d - 2 pi = 2.4e-16 per turn the wrap takes off; the range innovation and H a few eps of
    themselves; the arc branch |lin / ang| eps per term (3.9e-12 at lin = 5 just above the threshold: why lin stays <= 0.5).
    The figures are printed (profiles/geometry_edges.txt)."""
    cfg = orc.EkfConfig()
    eps = np.finfo(float).eps
    worst = {}
    for th in (0.0, 3.1, -3.1, 40.0, -1000.0):
        pose = np.array([0.3, -0.2, th])
        w = worst.setdefault(abs(th), dict(y0=0.0, y1=0.0, H=0.0, arc=0.0, theta=0.0))
        for r, phi in gc.COMBOS:
            l = pose[0:2] + r * np.array([np.cos(phi), np.sin(phi)])
            d = l - pose[0:2]
            true_b = float(orc.wrap_pi(np.arctan2(d[1], d[0]) - th))
            for e in gc.EXTRAS:
                y, h5 = orc.innovation_and_h5(pose, l, 1.01 * r, true_b + e)
                my, mh = gm.innovation_and_h5(pose, l, 1.01 * r, true_b + e)
                assert gm.pi_margin(gm.unwrapped_residual(pose, l, true_b + e)) >= MARGIN
                w["y0"] = max(w["y0"], float(abs(y[0] - my[0])) / float(np.hypot(d[0], d[1])))
                w["y1"] = max(w["y1"], float(abs(y[1] - my[1])))
                w["H"] = max(w["H"], block_err(h5[:, [0, 1, 3, 4]].reshape(2, 2, 2), mh[:, [0, 1, 3, 4]].astype(float).reshape(2, 2, 2)))
        for lin in (0.12, -0.5, 0.5):
            for ang in (gc.NX, -gc.NX, 0.3, -7.0):
                if gm.pi_margin(gm.LD(th) + gm.LD(ang)) < MARGIN:
                    continue
                p, G = orc.motion_model(pose, lin, ang, cfg)
                mp, mG = gm.motion_model(pose, lin, ang, cfg)
                # -r sin(theta) + r sin(theta + ang): per term r, the sine, the product and the sum round at eps / 2 of |r|, and
                # theta + ang rounds at ulp(|theta|) / 2 inside the second sine: within 2 (|theta| + 4) eps |r| for the two terms
                w["arc"] = max(w["arc"], float(np.max(np.abs(p[0:2] - mp[0:2]))) / (abs(lin / ang) * (abs(th) + 4) * eps))
                w["theta"] = max(w["theta"], float(abs(p[2] - mp[2])))
        print(f"bare formulas, |theta| = {abs(th):g}: " + " ".join(f"{k}={v:.1e}" for k, v in w.items()))
        turns = abs(th) / 6.28 + 3
        assert w["y0"] <= 4 * eps and w["H"] <= 4 * eps
        assert w["y1"] <= 2 * (abs(th) + 16) * eps + turns * 2.5e-16
        assert w["theta"] <= (abs(th) + 8) * eps + turns * 2.5e-16
        assert w["arc"] <= 2.0


# ---- mutants ---------------------------------------------------------------------------------------------------------------------
def _motion(ge=False, wrap=orc.wrap_pi, wrap_arc=True, advance_straight=False):
    def motion_model(pose, lin, ang, cfg):
        th = pose[2]
        G = np.eye(3)
        new = np.array(pose[:3], dtype=float)
        if cfg.disable_motion_model:
            return new, G
        straight = abs(ang) < cfg.arc_threshold if ge else abs(ang) <= cfg.arc_threshold
        if cfg.enable_circular_interpolation and not straight:
            r = lin / ang
            new = new + np.array([-r * np.sin(th) + r * np.sin(th + ang), r * np.cos(th) - r * np.cos(th + ang), ang])
            if wrap_arc:
                new[2] = wrap(new[2])
            G[0, 2] = -r * np.cos(th) + r * np.cos(th + ang)
            G[1, 2] = -r * np.sin(th) + r * np.sin(th + ang)
        else:
            adv = ang if (advance_straight or not cfg.enable_circular_interpolation) else 0.0
            new = new + np.array([lin * np.cos(th), lin * np.sin(th), adv])
            G[0, 2] = -lin * np.sin(th)
            G[1, 2] = lin * np.cos(th)
        return new, G
    return motion_model


def _innovation(wrap=orc.wrap_pi, h_scale=1.0, swapped=False):
    def innovation_and_h5(pose3, lm2, z_range, z_bearing):
        d = lm2 - pose3[0:2]
        q = d @ d
        sq = np.sqrt(q)
        at = np.arctan2(d[0], d[1]) if swapped else np.arctan2(d[1], d[0])
        y = np.array([z_range - sq, wrap(z_bearing - (at - pose3[2]))])
        h5 = np.array([[-sq * d[0], -sq * d[1], 0.0, sq * d[0], sq * d[1]], [d[1], -d[0], -q, -d[1], d[0]]], dtype=float) / q
        return y, h5 * h_scale
    return innovation_and_h5


def wrap_upper_closed(a):
    """into (-pi, pi]"""
    return np.pi - (np.pi - a) % orc.TWO_PI


def wrap_truncating(a):
    """C fmod: the remainder takes the dividend's sign"""
    return np.fmod(a + np.pi, orc.TWO_PI) - np.pi


def wrap_one_turn(a):
    """one fix-up either way: right only while theta and the bearing lie in [-pi, pi)"""
    return a - orc.TWO_PI if a >= np.pi else (a + orc.TWO_PI if a < -np.pi else a)


MUTANTS = {
    ">= at the threshold": (dict(motion_model=_motion(ge=True)), "motion edges from theta 0"),
    "a wrap into (-pi, pi]": (dict(motion_model=_motion(wrap=wrap_upper_closed), innovation_and_h5=_innovation(wrap=wrap_upper_closed)),
                              "exact boundary, landmark at -0.75, bearing 0"),
    "a wrap with truncating remainder": (dict(motion_model=_motion(wrap=wrap_truncating),
                                              innovation_and_h5=_innovation(wrap=wrap_truncating)),
                                         "over -pi from -3.1, step 10 cut"),
    "a truncating remainder on the measurement side alone": (dict(innovation_and_h5=_innovation(wrap=wrap_truncating)),
                                                             "bearing edges at tame ranges, theta 0"),
    "no wrap on the arc branch": (dict(motion_model=_motion(wrap_arc=False)), "over +pi from 3.1"),
    "theta advanced on the straight branch": (dict(motion_model=_motion(advance_straight=True)), "motion edges from theta 0"),
    "H scaled by 1 + 3e-8": (dict(innovation_and_h5=_innovation(h_scale=1 + 3e-8)), "motion edges from theta 0"),
    "arctan2(dx, dy)": (dict(innovation_and_h5=_innovation(swapped=True)), "ranges and directions 0, theta 0"),
    "the bearing not re-wrapped when theta is outside [-pi, pi)": (dict(innovation_and_h5=_innovation(wrap=wrap_one_turn)),
                                                                   "theta 40 set through set_state"),
}


def test_the_restated_oracle_is_the_oracle():
    """oracle_run with its defaults, and with the mutants' rebuilt pieces switched to no mutation, gives the oracle's own bits."""
    for name in ("motion edges from theta 0", "ranges and directions 1, theta 3.1", "linear mode: motion edges"):
        s = SCRIPTS[name]
        a, b = oracle_run(s), oracle_run(s, motion_model=_motion(), innovation_and_h5=_innovation())
        om, oP = s.mean0.copy(), s.cov0.copy()
        for lin, ang, obs in s.steps:
            om, oP = orc.ekf_step_dense(om, oP, lin, ang, [o[0] for o in obs], [o[1] for o in obs], [o[2] for o in obs], s.cfg)
        assert np.array_equal(a.mean, om) and np.array_equal(a.cov, oP)
        assert np.array_equal(a.mean, b.mean) and np.array_equal(a.cov, b.cov)


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutants_fail_the_device_judge(mutant):
    pieces, name = MUTANTS[mutant]
    s, ref = SCRIPTS[name], reference(name)
    bars = gc.DEVICE_BARS
    gm.judge(oracle_run(s), ref, bars, what=name + ": ")            # the oracle itself passes the judge on this script
    with pytest.raises(AssertionError):
        gm.judge(oracle_run(s, **pieces), ref, bars, what=f"{mutant} on {name}: ")


# ---- detections ------------------------------------------------------------------------------------------------------------------
def test_detection_windows():
    """Tags ahead, abeam and behind, all inside the gate; the model's residuals clear of +-pi."""
    refs = gc.detection_reference()
    zs = [z for _, _, wins in gc.detection_windows() for w in wins for _, tags in w for _, _, z in tags]
    assert min(zs) < -1.0 and max(zs) > 1.0 and any(abs(z) <= 1e-2 for z in zs)
    for b, ref in enumerate(refs):
        brg = [t[5] for tags in ref.tags for t in tags.values()]
        assert max(brg) > 2.5 and min(brg) < -2.5 or b == 1, (b, brg)
        for tags in ref.tags:
            assert all(t[4] <= 1.5 for t in tags.values())
        for rec in ref.recs:
            assert all(gm.pi_margin(r) >= MARGIN for r in rec.residuals)
            assert rec.theta_sum is None or gm.pi_margin(rec.theta_sum) >= MARGIN
