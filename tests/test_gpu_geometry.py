"""GPU: motion and measurement geometry at its edges, on every path that runs it.  The paths share the arithmetic itself --
motion_model, linearize_h and innovation (csrc/ekf_devfn.h), the detection walk (csrc/ekf_det_walk.h) -- and differ in how they
fetch the pose, publish the result and order the work around it, which is what each row below names.

The case table of tests/geometry_cases.py -- scripts of twelve steps in banks of up to 16 slots -- runs on every path below, and
every path is judged against the longdouble model of tests/geometry_model.py (localisation: against tests/localize_model.py fed the
same inputs) on every logged y, S and NIS, every pose-log row, the final mean and covariance block by block, and flags == 0:

  step                 the general kernels, "fused_step" 0 and 1          (ekf_kernels.hip solve_body)
  predict + update     the general kernels
  run_stream           fused cadences with "chain" 0; chained solves -- the bank, and one script repeated in 16 slots --; the
                       per-step stream with "fused_cadence" 0             (ekf_solve_cad_body.inc: step heads and cut steps)
  small state          step, and run_stream in one launch                 (ekf_small.hip)
  localisation         localize, localize_update behind predict, run_localize, small state and general kernels (ekf_localize.hip)
  associate(full=True) behind the last step, ranks pending: every candidate's NIS and ln det S, and the two best (ekf_associate.hip)
  step_detections      tags ahead, abeam and behind: range and bearing formed on the device

The path is asserted through gpu_support.counters and conftest.path_ran.  The bars are geometry_cases.DEVICE_BARS (y and pose
absolute, the others relative; 16 x the measured distance, never above the project's 1e-9); no observation is excused but the
exact-boundary scripts' single ones, which are judged on y alone: in [-pi, pi) and equal to the model's modulo 2 pi.  Every test
prints its worst distances from the model: profiles/geometry_edges.txt is that table.
"""
import numpy as np
import pytest

from tests import geometry_cases as gc
from tests import geometry_model as gm
from tests.conftest import path_ran
from tests.gpu_support import REL_TOL, TIGHT, counters, sd  # noqa: F401

pytestmark = pytest.mark.gpu

TOL = gc.DEVICE_TOL
assert TOL <= TIGHT <= REL_TOL
BARS = gc.DEVICE_BARS
K, NS = gc.K, gc.NS

_REFS = {}


def reference(script):
    if script.name not in _REFS:
        _REFS[script.name] = gm.run(script)
    return _REFS[script.name]


def sdcfg(sd, cfg):
    return sd.EkfConfig(motion_sigma=cfg.motion_sigma, meas_sigma=cfg.meas_sigma, arc_threshold=cfg.arc_threshold,
                        landmark_init_var=cfg.landmark_init_var, enable_measurement_model=cfg.enable_measurement_model,
                        enable_circular_interpolation=cfg.enable_circular_interpolation,
                        disable_motion_model=cfg.disable_motion_model)


def handle(sd, scripts, options=()):
    """A bank handle with the scripts' starts uploaded and both logs on."""
    f = sd.EkfSlam(NS, batch=len(scripts), config=sdcfg(sd, scripts[0].cfg))
    for name, value in options:
        f.set_option(name, value)
    f.profile_enable(True)
    for b, s in enumerate(scripts):
        f.set_state(s.mean0, s.cov0, b)
    f.log_innovations(K)
    f.log_poses(2 * K)
    return f


def collect(f, scripts, rows_per_step=1):
    """The handle's logs and final states as one geometry_model.Run per slot (`rows_per_step` = 2: predict and update each left a
    pose row; the update's is the step's, the prediction's is returned apart)."""
    inn, tr = f.innovations(), f.poses()
    measured = scripts[0].cfg.enable_measurement_model
    assert len(inn.steps) == K or (not measured and len(inn.steps) == 0), f"{len(inn.steps)} logged steps"
    assert tr.mean.shape[0] == rows_per_step * K, f"{tr.mean.shape[0]} pose rows"
    runs, predicted = [], []
    for b in range(len(scripts)):
        obs = []
        for k in range(K):
            m = int(inn.m[k, b]) if len(inn.steps) else 0
            obs.append([(int(inn.idx[k, b, i]), inn.y[k, b, i].copy(), inn.S[k, b, i].copy(), float(inn.nis[k, b, i]))
                        for i in range(m)])
            if len(inn.steps):
                assert (inn.rejected[k, b, :m] == 0).all()
        last = rows_per_step - 1
        poses = [(tr.mean[rows_per_step * k + last, b].copy(), tr.cov[rows_per_step * k + last, b].copy()) for k in range(K)]
        predicted.append([tr.mean[rows_per_step * k, b].copy() for k in range(K)])
        mu, P = f.state(b)
        runs.append(gm.Run(obs, poses, mu, P, f.flags(b)))
    return runs, predicted


def judge_bank(path, bank, scripts, runs, refs):
    worst = {k: 0.0 for k in gm.FIGURES}
    for run, ref in zip(runs, refs):                           # (every figure is printed before any is judged)
        w, _ = gm.distances(run, ref)
        worst = {k: max(worst[k], w[k]) for k in worst}
    print(f"geometry path={path} bank={bank} " + " ".join(f"{k}={v:.2e}" for k, v in worst.items()))
    for s, run, ref in zip(scripts, runs, refs):
        gm.judge(run, ref, BARS, what=f"{path}, {s.name}: ", symmetric=True)
    return worst


# ---- SLAM paths ------------------------------------------------------------------------------------------------------------------
def drive_steps(f, scripts):
    for k in range(K):
        f.step(*gc.step_args(scripts, k))


def drive_predict_update(f, scripts):
    for k in range(K):
        lin, ang, idx, zr, zb = gc.step_args(scripts, k)
        f.predict(lin, ang)
        f.update(idx, zr, zb)


def drive_stream(f, scripts):
    f.run_stream(*gc.stacked(scripts))


GENERAL = (("small_state", 0),)
PATHS = {
    # name: (options, driver, pose rows per step, check of the counters; `two`: the stream's updates fill a second cadence -- with
    # the measurement model off the planner has nothing to pack, and a single cadence has nothing to chain)
    "step_two_launches": (GENERAL + (("fused_step", 0),), drive_steps, 1,
                          lambda c, two: c.small_launches == 0 and c.cadences == 0),
    "step_one_launch": (GENERAL + (("fused_step", 1),), drive_steps, 1,
                        lambda c, two: c.small_launches == 0 and c.cadences == 0),
    "predict_update": (GENERAL, drive_predict_update, 2, lambda c, two: c.small_launches == 0 and c.cadences == 0),
    "stream_fused": (GENERAL + (("chain", 0),), drive_stream, 1,
                     lambda c, two: c.small_launches == 0 and c.cadences == 1 + two and c.covered == K and c.chained == 0),
    "stream_chained": (GENERAL, drive_stream, 1,
                       lambda c, two: c.small_launches == 0 and c.cadences == 1 + two and c.covered == K and (c.chained > 0) == two),
    "stream_per_step": (GENERAL + (("fused_cadence", 0),), drive_stream, 1,
                        lambda c, two: c.small_launches == 0 and c.cadences == 0 and c.chained == 0),
    "small_step": ((), drive_steps, 1, lambda c, two: c.small_launches > 0 and c.cadences == 0),
    "small_stream": ((), drive_stream, 1, lambda c, two: c.small_launches > 0 and c.cadences == 0),
}


@pytest.mark.parametrize("bank", gc.BANK_NAMES)
@pytest.mark.parametrize("path", list(PATHS))
def test_slam_paths(sd, path, bank):
    scripts = gc.bank(bank)
    options, drive, rows, ran = PATHS[path]
    refs = [reference(s) for s in scripts]
    with handle(sd, scripts, options) as f:
        drive(f, scripts)
        runs, predicted = collect(f, scripts, rows)
        c = counters(sd, f)
        assert ran(c, scripts[0].cfg.enable_measurement_model), (path, c)
        assert path_ran(f, "default_path" if path.startswith("small") else "general_kernels")
    judge_bank(path, bank, scripts, runs, refs)
    if rows == 2:                                              # the lone prediction's row: the model's pose behind its motion model
        for s, ref, rows_b in zip(scripts, refs, predicted):
            for k, rec in enumerate(ref.recs[:-1] if s.exact else ref.recs):
                e = float(np.max(np.abs(gm.ld(rows_b[k]) - rec.predicted)))
                assert e <= BARS["pose"], (s.name, k, e)


@pytest.mark.parametrize("bank", gc.BANK_NAMES)
def test_chained_stream_of_one_script_repeated(sd, bank):
    """The chained solves' shape in the benchmark: one stream in every slot.  The bank's first stream script and its last, 16 slots
    each: every slot the same bits, and those against the model."""
    stream = [s for s in gc.bank(bank) if s.updates > 40]
    two = stream[0].cfg.enable_measurement_model               # (measurement model off: one cadence, nothing to chain)
    for s in (stream[0], stream[-1]):
        copies = [s] * 16
        with handle(sd, copies, GENERAL) as f:
            drive_stream(f, copies)
            runs, _ = collect(f, copies)
            c = counters(sd, f)
            assert c.small_launches == 0 and c.cadences == 1 + two and c.covered == K and (c.chained > 0) == two, c
        for run in runs[1:]:
            assert np.array_equal(run.mean, runs[0].mean) and np.array_equal(run.cov, runs[0].cov)
            assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(run.poses, runs[0].poses))
        judge_bank("stream_chained_repeated", bank, [s], runs[:1], [reference(s)])


# ---- localisation ----------------------------------------------------------------------------------------------------------------
_LOC_REFS = {}


def drive_localize(f, scripts):
    for k in range(K):
        f.localize(*gc.step_args(scripts, k))


def drive_localize_update(f, scripts):
    for k in range(K):
        lin, ang, idx, zr, zb = gc.step_args(scripts, k)
        f.predict(lin, ang)
        f.localize_update(idx, zr, zb)


def drive_run_localize(f, scripts):
    f.stream_upload(*gc.stacked(scripts))
    f.run_localize(0, K)


LOCALIZE = {"localize": (drive_localize, 1), "localize_update": (drive_localize_update, 2), "run_localize": (drive_run_localize, 1)}


@pytest.mark.parametrize("bank", gc.BANK_NAMES)
@pytest.mark.parametrize("kernels", ["default_path", "general_kernels"])
@pytest.mark.parametrize("path", list(LOCALIZE))
def test_localisation_paths(sd, path, kernels, bank):
    scripts = gc.bank(bank)
    drive, rows = LOCALIZE[path]
    for s in scripts:
        if s.name not in _LOC_REFS:
            _LOC_REFS[s.name] = gm.localize_reference(s)
    refs = [_LOC_REFS[s.name] for s in scripts]
    with handle(sd, scripts, (("profile_kernels", 1),) + (GENERAL if kernels == "general_kernels" else ())) as f:
        before = counters(sd, f)
        drive(f, scripts)
        runs, _ = collect(f, scripts, rows)
        c = counters(sd, f)
        assert c.cadences == 0 and c.passes == before.passes, c        # no rank, never a covariance pass
        assert f.profile_read_class(9)[1] > 0                           # the localisation solve was launched
        # (localisation has one solve kernel; the setting shows in the prediction that localize_update follows)
        assert c.small_launches == 0 if kernels == "general_kernels" else (c.small_launches > 0 or path != "localize_update"), c
    judge_bank(f"{path}[{kernels}]", bank, scripts, runs, refs)


# ---- association scores ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bank", [b for b in gc.BANK_NAMES if b != "no_measurement"])
def test_association_scores_at_the_last_state(sd, bank):
    """associate(full=True) behind the script's steps, the last step's ranks still pending: geometry_cases.association_observations
    (the last step's measurements, moved a little) against every landmark.  The model scores the state the device itself returns
    afterwards (associate changes nothing), so the bars are on the association kernel alone: every pair's NIS relatively, ln det S
    over max(1, |ln det S|), and the two best candidates of every observation (tests/test_geometry_cpu.py holds their separation).
    The exact-boundary scripts are not scored: their state hangs on which side of +-pi the one residual landed."""
    scripts = gc.bank(bank)
    asked = [gc.association_observations(s) for s in scripts]
    zr, zb = [a[0] for a in asked], [a[1] for a in asked]
    with handle(sd, scripts, GENERAL + (("fused_step", 1),)) as f:
        drive_steps(f, scripts)
        before = counters(sd, f)
        a = f.associate(zr, zb, full=True)
        assert counters(sd, f) == before and before.small_launches == 0
        states = [f.state(b) for b in range(len(scripts))]
    bar = gc.ASSOCIATE_BARS["nis"]
    worst, checks = dict(nis=0.0, logdet=0.0), []
    for b, s in enumerate(scripts):
        if s.exact:
            continue
        nis, logdet, res = gm.associate_scores(states[b][0], states[b][1], zr[b], zb[b], s.cfg)
        S = len(zr[b])
        got_nis, got_ld = a.all_nis[b, :S, :gc.N], a.all_logdet[b, :S, :gc.N]
        e_nis = float(np.max(np.abs(got_nis - nis) / nis))
        e_ld = float(np.max(np.abs(got_ld - logdet[None, :]) / np.maximum(1.0, np.abs(logdet[None, :]))))
        worst = dict(nis=max(worst["nis"], e_nis), logdet=max(worst["logdet"], e_ld))
        checks.append((b, s, nis, logdet, res, e_nis, e_ld))
    print(f"geometry path=associate bank={bank} " + " ".join(f"{k}={v:.2e}" for k, v in worst.items()))
    for b, s, nis, logdet, res, e_nis, e_ld in checks:
        assert (np.abs(res.astype(float)) <= np.pi - 1e-6).all(), s.name
        assert e_nis <= bar and e_ld <= gc.ASSOCIATE_BARS["logdet"], (s.name, e_nis, e_ld)
        d = (nis + logdet[None, :]).astype(float)
        for q in range(len(zr[b])):
            order = np.argsort(d[q])
            assert list(a.cand[b, q]) == list(order[:2]), (s.name, q, a.cand[b, q], order[:3])
            assert np.allclose(a.nis[b, q], nis[q][order[:2]].astype(float), rtol=bar, atol=0)
            assert abs(a.min_nis[b, q] - float(nis[q].min())) <= bar * float(nis[q].min())


# ---- detections ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernels", ["default_path", "general_kernels"])
def test_step_detections(sd, kernels):
    """Windows whose tags lie ahead, abeam and behind the robot (pose_t z < 0, off the axis), inside the gate: the device's own
    range and bearing through tags_positions() and through the logged y; S, NIS, the pose rows and the final state as on every path."""
    wins = gc.detection_windows()
    refs = gc.detection_reference()
    B = len(refs)
    with sd.EkfSlam(3 + 2 * 10, batch=B) as f:
        if kernels == "general_kernels":
            f.set_option("small_state", 0)
        f.log_innovations(len(wins))
        f.log_poses(len(wins))
        worst_tags = 0.0
        for k, (lin, ang, per_traj) in enumerate(wins):
            f.step_detections(np.full(B, lin), np.full(B, ang), [gc.tag_objects(w) for w in per_traj])
            for b in range(B):
                got, want = f.tags_positions(b), refs[b].tags[k]
                assert list(got.keys()) == list(want.keys()), (k, b)
                for j in want:
                    assert got[j][3] == want[j][3]
                    e = max(abs(got[j][i] - want[j][i]) for i in (0, 1, 4, 5))      # world guess, range, bearing
                    worst_tags = max(worst_tags, float(e))
        assert f.assoc_fallbacks() == 0 and path_ran(f, kernels)
        inn, tr = f.innovations(), f.poses()
        runs = []
        for b in range(B):
            obs = [[(int(inn.idx[k, b, i]), inn.y[k, b, i].copy(), inn.S[k, b, i].copy(), float(inn.nis[k, b, i]))
                    for i in range(int(inn.m[k, b]))] for k in range(len(wins))]
            poses = [(tr.mean[k, b].copy(), tr.cov[k, b].copy()) for k in range(len(wins))]
            mu, P = f.state(b)
            runs.append(gm.Run(obs, poses, mu, P, f.flags(b)))
    assert worst_tags <= gc.TAGS_BAR, worst_tags
    worst = {k: 0.0 for k in gm.FIGURES}
    for b, (run, ref) in enumerate(zip(runs, refs)):
        w = gm.judge(run, gm.Reference(ref.mean, ref.cov, ref.recs, False, 1e4), BARS, what=f"detections, trajectory {b}: ",
                     symmetric=True)
        worst = {k: max(worst[k], w[k]) for k in worst}
    print(f"geometry path=step_detections[{kernels}] bank=detections tags={worst_tags:.2e} " +
          " ".join(f"{k}={v:.2e}" for k, v in worst.items()))
