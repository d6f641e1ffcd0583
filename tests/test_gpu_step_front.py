"""GPU: what the step entries share on the host -- the planners of ekf_host_plan.h, the input ring (res::InputRing) and the
log rows (LogScope) -- seen from outside: ekf_step, ekf_localize_step, ekf_step_detections, ekf_localize_detections and
ekf_predict_linear.

Shapes: n_max = 43 (the small-state path: the kernels read their records from the pinned ring itself) and n_max = 263 (the
general kernels: the records are staged to the device), batch 1 and a bank of 3 with uneven sizes.  2 x RING + 1 consecutive
calls take every slot of the ring three times at least.  (Which path a handle takes follows from n_max alone; where SLAM
steps run it is asserted through the small-state launch counter, which the localisation and prediction kernels do not move.)  Each entry is judged by the model and at the tolerance its own suite
uses: the dense oracle / tests/localize_model.py / tests/loc_det_world.py through parity_blocks.assert_state_close at the block
bar of 1e-9, tests/motion_model.py at 1e-9 relative Frobenius (tests/test_gpu_predict_linear.py)."""
import ctypes as C

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests import loc_det_world as ldw
from tests import localize_model as lm
from tests import motion_model as mm
from tests import streams
from tests.conftest import path_ran
from tests.gpu_support import counters, same, sd  # noqa: F401
from tests.parity_blocks import assert_state_close, fmt_state

pytestmark = pytest.mark.gpu

TOL = 1e-9
INIT_VAR = 1e4
CFG = orc.EkfConfig()
RING = 16                                                  # (csrc/ekf_api.hip)
CALLS = 2 * RING + 1
EKF_ERR_ARG = -1
EKF_DMAX = 256
LIN, ANG = ldw.LIN, ldw.ANG
SHAPES = [(43, 1), (43, 3), (263, 1), (263, 3)]            # (n_max, batch)
dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


def sizes_of(n_max, B):
    return (n_max,) if B == 1 else (n_max, n_max - 16, 13)


def check(f, b, model, what):
    got = (*f.state(b), f.tag_index(b), f.flags(b))
    err = assert_state_close(got, (model[0], model[1], f.tag_index(b)), INIT_VAR, tol=TOL, entry_tol=TOL, what=what + ": ")
    print(f"{what}: {fmt_state(err)}")


def per_traj(B, values):
    """What a call takes for a bank of B: the value itself for one trajectory, else one per trajectory."""
    return values[0] if B == 1 else list(values)


def observe(mean, lms, rng, noise=0.01):
    """Ranges and bearings of the landmarks `lms` as the mean itself sees them, plus a little noise."""
    lms = np.asarray(lms, dtype=np.int64)
    d = np.asarray(mean)[3:].reshape(-1, 2)[lms] - np.asarray(mean)[:2]
    zr = np.hypot(d[:, 0], d[:, 1]) + rng.normal(0.0, noise, len(lms))
    zb = orc.wrap_pi(np.arctan2(d[:, 1], d[:, 0]) - mean[2] + rng.normal(0.0, noise, len(lms)))
    return lms.astype(np.int32), zr, zb


def logged(sd, f):
    """(ekf_innovation_steps, ekf_pose_steps)"""
    n = C.c_longlong(0)
    assert sd.load_library().ekf_innovation_steps(f._h, C.byref(n)) == 0
    return n.value, f.pose_steps


def dense_bank(sd, n_max, B, seed):
    """A handle whose trajectories (sizes_of) hold dense covariances: every landmark correlated with the pose."""
    f = sd.EkfSlam(n_max, batch=B)
    for b, n in enumerate(sizes_of(n_max, B)):
        f.set_state(orc.synthetic_world((n - 3) // 2, seed + b)[2], streams.dense_start(n, seed + 10 + b), b)
    return f


# ---- the ring wraps on every entry ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_max,B", SHAPES)
def test_ring_wrap_step(sd, n_max, B):
    sizes = sizes_of(n_max, B)
    ss = [orc.synthetic_stream((n - 3) // 2, CALLS, (8, 5, 3)[b], 40 + b) for b, n in enumerate(sizes)]
    with sd.EkfSlam(n_max, batch=B) as f:
        for b, s in enumerate(ss):
            f.set_state_diag(s[0], s[1], b)
        for k in range(CALLS):
            f.step(*(per_traj(B, [s[i][k] for s in ss]) for i in (2, 3, 4, 5, 6)))
        f.flush()
        for b, s in enumerate(ss):
            om, oP = s[0].copy(), np.diag(s[1])
            for k in range(CALLS):
                om, oP = orc.ekf_step_dense(om, oP, s[2][k], s[3][k], s[4][k], s[5][k], s[6][k], CFG)
            check(f, b, (om, oP), f"{CALLS} steps, n_max {n_max}, trajectory {b} of {B}")
        assert path_ran(f, "default_path")


@pytest.mark.parametrize("n_max,B", SHAPES)
def test_ring_wrap_localize(sd, n_max, B):
    rng = np.random.default_rng(n_max + B)
    with dense_bank(sd, n_max, B, 3) as f:
        model = [f.state(b) for b in range(B)]
        for k in range(CALLS):
            obs = [observe(model[b][0], (3 * k + b + np.arange((4, 0, 2)[b] + k % 3)) % ((len(model[b][0]) - 3) // 2), rng) for b in range(B)]
            w = 0.005 if k % 7 == 6 else 0.02
            f.localize(0.004, w, *(per_traj(B, [o[i] for o in obs]) for i in range(3)))
            model = [lm.literal_step(*model[b], 0.004, w, *obs[b], CFG) for b in range(B)]
        for b in range(B):
            check(f, b, model[b], f"{CALLS} localize calls, n_max {n_max}, trajectory {b} of {B}")


def detection_worlds(B):
    return [ldw.World((6, 4, 3)[b], 5 + b) for b in range(B)]


@pytest.mark.parametrize("n_max,B", SHAPES)
def test_ring_wrap_step_detections(sd, n_max, B):
    worlds = detection_worlds(B)
    model = [(np.zeros(3), np.eye(3) * CFG.motion_sigma, {}) for _ in range(B)]
    with sd.EkfSlam(n_max, batch=B) as f:
        for k in range(CALLS):
            wins = []
            for b, w in enumerate(worlds):
                w.move()
                wins.append(w.window([(k + i) % w.N for i in range(1 + (k + b) % min(3, w.N))], 1 + k % 2))
                mean, cov, index = model[b]
                mean, cov, _ = orc.ekf_pose_estimation_dense(ANG, LIN, mean, cov, 0.7, wins[b], index, CFG)
                model[b] = (mean, cov, index)
            f.step_detections(LIN, ANG, per_traj(B, wins))
        f.flush()
        assert f.assoc_fallbacks() == 0
        for b in range(B):
            assert f.tag_index(b) == model[b][2]
            check(f, b, model[b], f"{CALLS} windows of step_detections, n_max {n_max}, trajectory {b} of {B}")
        assert path_ran(f, "default_path")


@pytest.mark.parametrize("n_max,B", SHAPES)
def test_ring_wrap_localize_detections(sd, n_max, B):
    worlds = detection_worlds(B)
    with sd.EkfSlam(n_max, batch=B) as f:
        maps = [ldw.mapping_windows(w) for w in worlds]
        for k in range(4):
            f.step_detections(LIN, ANG, per_traj(B, [m[k] for m in maps]))
        f.flush()
        model, index = [f.state(b) for b in range(B)], [f.tag_index(b) for b in range(B)]
        assert [len(x[0]) for x in model] == [3 + 2 * w.N for w in worlds]
        for k in range(CALLS):
            wins = []
            for b, w in enumerate(worlds):
                w.move()
                wins.append(w.window([(2 * k + i) % w.N for i in range(1 + (k + b) % w.N)], 1 + k % 3))
                model[b], _, unmatched = ldw.model_window(*model[b], index[b], wins[b])
                assert unmatched == []
            f.localize_detections(LIN, ANG, per_traj(B, wins))
        assert f.assoc_fallbacks() == 0
        for b in range(B):
            assert f.tag_index(b) == index[b]
            check(f, b, model[b], f"{CALLS} windows of localize_detections, n_max {n_max}, trajectory {b} of {B}")
        assert path_ran(f, "default_path")


@pytest.mark.parametrize("n_max,B", SHAPES)
def test_ring_wrap_predict_linear(sd, n_max, B):
    rng = np.random.default_rng(7 * n_max + B)
    with dense_bank(sd, n_max, B, 9) as f:
        for k in range(CALLS):
            b = k % B
            before = f.state(b)
            pose, F, Q = mm.draw(rng, *before, kind=mm.KINDS[k % 3])
            f.predict_linear(pose, F, Q, b=b)
            wm, wP = mm.predict_linear(before[0], before[1], pose, F, Q)
            mu, P = f.state(b)
            e = orc.rel_fro(mu, wm), orc.rel_fro(P, wP), orc.rel_fro(P[:3], wP[:3])
            assert max(e) <= TOL, (k, b, e)
            assert np.array_equal(mu[3:], before[0][3:]) and np.array_equal(P[3:, 3:], before[1][3:, 3:])


# ---- a call of several update passes is one logged step ------------------------------------------------------------------------
@pytest.mark.parametrize("n_max", [43, 263])
def test_localize_in_two_and_three_passes_is_one_logged_step(sd, n_max):
    """17 and 33 observations of trajectory 0 (two and three update passes: log entries from position 0, 16 and 32 on), 3 and
    none on the others: one innovation-log step, one pose row, both counters advanced by one.  (ekf_step / ekf_update:
    tests/test_gpu_innovations.py and tests/test_gpu_pose_trace.py, test_update_with_more_than_sixteen_and_thirty_two_landmarks.)"""
    rng = np.random.default_rng(n_max)
    AMAX = 32
    with dense_bank(sd, n_max, 3, 17) as f:
        f.log_innovations(4)
        f.log_poses(4)
        model = [f.state(b) for b in range(3)]
        for k, m0 in enumerate((17, 33)):
            nl = [(len(x[0]) - 3) // 2 for x in model]
            obs = [observe(model[0][0], (5 * k + np.arange(m0)) % nl[0], rng), observe(model[1][0], [2, 1, 2], rng), observe(model[2][0], [], rng)]
            logs = [[] for _ in range(3)]
            f.localize(0.004, 0.02, [o[0] for o in obs], [o[1] for o in obs], [o[2] for o in obs])
            model = [lm.literal_step(*model[b], 0.004, 0.02, *obs[b], CFG, log=logs[b]) for b in range(3)]
            assert logged(sd, f) == (k + 1, k + 1)
            inn, tr = f.innovations(k, 1), f.poses(k, 1)
            assert [int(x) for x in inn.m[0]] == [m0, 3, 0] and inn.idx.shape[2] == min(m0, AMAX)
            worst = 0.0
            for b in range(3):
                kept = min(len(logs[b]), AMAX)
                assert [int(i) for i in inn.idx[0, b, :kept]] == [int(l[0]) for l in logs[b][:kept]]
                for j, (_l, y, S, nis, _rej) in enumerate(logs[b][:kept]):
                    worst = max(worst, float(np.abs(inn.y[0, b, j] - y).max()) / max(1e-3, float(np.abs(y).max())), lm.rel(inn.S[0, b, j], S),
                                abs(inn.nis[0, b, j] - nis) / max(nis, 1e-6))
                worst = max(worst, lm.rel(tr.mean[0, b], model[b][0][:3]), lm.rel(tr.cov[0, b], model[b][1][:3, :3]))
            print(f"m = {m0}: worst relative deviation of y, S, NIS and the pose row from the model {worst:.2e}")
            assert worst <= TOL
        for b in range(3):
            check(f, b, model[b], f"localize in passes, n_max {n_max}, trajectory {b}")


# ---- refused calls -----------------------------------------------------------------------------------------------------------------
def everything(sd, f):
    """What a refused call must leave as a run without it leaves it: states, tag tables, both logs, both counters, the cadences."""
    B = f.batch
    inn, tr, c = f.innovations(), f.poses(), counters(sd, f)
    return dict(mean=[f.state(b)[0] for b in range(B)], cov=[f.state(b)[1] for b in range(B)], tags=[f.tag_index(b) for b in range(B)],
                flags=[f.flags(b) for b in range(B)], inn=[inn.steps, inn.m, inn.idx, inn.y, inn.S, inn.nis], poses=[tr.first, tr.mean, tr.cov],
                steps=logged(sd, f), cadences=(c.cadences, c.covered))


def same_everything(a, b):
    for key in a:
        if key in ("tags", "flags", "steps", "cadences"):
            assert a[key] == b[key], key
        else:
            for x, y in zip(a[key], b[key]):
                assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=np.asarray(x).dtype.kind == "f"), key


def test_refused_window_leaves_no_trace(sd):
    """n_max = 263, a bank of 3: 2 x RING windows of ekf_step_detections, run as they are and with two refused calls among them
    -- a count above EKF_DMAX in front of the first window, a NULL tag_id with a positive count in front of window RING / 2,
    where a ring group starts -- through the library itself (EkfSlam.step_detections keeps such windows from the device entry).
    EKF_ERR_ARG both times, and every bit of what the two runs leave is the same."""
    lib = sd.load_library()
    B, K = 3, 2 * RING

    def windows():
        worlds = detection_worlds(B)
        out = []
        for k in range(K):
            for w in worlds:
                w.move()
            out.append([w.window([(k + i) % w.N for i in range(1 + (k + b) % min(3, w.N))], 1 + k % 2) for b, w in enumerate(worlds)])
        return out

    def refuse(f, which):
        lin, ang = np.full(B, LIN), np.full(B, ANG)
        if which == "count":
            count, stride = np.array([EKF_DMAX + 1, 0, 0], dtype=np.int32), EKF_DMAX + 1
        else:
            count, stride = np.array([0, 2, 0], dtype=np.int32), 4
        ids, pt, pe = np.zeros((B, stride), dtype=np.int32), np.full((B, stride, 3), 0.5), np.zeros((B, stride))
        rc = lib.ekf_step_detections(f._h, lin.ctypes.data_as(dp), ang.ctypes.data_as(dp), count.ctypes.data_as(ip),
                                     ids.ctypes.data_as(ip) if which == "count" else None, pt.ctypes.data_as(dp), pe.ctypes.data_as(dp), stride)
        assert rc == EKF_ERR_ARG, (which, rc)

    def run(refused):
        with sd.EkfSlam(263, batch=B) as f:
            f.log_innovations(K + 8)
            f.log_poses(K + 8)
            for k, wins in enumerate(windows()):
                if refused and k == 0:
                    refuse(f, "count")
                if refused and k == RING // 2:
                    refuse(f, "null")
                f.step_detections(LIN, ANG, wins)
            assert f.assoc_fallbacks() == 0 and logged(sd, f) == (K, K)
            assert path_ran(f, "default_path")
            return everything(sd, f)

    same_everything(run(False), run(True))


def test_failed_localize_does_not_advance_the_logs(sd):
    """n_max = 43: a localize call naming a landmark outside the map between two valid logged ones.  Both counters say two, and
    the rows are those of a handle that ran the two valid calls alone."""
    rng = np.random.default_rng(4)
    with dense_bank(sd, 43, 1, 31) as f, dense_bank(sd, 43, 1, 31) as twin:
        for h in (f, twin):
            h.log_innovations(4)
            h.log_poses(4)
        first, second = observe(f.state(0)[0], [3, 7, 3, 11], rng), observe(f.state(0)[0], [0, 19], rng)
        f.localize(0.004, 0.02, *first)
        with pytest.raises(sd.EkfError):
            f.localize(0.004, 0.02, [3, 20], [1.0, 1.0], [0.1, 0.2])           # landmarks 0..19 exist
        f.localize(0.004, 0.005, *second)
        twin.localize(0.004, 0.02, *first)
        twin.localize(0.004, 0.005, *second)
        assert logged(sd, f) == (2, 2)
        same_everything(everything(sd, f), everything(sd, twin))
        assert [int(x) for x in f.innovations().m[:, 0]] == [4, 2]
