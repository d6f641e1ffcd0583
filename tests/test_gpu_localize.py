"""GPU: localisation on a frozen map (ekf_localize_step / _update / _run; EkfSlam.localize / localize_update / run_localize)
against the dense model tests/localize_model.py fed the same calls from state() taken just before them.

Comparisons go through parity_blocks.assert_state_close at the project's block bar of 1e-9 (pose block, cross rows, landmark
block, correlation-scaled maximum, means, each on its own scale; tests/test_localize_cpu.py shows the model's two forms agree to
4e-16, so 1e-9 is a statement about the device code), plus bit comparisons: what the call must leave alone -- every row >= 3
of the stored P_base and every landmark mean -- is read raw (pbase) before and after.  Small cases run on the small-state path
and on the general kernels (both_paths), with the path asserted."""
import ctypes as C

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests import localize_model as lm
from tests import sequence_cases as sc
from tests import streams
from tests.conftest import path_ran
from tests.gpu_support import bank, counters, pbase, same, sd  # noqa: F401
from tests.parity_blocks import assert_state_close, fmt_state

pytestmark = pytest.mark.gpu

TOL = 1e-9
INIT_VAR = 1e4
CFG = orc.EkfConfig()
SLAM_STEPS = 30


def wrap(a):
    return (a + np.pi) % (2 * np.pi) - np.pi


def observe(mean, lms, rng, noise=0.01):
    """Ranges and bearings of the landmarks `lms` as the mean itself sees them, plus a little noise."""
    lms = np.asarray(lms, dtype=np.int64)
    d = np.asarray(mean)[3:].reshape(-1, 2)[lms] - np.asarray(mean)[:2]
    zr = np.hypot(d[:, 0], d[:, 1]) + rng.normal(0.0, noise, len(lms))
    zb = wrap(np.arctan2(d[:, 1], d[:, 0]) - mean[2] + rng.normal(0.0, noise, len(lms)))
    return lms.astype(np.int32), zr, zb


def small_streams(B, steps=SLAM_STEPS + 12, m=8):
    return [orc.synthetic_stream(20, steps, m, tid) for tid in range(B)]


def frozen_part(sd, f, b):
    """What a localisation call must leave alone, raw: every stored P(a, b) with a, b >= 3 -- also below the diagonal and in the
    padding --, and the landmark means."""
    raw = pbase(sd, f, b)
    n_max = f.n_max
    if n_max <= 4096:
        ld = 64
        while ld < n_max:
            ld *= 2
        rows = raw.reshape(-1, ld)[3:].copy()
        rows[:, :3] = 0.0                                  # (columns 0..2 below the diagonal: a download's mirror of rows 0..2)
    else:
        ld = (n_max + 63) // 64 * 64
        rows = raw.reshape(-1, ld, 4096)[:, 3:].copy()
        rows[0, :, :3] = 0.0
    return rows, f.state(b)[0][3:].copy()


def frozen_same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def got_state(f, b):
    return (*f.state(b), f.tag_index(b), f.flags(b))


def check(f, b, model, what, entry_tol=TOL):
    err = assert_state_close(got_state(f, b), (model[0], model[1], f.tag_index(b)), INIT_VAR, tol=TOL, entry_tol=entry_tol,
                             what=what + ": ")
    print(f"{what}: {fmt_state(err)}")
    return err


def scheduling(sd, f):
    c = counters(sd, f)
    return c.passes, c.cadences, c.covered, c.chained, c.lookaheads


# ---- 1: a bank with m = (0, 3, 8), one trajectory naming a landmark twice ------------------------------------------------------
def test_basic_bank(sd, both_paths):
    B, N, K = 3, 20, 6
    _, lin, ang, idx, zr, zb, m = streams.wandering(N, B, SLAM_STEPS, 8, 11)
    worlds = [orc.synthetic_world(N, 11 + 1 + t) for t in range(B)]
    rng = np.random.default_rng(5)
    with sd.EkfSlam(3 + 2 * N, batch=B) as f:
        for b in range(B):
            f.set_state_diag(worlds[b][2], worlds[b][3], b)
        f.stream_upload(lin, ang, idx, zr, zb, m)
        f.stream_run(0, SLAM_STEPS)                        # dense cross-covariances
        f.flush()
        f.profile_enable(True)
        model = [f.state(b) for b in range(B)]
        frozen = [frozen_part(sd, f, b) for b in range(B)]
        sched = scheduling(sd, f)
        for k in range(K):
            obs = [observe(model[0][0], [], rng),
                   observe(model[1][0], [(3 * k) % N, (3 * k + 7) % N, (3 * k) % N], rng),       # landmark 3k twice
                   observe(model[2][0], (5 * k + np.arange(8)) % N, rng)]
            f.localize(0.004, 0.02 if k % 3 else 0.005, [o[0] for o in obs], [o[1] for o in obs], [o[2] for o in obs])
            for b in range(B):
                model[b] = lm.literal_step(*model[b], 0.004, 0.02 if k % 3 else 0.005, *obs[b], CFG)
        for b in range(B):
            check(f, b, model[b], f"basic bank, trajectory {b} (m = {(0, 3, 8)[b]})")
            assert frozen_same(frozen_part(sd, f, b), frozen[b]), f"trajectory {b}: the map moved"
        assert scheduling(sd, f) == sched                  # no covariance pass, no cadence
        assert path_ran(f, both_paths)


# ---- 2: state indices 255..258 straddle the row kernel's workgroup boundary ----------------------------------------------------
@pytest.mark.parametrize("m", [16, 20])
def test_workgroup_boundary(sd, m):
    N = 150
    s = orc.synthetic_stream(N, SLAM_STEPS, 8, 3)
    rng = np.random.default_rng(m)
    with bank(sd, [s], steps=SLAM_STEPS, options=[("small_state", 0)]) as f:
        f.flush()
        model = f.state(0)
        frozen = frozen_part(sd, f, 0)
        lms = [0, 126, 127, 149] + [int(x) for x in rng.choice(np.setdiff1d(np.arange(N), [0, 126, 127, 149]), m - 4, replace=False)]
        for k in range(2):
            obs = observe(model[0], lms, rng)
            f.localize(0.004, 0.02, *obs)
            model = lm.literal_step(*model, 0.004, 0.02, *obs, CFG)
        check(f, 0, model, f"N = 150, m = {m}")
        assert frozen_same(frozen_part(sd, f, 0), frozen)
        assert path_ran(f, "general_kernels")


# ---- 3: the column-panel layout (ld > 4096) ------------------------------------------------------------------------------------
def test_column_panel_layout(sd):
    N = 2100
    n = 3 + 2 * N
    rng = np.random.default_rng(9)
    mean = orc.synthetic_world(N, 2)[2].copy()
    cov = streams.dense_start(n, 4)
    with sd.EkfSlam(n, batch=1) as f:
        f.set_state(mean, cov)
        model = f.state(0)
        frozen = frozen_part(sd, f, 0)
        for k in range(2):
            obs = observe(model[0], [10, 2046, 2099], rng)       # t = 4095, 4096 straddles the panel
            f.localize(0.004, 0.02, *obs)
            model = lm.rows_step(*model, 0.004, 0.02, *obs, CFG)
        check(f, 0, model, "N = 2100 (column panels)")
        assert frozen_same(frozen_part(sd, f, 0), frozen)


# ---- 4: ranks pending at entry -------------------------------------------------------------------------------------------------
def test_ranks_pending_at_entry(sd):
    N = 150
    s = orc.synthetic_stream(N, 12, 8, 1)
    rng = np.random.default_rng(2)
    with sd.EkfSlam(3 + 2 * N, batch=1) as f:
        f.set_option("small_state", 0)
        f.set_state_diag(s[0], s[1])
        f.profile_enable(True)
        om, oP = s[0].copy(), np.diag(s[1])
        for k in range(3):
            f.step(s[2][k], s[3][k], s[4][k], s[5][k], s[6][k])
            om, oP = orc.ekf_step_dense(om, oP, s[2][k], s[3][k], s[4][k], s[5][k], s[6][k], CFG)
        p0 = f.profile_passes()                            # 48 ranks pending, no pass yet
        model = (om, 0.5 * (oP + oP.T))
        passes = []
        for k in range(6):
            obs = observe(model[0], (4 * k + np.arange(5)) % 24, rng)
            f.localize(0.004, 0.02, *obs)
            passes.append(f.profile_passes() - p0)
            model = lm.literal_step(*model, 0.004, 0.02, *obs, CFG)
        assert passes == [1] * 6, passes                   # exactly one pass, at entry of the first call
        check(f, 0, model, "three SLAM steps pending, then six localisation steps")


# ---- 5: the active bound -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("active_bound", [1, 0])
def test_active_bound_rises(sd, both_paths, active_bound):
    N = 20
    mean0, diag0 = orc.synthetic_world(N, 4)[2:4]
    s = orc.synthetic_stream(8, 4, 4, 4)                   # the first 8 landmarks only: the bound stays at 19
    mean0 = mean0.copy()
    mean0[3:19] = s[0][3:19]
    rng = np.random.default_rng(3)
    with sd.EkfSlam(3 + 2 * N, batch=1) as f:
        f.set_option("active_bound", active_bound)
        f.set_state_diag(mean0, diag0)
        for k in range(4):
            f.step(s[2][k], s[3][k], s[4][k], s[5][k], s[6][k])
        f.flush()
        model = f.state(0)
        assert not model[1][:3, 19:].any()
        obs = observe(model[0], [2, 15], rng)              # landmark 15: added, never observed
        f.localize(0.004, 0.02, *obs)
        model = lm.literal_step(*model, 0.004, 0.02, *obs, CFG)
        check(f, 0, model, f"active_bound = {active_bound}: a never-observed landmark")
        assert f.state(0)[1][:3, 33:35].any()              # the bound has risen over landmark 15: its columns were written
        # two SLAM steps behind it: a stale mirror of the bound would leave landmark 15's correlations out of their pass
        for lms in ([15, 3], [9, 15, 1]):
            obs = observe(model[0], lms, rng)
            f.step(0.004, 0.02, *obs)
            model = orc.ekf_step_dense(*model, 0.004, 0.02, *obs, CFG)
        f.flush()
        check(f, 0, model, f"active_bound = {active_bound}: two SLAM steps behind it")
        assert path_ran(f, both_paths)


def forked_pair(sd, streams_, both_paths=None):
    """Two bit-identical trajectories with dense cross-covariances: 30 SLAM steps, then slot 1 forked from slot 0."""
    f = bank(sd, streams_, steps=SLAM_STEPS)
    f.flush()
    f.fork(0, [1])
    return f


# ---- 6: the NIS gate -----------------------------------------------------------------------------------------------------------
def test_nis_gate_rejection_is_the_call_without_it(sd, both_paths):
    rng = np.random.default_rng(6)
    with forked_pair(sd, small_streams(2)) as f:
        start = f.state(0)
        assert same(start, f.state(1))
        idx, zr, zb = observe(start[0], [4, 9, 13], rng)
        zb[1] = wrap(zb[1] + 1.0)                          # a bearing off by 1 rad
        log = []
        lm.literal_step(*start, 0.004, 0.02, idx, zr, zb, CFG, log=log)
        bad = log[1][3]
        gate = 0.5 * bad                                   # below the outlier's NIS, above everything else's
        log = []
        lm.literal_step(*start, 0.004, 0.02, idx, zr, zb, CFG, gate=gate, log=log)
        assert [r[4] for r in log] == [False, True, False] and max(log[0][3], log[2][3]) < 0.5 * gate, [r[3] for r in log]
        f.set_nis_gate(gate)
        f.log_innovations(4)
        keep = [0, 2]
        f.localize(0.004, 0.02, [idx, idx[keep]], [zr, zr[keep]], [zb, zb[keep]])
        assert list(f.gate_counts()) == [1, 0]
        inn = f.innovations()
        assert list(inn.m[0]) == [3, 2] and list(inn.rejected[0, 0, :3]) == [0, 1, 0] and list(inn.rejected[0, 1, :2]) == [0, 0]
        assert abs(inn.nis[0, 0, 1] - bad) <= 1e-9 * bad
        # the header's promise: bit-identical to the call without the rejected observation; the others are applied
        assert same(f.state(0), f.state(1))
        model = lm.literal_step(*start, 0.004, 0.02, idx, zr, zb, CFG, gate=gate)
        check(f, 0, model, "gated step")
        assert lm.rel(f.state(0)[0][:3], start[0][:3]) > 1e-6
        assert path_ran(f, both_paths)


# ---- 7: the noise bank ---------------------------------------------------------------------------------------------------------
def test_noise_bank(sd, both_paths):
    rng = np.random.default_rng(7)
    motion, meas = [0.1, 0.05], [0.7, 0.3]
    with forked_pair(sd, small_streams(2)) as f:
        f.set_noise(motion_sigma=motion, meas_sigma=meas)
        model = [f.state(b) for b in range(2)]
        for k in range(3):
            obs = observe(model[0][0], (3 * k + np.arange(4)) % 20, rng)
            f.localize(0.004, 0.02, [obs[0]] * 2, [obs[1]] * 2, [obs[2]] * 2)
            for b in range(2):
                model[b] = lm.literal_step(*model[b], 0.004, 0.02, *obs, lm.with_noise(CFG, motion[b], meas[b]))
        for b in range(2):
            check(f, b, model[b], f"noise row {b} (motion {motion[b]}, meas {meas[b]})")
        assert lm.rel(model[1][1][:3, :3], model[0][1][:3, :3]) > 1e-3
        assert path_ran(f, both_paths)


# ---- 8: the logs ---------------------------------------------------------------------------------------------------------------
def test_logs(sd, both_paths):
    rng = np.random.default_rng(8)
    with bank(sd, small_streams(1), steps=SLAM_STEPS) as f, bank(sd, small_streams(1), steps=SLAM_STEPS) as twin:
        f.flush()
        f.log_innovations(8)
        f.log_poses(8)
        model = f.state(0)
        logs, poses = [], []
        for k in range(3):
            obs = observe(model[0], (2 * k + np.arange(3 + k)) % 20, rng)
            log = []
            f.localize(0.004, 0.02, *obs)
            model = lm.literal_step(*model, 0.004, 0.02, *obs, CFG, log=log)
            logs.append(log)
            poses.append((model[0][:3].copy(), model[1][:3, :3].copy()))
        obs = observe(model[0], [5, 6], rng)
        log = []
        f.localize_update(*obs)                            # no prediction
        model = lm.literal_step(*model, 0.0, 0.0, *obs, CFG, predict=False, log=log)
        logs.append(log)
        poses.append((model[0][:3].copy(), model[1][:3, :3].copy()))
        inn, tr = f.innovations(), f.poses()
        assert len(inn.steps) == 4 and tr.mean.shape[0] == 4 and [int(x) for x in inn.m[:, 0]] == [3, 4, 5, 2]
        worst = 0.0
        for k, log in enumerate(logs):
            for j, (l, y, S, nis, rej) in enumerate(log):
                assert inn.idx[k, 0, j] == l and inn.rejected[k, 0, j] == 0
                e = max(float(np.abs(inn.y[k, 0, j] - y).max()) / max(1e-3, float(np.abs(y).max())), lm.rel(inn.S[k, 0, j], S),
                        abs(inn.nis[k, 0, j] - nis) / max(nis, 1e-6))
                worst = max(worst, e)
            worst = max(worst, lm.rel(tr.mean[k, 0], poses[k][0]), lm.rel(tr.cov[k, 0], poses[k][1]))
        print(f"logs: worst relative deviation of y, S, NIS, pose rows from the model {worst:.2e}")
        assert worst <= TOL                                # (y: absolute error a few eps of an O(1) angle, over max(|y|, 1e-3): ~1e-12)
        check(f, 0, model, "behind the logged calls")
        # a lone localize_update logs as a lone update does: one innovation step, one pose row
        twin.flush()
        twin.log_innovations(8)
        twin.log_poses(8)
        twin.update(*obs)
        assert len(twin.innovations().steps) == 1 and twin.pose_steps == 1
        f.log_innovations(8)
        f.log_poses(8)
        f.localize_update(*obs)
        assert len(f.innovations().steps) == 1 and f.pose_steps == 1 and int(f.innovations().m[0, 0]) == int(twin.innovations().m[0, 0])
        assert path_ran(f, both_paths)


# ---- 9: the uploaded stream, and the position in a bank ------------------------------------------------------------------------
def test_stream_and_bank_position(sd, both_paths):
    K = 12
    ss = small_streams(3)
    with bank(sd, ss, steps=SLAM_STEPS) as f, sd.EkfSlam(43, batch=3) as g, sd.EkfSlam(43, batch=1) as alone:
        f.flush()
        for b in range(3):                                 # the same bits in all three handles
            g.set_state(*f.state(b), b)
        alone.set_state(*f.state(2), 0)
        assert all(same(f.state(b), g.state(b)) for b in range(3)) and same(f.state(2), alone.state(0))
        model = f.state(1)
        f.run_localize(SLAM_STEPS, K)
        for k in range(SLAM_STEPS, SLAM_STEPS + K):
            g.localize(*streams.steps_of(ss, k))
            alone.localize(ss[2][2][k], ss[2][3][k], ss[2][4][k], ss[2][5][k], ss[2][6][k])
            model = lm.literal_step(*model, ss[1][2][k], ss[1][3][k], ss[1][4][k], ss[1][5][k], ss[1][6][k], CFG)
        for b in range(3):
            assert same(f.state(b), g.state(b)), f"trajectory {b}: run_localize and {K} localize calls differ"
        assert same(g.state(2), alone.state(0)), "the same trajectory alone and in slot 2 of a bank"
        check(f, 1, model, f"run_localize over {K} steps")
        # the stream stays runnable
        before = f.state(0)
        f.stream_run(0, 2)
        want = before
        for k in range(2):
            want = orc.ekf_step_dense(*want, ss[0][2][k], ss[0][3][k], ss[0][4][k], ss[0][5][k], ss[0][6][k], CFG)
        check(f, 0, want, "stream_run behind run_localize")
        assert path_ran(f, both_paths)


# ---- 10: back to SLAM, and the read-only queries ---------------------------------------------------------------------------------
def test_back_to_slam_and_queries(sd, both_paths):
    s = small_streams(1)[0]
    with bank(sd, [s], steps=SLAM_STEPS) as f:
        f.flush()
        model = f.state(0)
        for k in range(SLAM_STEPS, SLAM_STEPS + 10):
            f.localize(s[2][k], s[3][k], s[4][k], s[5][k], s[6][k])
            model = lm.literal_step(*model, s[2][k], s[3][k], s[4][k], s[5][k], s[6][k], CFG)
        pose, lms = f.marginals(0)
        jm, jc = f.joint([7, 2], 0)
        sel = [0, 1, 2, 17, 18, 7, 8]
        assert lm.rel(pose, model[1][:3, :3]) <= TOL and lm.rel(jc, model[1][np.ix_(sel, sel)]) <= TOL
        assert lm.rel(jm, model[0][sel]) <= TOL and lm.rel(lms[5], model[1][13:15, 13:15]) <= TOL
        fac = f.factor(0)
        assert int(np.ravel(fac.info)[0]) == 0
        check(f, 0, model, "ten localisation steps")
        for k in range(5):
            f.step(s[2][k], s[3][k], s[4][k], s[5][k], s[6][k])
            model = orc.ekf_step_dense(*model, s[2][k], s[3][k], s[4][k], s[5][k], s[6][k], CFG)
        f.flush()
        check(f, 0, model, "five SLAM steps behind them")
        assert path_ran(f, both_paths)


# ---- 11: errors ------------------------------------------------------------------------------------------------------------------
def test_errors_change_nothing(sd, both_paths):
    s = small_streams(1)[0]
    with bank(sd, [s], steps=SLAM_STEPS) as f:
        f.flush()
        before, raw = f.state(0), pbase(sd, f, 0)
        with pytest.raises(sd.EkfError):
            f.localize(0.004, 0.02, [3, 20], [1.0, 1.0], [0.1, 0.2])           # landmarks 0..19 exist
        with pytest.raises(sd.EkfError):
            f.localize_update([-1], [1.0], [0.1])
        lib = sd.load_library()
        one, idx, m = np.array([0.004]), np.array([1, 2, 3, 4], dtype=np.int32), np.array([5], dtype=np.int32)
        z = np.ones(4)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        with pytest.raises(sd.EkfError):                                       # m > stride
            f._check(lib.ekf_localize_step(f._h, one.ctypes.data_as(dp), one.ctypes.data_as(dp), idx.ctypes.data_as(ip),
                                           z.ctypes.data_as(dp), z.ctypes.data_as(dp), m.ctypes.data_as(ip), 4))
        with pytest.raises(sd.EkfError):
            f.run_localize(0, 10 ** 6)                                         # beyond the uploaded stream
        assert same(f.state(0), before) and np.array_equal(pbase(sd, f, 0), raw) and f.flags(0) == 0
        f.localize(0.004, 0.02, [3], [1.0], [0.1])                             # and the handle is usable
        assert not same(f.state(0), before)
        assert path_ran(f, both_paths)


# ---- 12: degenerate geometry -------------------------------------------------------------------------------------------------------
def test_pose_on_the_landmark_sets_nonfinite(sd, both_paths):
    """q = 0 (the pose mean on the observed landmark's mean) gives NaN as on the other paths, and the sticky flag; the map and
    the neighbour in the bank stay as they were."""
    mean0, diag0 = (x.copy() for x in orc.synthetic_world(20, 0)[2:4])
    diag0[3:] = 0.5
    with sd.EkfSlam(43, batch=2) as f:
        for b in range(2):
            f.set_state_diag(mean0, diag0, b)
        f.step(0.004, 0.02, [[1, 2]] * 2, [[1.0, 1.1]] * 2, [[0.1, 0.2]] * 2)       # (a SLAM step: the path is visible)
        f.flush()
        bad = f.state(0)[0].copy()
        bad[3:5] = bad[0:2]                                 # landmark 0 at the pose
        f.set_state(bad, f.state(0)[1], 0)
        frozen, other = frozen_part(sd, f, 0), f.state(1)
        f.localize_update([[0], []], [[1.0], []], [[0.1], []])
        assert f.flags(0) & 1 and f.flags(1) == 0         # EKF_FLAG_NONFINITE
        mu = f.mean(0)
        assert np.isnan(mu[:3]).all() and np.array_equal(mu[3:], bad[3:])
        assert np.array_equal(frozen_part(sd, f, 0)[0], frozen[0]) and same(f.state(1), other)
        assert path_ran(f, both_paths)


# ---- 13: an uneven bank: three sizes and three bounds under one launch grid ----------------------------------------------------
def pose_rows(sd, f, b):
    """Rows 0..2 of trajectory b's stored P_base, every stored column (n_max = 79: a leading dimension of 128)."""
    assert f.n_max == 79
    return pbase(sd, f, b).reshape(-1, 128)[:3].copy()


def test_uneven_bank(sd, both_paths):
    """One handle, n = (23, 63, 79).  Trajectory 0 and 2 are dense; trajectory 1 is the pair table's start after its prelude
    (tests/sequence_cases.py): bound 55, four loose landmarks with exact zeros.  Four localize calls with m = (2, 3, 0), the
    third naming a loose landmark of trajectory 1, then one localize_update in which trajectory 2 has m = 0.  The smallest
    sizes that put three different bounds under one launch grid."""
    s = sc.start()
    sizes, bound1, T, K0 = (23, 63, 79), 3 + 2 * sc.N_OBSERVED, sc.STREAM_STEPS + sc.SINGLE_STEPS, sc.STREAM_STEPS
    rng = np.random.default_rng(13)
    lin, ang = np.zeros((T, 3)), np.zeros((T, 3))
    idx, zr, zb, m = np.zeros((T, 3, 4), dtype=np.int32), np.zeros((T, 3, 4)), np.zeros((T, 3, 4)), np.zeros((T, 3), dtype=np.int32)
    lin[:, 1], ang[:, 1], idx[:, 1], zr[:, 1], zb[:, 1], m[:, 1] = s[2][:T], s[3][:T], s[4][:T], s[5][:T], s[6][:T], 4
    want1 = sc.new_model()
    drv = sc.Driver(want1)
    sc.setup(drv)
    sc.prelude(drv)
    with sd.EkfSlam(79, batch=3) as f:
        f.set_state(orc.synthetic_world(10, 21)[2], streams.dense_start(23, 5), 0)
        f.set_state_diag(s[0], s[1], 1)
        f.set_state(orc.synthetic_world(38, 22)[2], streams.dense_start(79, 6), 2)
        f.run_stream(lin[:K0], ang[:K0], idx[:K0], zr[:K0], zb[:K0], m[:K0])     # the prelude: trajectories 0 and 2 see nothing
        for k in range(K0, T):
            f.step(lin[k], ang[k], [[], idx[k, 1], []], [[], zr[k, 1], []], [[], zb[k, 1], []])
        f.flush()
        f.profile_enable(True)
        model = [f.state(b) for b in range(3)]             # taken once, before the first call
        assert [len(x[0]) for x in model] == list(sizes) == [f.size(b) for b in range(3)]
        check(f, 1, (want1.tr.mean, want1.tr.cov), "uneven bank, trajectory 1: the pair table's start")
        assert not model[1][1][:bound1, bound1:].any() and model[0][1][:3, 3:].all() and model[2][1][:3, 3:].all()
        frozen = [frozen_part(sd, f, b) for b in range(3)]
        raw = [pose_rows(sd, f, b) for b in range(3)]
        sched = scheduling(sd, f)
        named = ([[1, 7], [9, 0], [4, 4], [2, 8]],
                 [[3, 12, 3], [25, 0, 14], [27, 5, 1], [8, 27, 20]],       # landmark 27 is loose: named in the third call
                 [[], [], [], []])
        for k in range(4):
            obs = [observe(model[b][0], named[b][k], rng) for b in range(3)]
            w = 0.02 if k % 2 else 0.005
            f.localize(0.004, w, [o[0] for o in obs], [o[1] for o in obs], [o[2] for o in obs])
            for b in range(3):
                model[b] = lm.literal_step(*model[b], 0.004, w, *obs[b], CFG)
            if k < 2:                                      # no loose landmark named yet: nothing at or beyond the bound moves
                assert np.array_equal(pose_rows(sd, f, 1)[:, bound1:], raw[1][:, bound1:]), f"call {k}: columns beyond the bound moved"
        assert pose_rows(sd, f, 1)[:, 3 + 2 * 27:5 + 2 * 27].all()
        whole = (pbase(sd, f, 2), f.mean(2))
        obs = [observe(model[0][0], [5, 3], rng), observe(model[1][0], [26, 10, 27], rng), observe(model[2][0], [], rng)]
        f.localize_update([o[0] for o in obs], [o[1] for o in obs], [o[2] for o in obs])
        for b in range(3):
            model[b] = lm.literal_step(*model[b], 0.0, 0.0, *obs[b], CFG, predict=False)
        assert np.array_equal(pbase(sd, f, 2), whole[0]) and np.array_equal(f.mean(2), whole[1]), "m = 0: the trajectory moved"
        assert scheduling(sd, f) == sched                  # no covariance pass, no cadence
        for b in range(3):
            after = pose_rows(sd, f, b)
            assert np.array_equal(after[:, sizes[b]:], raw[b][:, sizes[b]:]), f"trajectory {b}: columns beyond n = {sizes[b]} moved"
            assert not np.array_equal(after[:, :sizes[b]], raw[b][:, :sizes[b]])
            check(f, b, model[b], f"uneven bank, trajectory {b} (n = {sizes[b]})")
            assert frozen_same(frozen_part(sd, f, b), frozen[b]), f"trajectory {b}: the map moved"
        assert path_ran(f, both_paths)
