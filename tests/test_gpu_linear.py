"""GPU: linear measurements (ekf_update_linear, EkfSlam.update_linear / constrain_landmarks / update_custom) against the NumPy
reference tests/linear_model.py applied to state() taken just before the call.

Tolerance: TIGHT = 1e-9, held twice.  As a relative Frobenius norm over the whole mean and the whole covariance
(tests/test_gpu_direct.py's bound) -- a metric the never-observed landmarks at variance 1e4 dominate: a pose block 0.1 % off
moves it by 4e-10 (tests/test_update_blocks_cpu.py pins that).  And block by block (parity_blocks.assert_update_close, against
the Joseph form of the reference): pose block, pose-landmark cross rows, landmark block, the correlation-scaled largest entry
and the means of everything that was active before the call, each on its own scale at TIGHT; a landmark the call touches
first: its own block to 32 eps landmark_init_var, its mean to 1e-9, its cross terms entrywise at TIGHT; every other
never-observed landmark bit for bit, with exact zeros in its rows; P exactly symmetric.  tests/test_update_blocks_cpu.py shows
that on these very inputs the simple and the Joseph form of the reference agree on every such piece to 1e-11, so 1e-9 is a
statement about the device code and not about the conditioning of the inputs.  The exception is trajectory 1 of the bank test,
whose dense H ties two never-observed landmarks in: there the forms themselves differ by 2.2e-10 in single entries, and the
per-entry pieces (corr_max, mean_landmarks, the first-touched cross terms) are held to ten times that measured figure
(update_cases.DENSE_NEVER), the relative Frobenius pieces to TIGHT like everywhere else."""
import ctypes as C

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests import direct_model as dm
from tests import linear_model as lm
from tests import parity_blocks as pb
from tests import update_cases as uc
from tests.conftest import path_ran
from tests.gpu_support import bank, sd  # noqa: F401

pytestmark = pytest.mark.gpu

TIGHT = 1e-9
EKF_ERR_ARG, EKF_ERR_STATE = -1, -3


def check_against_model(f, b, before, meas, res, innovation=False, gate=np.inf):
    lms, H, R, r = meas
    wm, wP, nis, dof, ok = lm.linear_update(before[0], before[1], lms, H, R, r, innovation, gate)
    mu, P = f.state(b)
    assert np.array_equal(P, P.T)
    assert bool(res.applied[b]) == ok and res.dof[b] == dof
    if dof:
        assert res.nis[b] == pytest.approx(nis, rel=1e-9)
    e_mu, e_P = orc.rel_fro(mu, wm), orc.rel_fro(P, wP)
    print(f"trajectory {b}: D = {dof} nis {res.nis[b]:.6g} rel_fro mean {e_mu:.2e} cov {e_P:.2e}")
    assert e_mu <= TIGHT and e_P <= TIGHT, (b, e_mu, e_P)
    # block by block against the Joseph form (on the closed system the call touches: affordable at N = 2050 too)
    entry_tol, cross_tol = uc.dense_never_bounds(lms, before[1])
    want = uc.linear_reference(before, meas, innovation, gate)
    err = pb.assert_update_close((mu, P), want, before, lms, f.config.landmark_init_var, TIGHT, what=f"trajectory {b}: ",
                                 entry_tol=entry_tol, first_cross_tol=cross_tol)
    print(f"trajectory {b}: {pb.fmt_update(err)}")
    return wm, wP


def test_small_state_on_both_paths(sd, both_paths):
    """N = 20, 30 steps: a dense H with D = 7 over the pose and three landmarks in z mode, on the small-state path and on the
    general kernels; one more step."""
    s, lms, H, R, z = lm.case_small()
    k = dm.SMALL_STEPS
    with bank(sd, [s], steps=k) as f:
        assert path_ran(f, both_paths)
        before = f.state(0)
        res = f.update_linear(lms, H, R, z=z, b=0)
        assert res.applied[0] and res.dof[0] == 7
        check_against_model(f, 0, before, (lms, H, R, z), res)
        mu, P = f.state(0)
        f.step(s[2][k], s[3][k], s[4][k], s[5][k], s[6][k])
        want = orc.ekf_step_dense(mu, P, s[2][k], s[3][k], s[4][k], s[5][k], s[6][k], orc.EkfConfig())
        got = f.state(0)
        e = orc.rel_fro(got[0], want[0]), orc.rel_fro(got[1], want[1])
        print("the step behind it: rel_fro mean %.2e cov %.2e" % e)
        assert max(e) <= TIGHT
        err = pb.assert_filter_close(got[0], got[1], want[0], want[1], pb.active_of(want[1], f.config.landmark_init_var),
                                     mean0=mu, diag0=np.diag(P), tol=TIGHT, what="the step behind it: ")
        print("the step behind it:", pb.fmt(err))
        assert path_ran(f, both_paths)


def test_the_hook_reproduces_the_built_in_model(sd):
    """The reference's own range/bearing observation of one landmark, linearised on the host at joint()'s sub-mean and applied
    in innovation mode with the filter's measurement noise, against a twin that takes the same observation through update()."""
    s, l, zr, zb = lm.case_hook()
    with bank(sd, [s], steps=dm.SMALL_STEPS) as f, bank(sd, [s], steps=dm.SMALL_STEPS) as twin:
        xs, _ = f.joint([l], 0)
        h, J = lm.range_bearing(np.array(xs))
        y = np.array([zr - h[0], orc.wrap_pi(zb - h[1])])
        res = f.update_linear([l], J, np.diag(orc.EkfConfig().meas_noise_diag()), innovation=y, b=0)
        assert res.applied[0] and res.dof[0] == 2
        twin.update([l], [zr], [zb])
        a, b = f.state(0), twin.state(0)
        e = orc.rel_fro(a[0], b[0]), orc.rel_fro(a[1], b[1])
        print("hook against update(): rel_fro mean %.2e cov %.2e" % e)
        assert max(e) <= TIGHT and np.array_equal(a[1], a[1].T)


def test_a_selection_equals_update_direct(sd):
    s, t, z, R = lm.case_selection()
    lms, H, RR, zz = lm.selection_of(t, z, R)
    with bank(sd, [s], steps=dm.SMALL_STEPS) as f, bank(sd, [s], steps=dm.SMALL_STEPS) as twin:
        res = f.update_linear(lms, H, RR, z=zz, b=0)
        ref = twin.update_direct(t, z, R)
        assert res.applied[0] and ref.applied[0] and res.dof[0] == ref.dof[0] == 6
        assert res.nis[0] == pytest.approx(ref.nis[0], rel=1e-9)
        a, b = f.state(0), twin.state(0)
        e = orc.rel_fro(a[0], b[0]), orc.rel_fro(a[1], b[1])
        print("selection against update_direct: rel_fro mean %.2e cov %.2e" % e)
        assert max(e) <= TIGHT


def test_bank_with_ranks_pending_gate_untouched_rest_and_the_bound(sd):
    """N = 150 x 4 on the general kernels, ranks pending before the call, sizes differing per trajectory (the preparation of
    test_gpu_direct.py's bank test), one call in innovation mode: a pose-only heading row; D = 32 over 16 landmarks, two of
    them never observed; nothing; a constraint 10 sigma off under the 0.99 chi-square gate of its 2 rows.  Then ten steps
    that observe the formerly unobserved landmarks of trajectory 1 (the check of the bound rise), against the oracle continued
    from the model's result."""
    from scipy.stats import chi2
    streams, meas, draw = lm.case_bank()
    lib = sd.load_library()
    motion = [0.1, 0.11, 0.1, 0.09]

    def prepare(f):
        f.set_option("fused_cadence", 0)
        f.log_innovations(64)
        f.log_poses(64)
        f.set_nis_gate(confidence=0.999999)
        f.set_noise(motion_sigma=motion)
        f.stream_run(0, 30)
        f.remove_landmarks([149], b=0)                       # sizes differ: trajectory 0 has 149 landmarks, 3 has 148
        f.remove_landmarks([148, 149], b=3)
        f.set_tag_index({7: 0, 9: 1, 300: 2}, 1)
        f.flush()
        f.step([s[2][0] for s in streams], [s[3][0] for s in streams], [s[4][0][:2] for s in streams],
               [s[5][0][:2] for s in streams], [s[6][0][:2] for s in streams])       # 4 ranks are pending from here on

    def counters(f):
        logged = C.c_longlong()
        assert lib.ekf_innovation_steps(f._h, C.byref(logged)) == 0
        return (f.gate_counts().copy(), int(logged.value), f.pose_steps, [np.array(x).copy() for x in f.noise()],
                [f.size(b) for b in range(4)], f.tag_index(1))

    # the flushed pre-call state comes from a twin driven through the identical sequence: the bank under test is neither
    # flushed nor downloaded between its last step() and the call
    with bank(sd, streams, run=False) as twin:
        prepare(twin)
        before = [twin.state(b) for b in range(4)]
    ys = [lm.bank_innovation(b, meas, draw, *before[b]) for b in range(4)]
    gate = [np.inf, np.inf, np.inf, chi2.ppf(0.99, 2)]
    with bank(sd, streams, run=False) as f:
        prepare(f)
        f.set_option("profile_kernels", 1)
        f.profile_enable(True)                               # (synchronises; applies nothing)
        c0 = counters(f)
        assert f.profile_passes() == 0
        res = f.update_linear([m[0] for m in meas], [m[1] for m in meas], [m[2] for m in meas], innovation=ys, gate=gate)
        assert f.profile_passes() == 2                       # the pass of what was pending, then the pass of the call
        assert f.profile_read_class(5)[1] == 1               # one k_linear launch for the whole bank
        assert list(res.applied) == [True, True, False, False] and list(res.dof) == [1, 32, 0, 2]
        assert res.nis[3] > gate[3]
        after = []
        for b in range(4):
            after.append(check_against_model(f, b, before[b], meas[b] + (ys[b],), res, True, gate[b]))
        for b in (2, 3):
            got = f.state(b)
            assert np.array_equal(got[0], before[b][0]) and np.array_equal(got[1], before[b][1])
        c1 = counters(f)
        assert np.array_equal(c0[0], c1[0]) and c0[1:3] == c1[1:3] and c0[4:] == c1[4:]
        assert all(np.array_equal(a, b) for a, b in zip(c0[3], c1[3]))
        assert f.profile_passes() == 2                       # nothing was pending: the downloads above ran no pass
        # life goes on: ten steps; trajectory 1's observe the landmarks its bound was raised over
        for k in range(1, 11):
            obs = [lm.follow_up_obs(after[b][0], lm.bank_follow_up(b), k) for b in range(4)]
            idx = [lm.bank_follow_up(b) for b in range(4)]
            f.step([s[2][k] for s in streams], [s[3][k] for s in streams], idx, [o[0] for o in obs], [o[1] for o in obs])
            for b, s in enumerate(streams):
                after[b] = orc.ekf_step_dense(after[b][0], after[b][1], s[2][k], s[3][k], idx[b], obs[b][0], obs[b][1],
                                              orc.EkfConfig(motion_sigma=motion[b]))
        assert np.array_equal(f.gate_counts(), c0[0])        # (the follow-up observations are no outliers)
        for b in range(4):
            mu, P = f.state(b)
            e = orc.rel_fro(mu, after[b][0]), orc.rel_fro(P, after[b][1])
            print("trajectory %d after ten more steps: rel_fro mean %.2e cov %.2e" % ((b,) + e))
            assert max(e) <= TIGHT
            # (trajectory 1 carries the entrywise difference of its update along: update_cases.DENSE_NEVER)
            err = pb.assert_filter_close(mu, P, after[b][0], after[b][1], pb.active_of(after[b][1], f.config.landmark_init_var),
                                         tol=TIGHT, what=f"trajectory {b} after ten more steps: ",
                                         corr_tol=uc.dense_never_bounds(meas[b][0], before[b][1])[0])
            print("trajectory %d after ten more steps: %s" % (b, pb.fmt(err)))


def test_relative_constraint_and_the_merge_recipe(sd):
    from slam_duckietown_amd import evaluation as ev
    s, i, j, offset, cov = lm.case_constraint()
    with bank(sd, [s], steps=dm.SMALL_STEPS) as f:
        before = f.state(0)
        res = f.constrain_landmarks(i, j, offset, cov, b=0)
        assert res.applied[0] and res.dof[0] == 2
        check_against_model(f, 0, before, lm.constraint_rows(i, j, offset, cov), res)
        dist, sigma, _ = ev.landmark_separation(f, [(i, j)], 0)
        print("separation %.6f against |offset| %.6f, sigma %.2e" % (dist[0], np.hypot(*offset), sigma[0]))
        assert abs(dist[0] - np.hypot(*offset)) <= sigma[0] and sigma[0] < 2 * lm.CONSTRAINT_SIGMA
        # the merge recipe: "i and j are the same landmark", then j leaves the map
        before = f.state(0)
        res = f.constrain_landmarks(i, j, [0.0, 0.0], cov, b=0)
        assert res.applied[0]
        wm, wP, _, _, _ = lm.linear_update(before[0], before[1], *lm.constraint_rows(i, j, [0.0, 0.0], cov))
        f.remove_landmarks([j], b=0)
        gone = [3 + 2 * j, 4 + 2 * j]
        wm, wP = np.delete(wm, gone), np.delete(np.delete(wP, gone, 0), gone, 1)
        mu, P = f.state(0)
        assert mu.shape == wm.shape and np.array_equal(P, P.T)
        e = orc.rel_fro(mu, wm), orc.rel_fro(P, wP)
        print("merged: rel_fro mean %.2e cov %.2e" % e)
        assert max(e) <= TIGHT


def test_constraint_across_the_column_panel(sd):
    """N = 2050 (n = 4103: two column panels), diagonal start, 5 steps: a constraint between landmark 2046 -- never observed,
    state indices 4095 and 4096 on either side of the panel boundary -- and an observed low landmark.  One call.

    |P|_F is 6e5 here, so the whole-matrix 1e-9 allows 6e-4 absolutely -- the size of the variances the update is about.  What
    judges the update is check_against_model's block-wise part: the pose and the 40 observed landmarks piece by piece at
    TIGHT, landmark 2046's block, mean and cross terms (it is touched first), the other 2009 landmarks bit for bit."""
    s, low, high, offset, cov = lm.case_panel()
    with bank(sd, [s]) as f:
        before = f.state(0)
        res = f.constrain_landmarks(low, high, offset, cov, b=0)
        assert res.applied[0] and res.dof[0] == 2
        check_against_model(f, 0, before, lm.constraint_rows(low, high, offset, cov), res)


def test_bank_position_and_repeat_leave_the_bits_alone(sd):
    """The same trajectory at positions 0 and 3 of a bank of 4 (another one at 1, nothing for 2): identical bits; the whole
    run repeated: identical bits."""
    s, lms, H, R, z = lm.case_small()
    other = dm.small_stream(8)
    runs = []
    # (the repeat hands the same call over as padded arrays with counts instead of ragged lists)
    Lp, Hp, Rp, zp = np.zeros((4, 3), dtype=np.int32), np.zeros((4, 7, 9)), np.zeros((4, 7, 7)), np.zeros((4, 7))
    for b in (0, 3):
        Lp[b], Hp[b], Rp[b], zp[b] = lms, H, R, z
    Lp[1, 0], Hp[1, :3, :5], Rp[1, :3, :3], zp[1, :3] = 2, H[:3, :5], R[:3, :3], z[:3]
    for rep in range(2):
        with bank(sd, [s, other, dm.small_stream(9), s], steps=dm.SMALL_STEPS) as f:
            if rep == 0:
                res = f.update_linear([lms, [2], [], lms], [H, H[:3, :5], None, H], [R, R[:3, :3], None, R], z=[z, z[:3], [], z])
            else:
                res = f.update_linear((Lp, [3, 1, 0, 3]), Hp, Rp, z=(zp, [7, 3, 0, 7]))
            assert list(res.applied) == [True, True, False, True] and list(res.dof) == [7, 3, 0, 7]
            runs.append([f.state(b) for b in range(4)] + [res.nis.copy()])
    a = runs[0]
    assert np.array_equal(a[0][0], a[3][0]) and np.array_equal(a[0][1], a[3][1]) and a[4][0] == a[4][3]
    for b in range(4):
        assert np.array_equal(runs[0][b][0], runs[1][b][0]) and np.array_equal(runs[0][b][1], runs[1][b][1])
    assert np.array_equal(runs[0][4], runs[1][4])


def test_update_custom_with_central_differences(sd):
    """A tape measure between two landmarks (nonlinear; no Jacobian given: central differences) against the model fed with
    the analytic Jacobian at the same sub-mean.

    Tolerance: TIGHT plus the finite-difference error.  With the step t = 1e-5 (update_custom's default) a Jacobian entry
    carries at most  fd = t^2 / 6 * max|h'''| + eps * (|h| + max|x_s|) / t  -- truncation, with |h'''| <= 3 / r^2 for the
    distance r, and the rounding of h's two values and of x_s +- t: about 5e-11 / r^2 + 7e-11 here.  J has four non-zero
    entries and Frobenius norm sqrt(2), so its relative error is at most  e = fd * 2 / sqrt(2).  P+ = P - P H^T S^-1 H P holds
    H four times (twice in S), so to first order |dP+| <= 4 e |P H^T S^-1 H P| <= 4 e |P|; K y holds it three times."""
    s, pair, z, R = lm.case_custom()
    step = 1e-5
    with bank(sd, [s], steps=dm.SMALL_STEPS) as f:
        before = f.state(0)
        xs = before[0][lm.sub_indices(pair)]
        h, J, d3 = lm.distance_model(xs)
        res = f.update_custom(pair, lambda x: lm.distance_model(x)[0], z, R, b=0, step=step)
        assert res.applied[0] and res.dof[0] == 1
        wm, wP, nis, _, _ = lm.linear_update(before[0], before[1], pair, J, R, z - h, True)
        fd = step ** 2 / 6.0 * d3 + np.finfo(float).eps * (h[0] + np.abs(xs).max()) / step
        tol = TIGHT + 4.0 * fd * 2.0 / np.sqrt(2.0)
        mu, P = f.state(0)
        e = orc.rel_fro(mu, wm), orc.rel_fro(P, wP)
        print("custom model: rel_fro mean %.2e cov %.2e, tolerance %.2e (fd %.2e)" % (e + (tol, fd)))
        assert max(e) <= tol and np.array_equal(P, P.T)
        assert res.nis[0] == pytest.approx(nis, rel=1e-6)


def test_abi_refusals_leave_the_state_alone(sd):
    from slam_duckietown_amd import ekf_bindings as eb
    s = orc.synthetic_stream(40, 6, 4, 3)
    lib = sd.load_library()
    with bank(sd, [s, s]) as f:
        before = [f.state(b) for b in range(2)]
        rng = np.random.default_rng(1)
        Hg = rng.uniform(-1.0, 1.0, (2, 4, 9))
        Rg = np.zeros((2, 4, 4))
        Rg[:] = np.diag([0.01, 0.02, 0.01, 0.03]) + 0.001
        rg = rng.normal(size=(2, 4)) * 0.1

        def call(b0=0, count=2, lm_=((5, 2, 7), (1, 0, 0)), k=(3, 1), lstride=3, H=Hg, r=rg, R=Rg, d=(3, 2), dstride=4,
                 innovation=1, gate=None, null=None):
            L, kk, dd = eb._i32(np.array(lm_)), eb._i32(np.array(k)), eb._i32(np.array(d))
            H, r, R = eb._f64(H), eb._f64(r), eb._f64(R)
            g = eb._f64(np.array(gate, dtype=float)) if gate is not None else None
            args = dict(landmarks=eb._p(L, eb._ip), k=eb._p(kk, eb._ip), H=eb._p(H), r=eb._p(r), R=eb._p(R), d=eb._p(dd, eb._ip))
            if null:
                args[null] = None
            return lib.ekf_update_linear(f._h, b0, count, args["landmarks"], args["k"], lstride, args["H"], args["r"], args["R"],
                                         args["d"], dstride, innovation, eb._p(g) if g is not None else None, None, None)

        bad_H, bad_r, bad_R, npd, zero_var = Hg.copy(), rg.copy(), Rg.copy(), Rg.copy(), Rg.copy()
        bad_H[0, 2, 8] = np.nan
        bad_r[1, 1] = np.inf
        bad_R[0, 0, 2] = np.inf
        npd[0, 0, 1] = 0.05
        zero_var[1, 1, 1] = 0.0
        refusals = [dict(b0=1, count=2), dict(b0=-1), dict(count=0), dict(lstride=0), dict(lstride=17), dict(dstride=0),
                    dict(dstride=33), dict(k=(4, 1)), dict(k=(3, -1)), dict(d=(5, 2)), dict(d=(3, -1)),
                    dict(lm_=((5, 2, 40), (1, 0, 0))), dict(lm_=((5, -1, 7), (1, 0, 0))), dict(lm_=((5, 2, 5), (1, 0, 0))),
                    dict(H=bad_H), dict(r=bad_r), dict(R=bad_R), dict(R=npd), dict(R=zero_var),
                    dict(gate=(np.nan, 1.0)), dict(gate=(1.0, 0.0)), dict(gate=(-1.0, 1.0)),
                    dict(null="landmarks"), dict(null="k"), dict(null="H"), dict(null="r"), dict(null="R"), dict(null="d")]
        for kw in refusals:
            assert call(**kw) == EKF_ERR_ARG, kw
            assert b"ekf_update_linear" in lib.ekf_last_error(f._h)
        for b in range(2):
            after = f.state(b)
            assert np.array_equal(after[0], before[b][0]) and np.array_equal(after[1], before[b][1])
        zero_row = Hg.copy()
        zero_row[0, 1, :] = 0.0
        assert call(H=zero_row, gate=(np.inf, 50.0)) == 0    # a zero row is legal; the handle is usable
        assert orc.rel_fro(f.state(0)[1], before[0][1]) > 1e-6
    with sd.EkfSlam(len(s[0])) as f:                         # EKF_FLAG_INTERNAL: the bounded wait of a single-launch step
        f.set_option("active_bound", 0)
        f.set_state_diag(s[0], s[1])
        f.step(s[2][0], s[3][0], s[4][0], s[5][0], s[6][0])
        f.sync()
        f.set_option("fused_step", 2)
        f.step(s[2][1], s[3][1], s[4][1], s[5][1], s[6][1])
        with pytest.raises(sd.EkfError, match="EKF_FLAG_INTERNAL"):
            f.update_linear([], [[0.0, 0.0, 1.0]], [[0.01]], innovation=[0.0], b=0)
        assert f.flags(0) & eb.EKF_FLAG_INTERNAL
