"""GPU: predictions with the caller's motion model (ekf_predict_linear, EkfSlam.predict_linear / predict_odometry /
predict_custom) against the NumPy reference tests/motion_model.py applied to state() taken just before the call.

Tolerance: TIGHT = 1e-9 relative Frobenius over the whole mean and the whole covariance (tests/test_gpu_direct.py's and
tests/test_gpu_linear.py's bound for a device update against its NumPy model); tests/test_predict_linear_cpu.py shows that on
these very inputs the dense and the delta form of the reference agree to 1e-11, so 1e-9 is a statement about the device
code.  The whole-matrix norm is dominated by the never-observed landmarks' 1e4 on the diagonal, so the same bound is also
asked of rows 0..2 alone -- the only entries the call writes."""
import ctypes as C

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests import direct_model as dm
from tests import linear_model as lm
from tests import motion_model as mm
from tests.conftest import path_ran
from tests.gpu_support import bank, raw00, same, sd  # noqa: F401

pytestmark = pytest.mark.gpu

TIGHT = 1e-9
EKF_ERR_ARG, EKF_ERR_STATE = -1, -3
I3, Z3 = np.eye(3), np.zeros((3, 3))


def check_against_model(got, before, inputs, what=""):
    """The state `got` against the model applied to `before`; what the call must leave alone, bit for bit.  Returns the
    model's result."""
    pose, F, Q = inputs
    wm, wP = mm.predict_linear(before[0], before[1], pose, F, Q)
    mu, P = got
    e = orc.rel_fro(mu, wm), orc.rel_fro(P, wP), orc.rel_fro(P[:3], wP[:3])
    print("%s rel_fro mean %.2e cov %.2e rows 0..2 %.2e" % ((what,) + e))
    assert max(e) <= TIGHT, e
    assert np.array_equal(P, P.T)
    assert np.array_equal(mu[:3], np.asarray(pose)) and np.array_equal(mu[3:], before[0][3:])
    assert np.array_equal(P[3:, 3:], before[1][3:, 3:])
    return wm, wP


# ---- 1: both paths ----------------------------------------------------------------------------------------------------------
def test_small_state_on_both_paths(sd, both_paths):
    """N = 20, 30 steps: a random F and a full Q on the small-state path and on the general kernels; one more step."""
    s, rng = mm.case_small()
    k = dm.SMALL_STEPS
    with bank(sd, [s], steps=k) as f:
        assert path_ran(f, both_paths)
        before = f.state(0)
        inputs = mm.draw(rng, *before)
        f.predict_linear(*inputs, b=0)
        wm, wP = check_against_model(f.state(0), before, inputs, "after the call:")
        f.step(s[2][k], s[3][k], s[4][k], s[5][k], s[6][k])
        want = orc.ekf_step_dense(wm, wP, s[2][k], s[3][k], s[4][k], s[5][k], s[6][k], orc.EkfConfig())
        got = f.state(0)
        e = orc.rel_fro(got[0], want[0]), orc.rel_fro(got[1], want[1])
        print("the step behind it: rel_fro mean %.2e cov %.2e" % e)
        assert max(e) <= TIGHT
        assert path_ran(f, both_paths)


@pytest.mark.parametrize("kind", ["rank1", "zero"])
def test_singular_noise(sd, kind):
    """A Q of rank 1 and an all-zero Q (both legal), N = 20 on the general kernels."""
    s, rng = mm.case_small(kind=kind)
    with bank(sd, [s], steps=dm.SMALL_STEPS, options=[("small_state", 0)]) as f:
        before = f.state(0)
        inputs = mm.draw(rng, *before, kind)
        f.predict_linear(*inputs, b=0)
        check_against_model(f.state(0), before, inputs, kind + ":")
        assert path_ran(f, "general_kernels")


# ---- 2: the built-in model ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("branch", ["arc", "straight"])
def test_the_built_in_model_is_reproduced(sd, branch):
    """A twin takes predict(lin, ang); the handle takes the same model linearised on the host, with the filter's noise."""
    s = dm.small_stream()
    with bank(sd, [s], steps=dm.SMALL_STEPS) as f, bank(sd, [s], steps=dm.SMALL_STEPS) as twin:
        xs, _ = f.joint([], 0)
        lin, ang, pose, G, Qd = mm.builtin_inputs(np.array(xs), branch)
        f.predict_linear(pose, G, Qd, b=0)
        twin.predict(lin, ang)
        a, b = f.state(0), twin.state(0)
        e = orc.rel_fro(a[0], b[0]), orc.rel_fro(a[1], b[1]), orc.rel_fro(a[1][:3], b[1][:3])
        print("%s against predict(): rel_fro mean %.2e cov %.2e rows 0..2 %.2e" % ((branch,) + e))
        assert max(e) <= TIGHT and np.array_equal(a[1], a[1].T)


# ---- 3: ranks pending, a bank -------------------------------------------------------------------------------------------------
def test_bank_with_ranks_pending_runs_no_pass(sd):
    """N = 150 x 4 on the general kernels, sizes differing per trajectory, 4 ranks pending before the call (the preparation of
    test_gpu_linear.py's bank test); apply = [1, 1, 0, 1].  The call runs no covariance pass; ten more steps against the
    oracle continued from the model's result."""
    streams, rng = mm.case_bank()
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
        return (f.gate_counts().copy(), int(logged.value), [np.array(x).copy() for x in f.noise()],
                [f.size(b) for b in range(4)], f.tag_index(1), f.cadence_counters(), lib.ekf_debug_chained(f._h),
                lib.ekf_debug_lookaheads(f._h))

    # the flushed pre-call state comes from a twin driven through the identical sequence: the bank under test is neither
    # flushed nor downloaded between its last step() and the call
    with bank(sd, streams, run=False) as twin:
        prepare(twin)
        before = [twin.state(b) for b in range(4)]
    inputs = [mm.draw(rng, *before[b]) for b in range(4)]
    with bank(sd, streams, run=False) as f:
        prepare(f)
        f.set_option("profile_kernels", 1)
        f.profile_enable(True)                               # (synchronises; applies nothing)
        assert raw00(sd, f, 0) != before[0][1][0, 0]         # ranks and pose noise are pending
        c0, poses0 = counters(f), f.pose_steps
        assert f.profile_passes() == 0
        f.predict_linear([i[0] for i in inputs], [i[1] for i in inputs], [i[2] for i in inputs], apply=mm.BANK_APPLY)
        assert f.profile_passes() == 0                       # no covariance pass
        assert f.profile_read_class(7)[1] == 1               # one k_predict_pose launch for the whole bank
        c1 = counters(f)
        assert np.array_equal(c0[0], c1[0]) and c0[1] == c1[1] and c0[3:] == c1[3:] and f.pose_steps == poses0 + 1
        assert all(np.array_equal(a, b) for a, b in zip(c0[2], c1[2]))
        f.flush()
        assert f.profile_passes() == 1                       # ... so the ranks were still pending when the call ran
        after = []
        for b in range(4):
            got = f.state(b)
            if mm.BANK_APPLY[b]:
                after.append(check_against_model(got, before[b], inputs[b], "trajectory %d:" % b))
            else:
                assert same(got, before[b])
                after.append(before[b])
        # life goes on: ten steps
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


# ---- 4: bits ------------------------------------------------------------------------------------------------------------------
def pending_bank(sd):
    """Four trajectories of N = 20 on the general kernels -- the same stream at positions 0 and 3 --, 30 stream steps and one
    online step: ranks are pending."""
    s, k = dm.small_stream(), dm.SMALL_STEPS
    streams = [s, dm.small_stream(8), dm.small_stream(9), s]
    f = bank(sd, streams, steps=k, options=[("small_state", 0)])
    f.flush()
    f.step([t[2][k] for t in streams], [t[3][k] for t in streams], [t[4][k] for t in streams], [t[5][k] for t in streams],
           [t[6][k] for t in streams])
    return f


def test_identity_leaves_the_bits_alone(sd):
    """F = I, Q = 0 and the current pose: state() is bit for bit, with ranks pending and with nothing pending."""
    with pending_bank(sd) as twin:
        pending = raw00(sd, twin)
        before = [twin.state(b) for b in range(4)]
    assert pending != before[0][1][0, 0]                     # the download applied what was pending
    with pending_bank(sd) as f:
        f.predict_linear([m[:3] for m, _ in before], I3, Z3)
        assert raw00(sd, f) == pending                       # nothing was applied, nothing was added
        for b in range(4):
            assert same(f.state(b), before[b]), b
        f.predict_linear([m[:3] for m, _ in before], I3, Z3)  # (the downloads applied it: nothing is pending now)
        for b in range(4):
            assert same(f.state(b), before[b]), b
        assert path_ran(f, "general_kernels")


def test_bank_position_and_repeat_leave_the_bits_alone(sd):
    """The same trajectory and the same inputs at positions 0 and 3 of a bank, ranks pending: identical bits; the whole run
    repeated: identical bits."""
    with pending_bank(sd) as twin:
        before = [twin.state(b) for b in range(4)]
    assert same(before[0], before[3])
    rng = np.random.default_rng(77)
    inputs = [mm.draw(rng, *before[b]) for b in range(3)]
    inputs.append(inputs[0])
    runs = []
    for rep in range(2):
        with pending_bank(sd) as f:
            f.predict_linear([i[0] for i in inputs], [i[1] for i in inputs], [i[2] for i in inputs])
            runs.append([f.state(b) for b in range(4)])
    for b in range(4):
        check_against_model(runs[0][b], before[b], inputs[b], "trajectory %d:" % b)
        assert same(runs[0][b], runs[1][b]), b
    assert same(runs[0][0], runs[0][3])


# ---- 5: the column-panel boundary under an active bound ---------------------------------------------------------------------------
def test_across_the_column_panel_under_an_active_bound(sd):
    """N = 2050 (n = 4103: two column panels), diagonal start, 5 steps of m = 8: landmarks 0 .. 39 are observed.  A constraint
    between an observed landmark and landmark 2046 (state indices 4095 and 4096, either side of the panel boundary) raises the
    active bound to 4097 and correlates the pose with them; then the call.  Rows 0..2 against the model, exact zeros beyond
    the bound, and the bound itself: the ranks of an update behind the call reach index 4096 and stop there."""
    s, low, high, offset, cov = lm.case_panel()
    n, bound = len(s[0]), 3 + 2 * (lm.PANEL_HIGH + 1)
    lib = sd.load_library()
    with bank(sd, [s]) as f:
        assert f.constrain_landmarks(low, high, offset, cov, b=0).applied[0]
        before = f.state(0)
        assert bound == 4097 and np.all(before[1][:3, 4095:4097] != 0.0) and np.all(before[1][:3, bound:] == 0.0)
        inputs = mm.draw(np.random.default_rng(31), *before)
        f.predict_linear(*inputs, b=0)
        mu, P = f.state(0)
        wm, wP = mm.predict_linear(before[0], before[1], *inputs)
        e = orc.rel_fro(P[:3], wP[:3]), orc.rel_fro(P[:3, 4000:], wP[:3, 4000:]), orc.rel_fro(mu, wm)
        print("rows 0..2: rel_fro %.2e, their columns 4000.. %.2e, mean %.2e" % e)
        assert max(e) <= TIGHT
        assert np.all(P[:3, bound:] == 0.0) and np.all(P[bound:, :3] == 0.0)
        assert np.array_equal(P[3:, 3:], before[1][3:, 3:]) and np.array_equal(P, P.T)
        # the bound: an update of the low landmark leaves V = H P[s, :] in the rank slots, zero from the bound on
        f.update([low], [float(np.hypot(*(mu[3 + 2 * low:5 + 2 * low] - mu[:2])))], [0.0])
        V = np.empty(f.n_max + 64)
        have = lib.ekf_debug_snapshot(f._h, 0, 1, V.ctypes.data_as(C.POINTER(C.c_double)), n)
        assert have >= n
        nz = np.nonzero(V[:n])[0]
        print("rank 0 of the update behind the call: last non-zero column", nz.max())
        assert nz.max() == bound - 1


# ---- 6: between two pieces of a chained run ---------------------------------------------------------------------------------------
def test_between_two_pieces_of_a_chained_run(sd):
    """N = 500 x 1: stream_run(0, 60), the call, stream_run(60, 60), against a twin that takes the same prediction by the host
    route (state() -> model -> set_state()) between the same two pieces."""
    s, rng = mm.case_chain()
    lib = sd.load_library()
    k = mm.CHAIN_PIECE

    def start():
        f = sd.EkfSlam(len(s[0]))
        f.set_state_diag(s[0], s[1])
        f.stream_upload(*s[2:])
        return f

    with start() as twin:
        twin.stream_run(0, k)
        before = twin.state(0)
        inputs = mm.draw(rng, *before)
        twin.set_state(*mm.predict_linear(before[0], before[1], *inputs))
        twin.stream_run(k, k)
        want = twin.state(0)
    with start() as f:
        ch0 = lib.ekf_debug_chained(f._h)
        f.stream_run(0, k)
        ch1 = lib.ekf_debug_chained(f._h)
        f.predict_linear(*inputs, b=0)
        f.stream_run(k, k)
        ch2 = lib.ekf_debug_chained(f._h)
        got = f.state(0)
        print("chained cadences: %d in the first piece, %d in the second" % (ch1 - ch0, ch2 - ch1))
        assert ch1 > ch0 and ch2 > ch1 and f.flags(0) == 0
    e = orc.rel_fro(got[0], want[0]), orc.rel_fro(got[1], want[1])
    print("against the host route: rel_fro mean %.2e cov %.2e" % e)
    assert max(e) <= TIGHT


# ---- 7: the logs ------------------------------------------------------------------------------------------------------------------
def test_the_call_is_one_pose_log_row(sd, both_paths):
    s, rng = mm.case_small()
    lib = sd.load_library()
    with bank(sd, [s], steps=dm.SMALL_STEPS) as f:
        f.log_poses(16)
        f.log_innovations(16)
        f.set_nis_gate(confidence=0.999999)
        k = dm.SMALL_STEPS
        f.step(s[2][k], s[3][k], s[4][k], s[5][k], s[6][k])

        def counters():
            logged = C.c_longlong()
            assert lib.ekf_innovation_steps(f._h, C.byref(logged)) == 0
            return f.gate_counts().copy(), int(logged.value), [np.array(x).copy() for x in f.noise()], f.size(0)

        before = f.state(0)
        c0, poses0 = counters(), f.pose_steps
        inputs = mm.draw(rng, *before)
        f.predict_linear(*inputs, b=0)
        assert f.pose_steps == poses0 + 1
        row = f.poses(first=poses0, count=1)
        _, wP = mm.predict_linear(before[0], before[1], *inputs)
        assert np.array_equal(row.mean[0, 0], inputs[0])
        e = orc.rel_fro(row.cov[0, 0], wP[:3, :3])
        print("the row's pose block: rel_fro %.2e" % e)
        assert e <= TIGHT and np.array_equal(row.cov[0, 0], row.cov[0, 0].T)
        c1 = counters()
        assert np.array_equal(c0[0], c1[0]) and c0[1] == c1[1] and c0[3] == c1[3]
        assert all(np.array_equal(a, b) for a, b in zip(c0[2], c1[2]))
        assert path_ran(f, both_paths)


# ---- 8: odometry and custom models ------------------------------------------------------------------------------------------------
def test_predict_odometry(sd):
    """A pose increment with its covariance, for a bank of two at once and for one trajectory: against the model with
    compose()'s analytic Jacobians."""
    s, other = dm.small_stream(), dm.small_stream(8)
    deltas = np.array([[0.11, -0.02, 0.07], [0.05, 0.01, -0.2]])
    cov = lm.sym_upper(dm.noise_block(np.random.default_rng(9), 3))
    with bank(sd, [s, other], steps=dm.SMALL_STEPS) as f:
        before = [f.state(b) for b in range(2)]
        f.predict_odometry(deltas, cov)
        for b in range(2):
            pose, Fp, Fd = mm.compose(before[b][0][:3], deltas[b])
            check_against_model(f.state(b), before[b], (pose, Fp, Fd @ cov @ Fd.T), "odometry, trajectory %d:" % b)
        before = [f.state(b) for b in range(2)]
        f.predict_odometry(deltas[0], cov, b=1)
        pose, Fp, Fd = mm.compose(before[1][0][:3], deltas[0])
        check_against_model(f.state(1), before[1], (pose, Fp, Fd @ cov @ Fd.T), "odometry, b = 1:")
        assert same(f.state(0), before[0])


def test_predict_custom_with_central_differences(sd):
    """A slip model (no Jacobian given: central differences) against the model fed with the analytic Jacobian.

    Tolerance: TIGHT plus what the differenced Jacobian is worth -- the same central differences formed on the host from the
    same pose, pushed through the model, against the analytic Jacobian pushed through the model (no device result enters)."""
    s, rng = mm.case_small()
    step, u = 1e-6, mm.SLIP_U
    Q = mm.draw(rng, *dm.dense_of(s, dm.SMALL_STEPS))[2]
    with bank(sd, [s], steps=dm.SMALL_STEPS) as f:
        before = f.state(0)
        x = before[0][:3].copy()
        J = mm.slip_jacobian(x, u)
        Jfd = np.empty((3, 3))
        for c in range(3):
            e = np.zeros(3)
            e[c] = step
            Jfd[:, c] = (mm.slip_model(x + e, u) - mm.slip_model(x - e, u)) / (2.0 * step)
        new = mm.slip_model(x, u)
        want = mm.predict_linear(*before, new, J, Q)
        fd = mm.predict_linear(*before, new, Jfd, Q)
        tol = TIGHT + max(orc.rel_fro(fd[1], want[1]), orc.rel_fro(fd[1][:3], want[1][:3]))
        f.predict_custom(mm.slip_model, u, Q, b=0, step=step)
        mu, P = f.state(0)
        e = orc.rel_fro(mu, want[0]), orc.rel_fro(P, want[1]), orc.rel_fro(P[:3], want[1][:3])
        print("custom model: rel_fro mean %.2e cov %.2e rows 0..2 %.2e, tolerance %.2e" % (e + (tol,)))
        assert max(e) <= tol and np.array_equal(P, P.T)
        before = f.state(0)                                  # ... and with the Jacobian given: the model itself
        f.predict_custom(mm.slip_model, u, Q, jac=mm.slip_jacobian, b=0)
        x = before[0][:3]
        check_against_model(f.state(0), before, (mm.slip_model(x, u), mm.slip_jacobian(x, u), Q), "custom, analytic:")


# ---- 9: refusals --------------------------------------------------------------------------------------------------------------------
def test_abi_refusals_leave_the_state_alone(sd):
    from slam_duckietown_amd import ekf_bindings as eb
    s = orc.synthetic_stream(40, 6, 4, 3)
    lib = sd.load_library()
    with bank(sd, [s, s]) as f:
        before = [f.state(b) for b in range(2)]
        rng = np.random.default_rng(1)
        pg = np.stack([before[b][0][:3] for b in range(2)])
        Fg = I3 + 0.3 * rng.normal(size=(2, 3, 3))
        A = rng.normal(size=(2, 3, 3)) * 0.1
        Qg = A @ A.transpose(0, 2, 1)

        def call(b0=0, count=2, pose=pg, F=Fg, Q=Qg, apply=None, null=None):
            args = dict(pose=eb._f64(pose), F=eb._f64(F), Q=eb._f64(Q))
            ptr = {k: eb._p(v) for k, v in args.items()}
            if null:
                ptr[null] = None
            ap = eb._i32(np.array(apply)) if apply is not None else None
            return lib.ekf_predict_linear(f._h, b0, count, ptr["pose"], ptr["F"], ptr["Q"], eb._p(ap, eb._ip) if ap is not None else None)

        def changed(x, at, v):
            y = x.copy()
            y[at] = v
            return y

        neg_det = Qg.copy()                                  # every pair passes, the determinant is negative
        sg, r = np.array([0.2, 0.1, 0.05]), np.array([[1.0, 0.9, -0.9], [0.9, 1.0, 0.9], [-0.9, 0.9, 1.0]])
        neg_det[1] = sg[:, None] * r * sg[None, :]
        assert np.linalg.det(neg_det[1]) < 0
        refusals = [dict(b0=1, count=2), dict(b0=-1), dict(count=0), dict(b0=2, count=1),
                    dict(null="pose"), dict(null="F"), dict(null="Q"),
                    dict(pose=changed(pg, (0, 2), np.nan)), dict(pose=changed(pg, (1, 0), np.inf)),
                    dict(F=changed(Fg, (0, 2, 1), np.nan)), dict(F=changed(Fg, (1, 0, 0), -np.inf)),
                    dict(Q=changed(Qg, (0, 0, 2), np.nan)), dict(Q=changed(Qg, (1, 1, 1), np.inf)),
                    dict(Q=changed(Qg, (0, 1, 1), -1e-6)),
                    dict(Q=changed(Qg, (1, 0, 1), 2.0 * np.sqrt(Qg[1, 0, 0] * Qg[1, 1, 1]))),
                    dict(Q=neg_det)]
        for kw in refusals:
            assert call(**kw) == EKF_ERR_ARG, kw
            assert b"ekf_predict_linear" in lib.ekf_last_error(f._h)
        for b in range(2):
            assert same(f.state(b), before[b])
        # what a trajectory that is not applied brings is not looked at; below Q's diagonal nothing is read
        assert call(pose=changed(pg, (0, 2), np.nan), Q=changed(Qg, (1, 2, 0), np.nan), apply=(0, 1)) == 0
        assert same(f.state(0), before[0])
        check_against_model(f.state(1), before[1], (pg[1], Fg[1], Qg[1]), "the valid call behind the refusals:")
        assert call(Q=np.zeros((2, 3, 3)), F=np.zeros((2, 3, 3))) == 0       # an all-zero Q and a singular F are legal
        mu, P = f.state(0)
        assert np.all(P[:3] == 0.0) and np.array_equal(P[3:, 3:], before[0][1][3:, 3:])
    with sd.EkfSlam(len(s[0])) as f:                         # EKF_FLAG_INTERNAL: the bounded wait of a single-launch step
        f.set_option("active_bound", 0)
        f.set_state_diag(s[0], s[1])
        f.step(s[2][0], s[3][0], s[4][0], s[5][0], s[6][0])
        f.sync()
        f.set_option("fused_step", 2)
        f.step(s[2][1], s[3][1], s[4][1], s[5][1], s[6][1])
        with pytest.raises(sd.EkfError, match="EKF_FLAG_INTERNAL"):
            f.predict_odometry([0.1, 0.0, 0.0], I3 * 1e-4, b=0)     # (reads the pose first: the read reports the flag)
        assert f.flags(0) & eb.EKF_FLAG_INTERNAL
