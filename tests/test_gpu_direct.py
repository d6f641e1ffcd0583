"""GPU: direct measurements (ekf_update_direct, EkfSlam.update_direct / fix_pose / anchor_landmarks) against the NumPy
reference tests/direct_model.py applied to state() taken just before the call.

Tolerance: TIGHT = 1e-9, held twice.  As a relative Frobenius norm over the whole mean and the whole covariance
(test_gpu_joint.py's bound against a dense reference) -- a metric the never-observed landmarks at variance 1e4 dominate: a pose
block 0.1 % off moves it by 5e-11 .. 5e-10 (tests/test_update_blocks_cpu.py pins that).  And block by block
(parity_blocks.assert_update_close, against the Joseph form of the reference): pose block, pose-landmark cross rows, landmark
block, the correlation-scaled largest entry and the means of everything that was active before the call, each on its own scale
at TIGHT; a never-observed landmark the call fixes: its own block to 32 eps landmark_init_var, its mean to 1e-9, its cross
terms exact zeros; every other never-observed landmark bit for bit; P exactly symmetric.  tests/test_direct_cpu.py and
tests/test_update_blocks_cpu.py show that on these very inputs the simple, Joseph and sequential forms of the reference agree to
1e-11, on the whole matrix and on every such piece, so 1e-9 is a statement about the device code and not about the conditioning
of the inputs."""
import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests import direct_model as dm
from tests import parity_blocks as pb
from tests import update_cases as uc
from tests.conftest import path_ran
from tests.gpu_support import bank, sd  # noqa: F401

pytestmark = pytest.mark.gpu

TIGHT = 1e-9
EKF_ERR_ARG, EKF_ERR_STATE = -1, -3


def check_against_model(f, b, before, fix, res, gate=np.inf):
    t, z, R = fix
    wm, wP, nis, dof, ok = dm.direct_update(before[0], before[1], t, z, R, gate)
    mu, P = f.state(b)
    assert np.array_equal(P, P.T)
    assert bool(res.applied[b]) == ok and res.dof[b] == dof
    if dof:
        assert res.nis[b] == pytest.approx(nis, rel=1e-9)
    e_mu, e_P = orc.rel_fro(mu, wm), orc.rel_fro(P, wP)
    print(f"trajectory {b}: D = {dof} nis {res.nis[b]:.6g} rel_fro mean {e_mu:.2e} cov {e_P:.2e}")
    assert e_mu <= TIGHT and e_P <= TIGHT, (b, e_mu, e_P)
    # block by block against the Joseph form (on the closed system the call touches: affordable at N = 2060 too)
    want = uc.direct_reference(before, fix, gate)
    err = pb.assert_update_close((mu, P), want, before, [x for x in t if x >= 0], f.config.landmark_init_var, TIGHT,
                                 what=f"trajectory {b}: ")
    print(f"trajectory {b}: {pb.fmt_update(err)}")
    return mu, P


def test_small_state_on_both_paths(sd, both_paths):
    """N = 20, 30 steps (landmarks 16 .. 19 never observed): a pose fix plus two landmark fixes, one of them on a
    never-observed landmark, on the small-state path and on the general kernels; one more step."""
    s, t, z, R = dm.case_small()
    with bank(sd, [s], steps=dm.SMALL_STEPS) as f:
        assert path_ran(f, both_paths)
        before = f.state(0)
        res = f.update_direct(t, z, R)
        mu, P = check_against_model(f, 0, before, (t, z, R), res)
        assert res.applied[0] and res.dof[0] == 7
        f.step(s[2][dm.SMALL_STEPS], s[3][dm.SMALL_STEPS], s[4][dm.SMALL_STEPS], s[5][dm.SMALL_STEPS], s[6][dm.SMALL_STEPS])
        want = orc.ekf_step_dense(mu, P, s[2][dm.SMALL_STEPS], s[3][dm.SMALL_STEPS], s[4][dm.SMALL_STEPS], s[5][dm.SMALL_STEPS], s[6][dm.SMALL_STEPS], orc.EkfConfig())
        got = f.state(0)
        assert orc.rel_fro(got[0], want[0]) <= TIGHT and orc.rel_fro(got[1], want[1]) <= TIGHT
        err = pb.assert_filter_close(got[0], got[1], want[0], want[1], pb.active_of(want[1], f.config.landmark_init_var),
                                     mean0=mu, diag0=np.diag(P), tol=TIGHT, what="the step behind it: ")
        print("the step behind it:", pb.fmt(err))
        assert path_ran(f, both_paths)


def test_bank_with_ranks_pending_gate_and_untouched_rest(sd):
    """N = 150 x 4 on the general kernels, ranks pending before the call, sizes differing per trajectory: pose only; position
    plus 15 landmarks (D = 32; two never observed, beyond the active bound); nothing; a pose fix 10 sigma off under the
    chi-square gate of 3 degrees of freedom at 0.99."""
    from scipy.stats import chi2
    streams, fixes = dm.case_bank()
    lib = sd.load_library()

    def prepare(f):
        f.set_option("fused_cadence", 0)
        f.log_innovations(64)
        f.log_poses(64)
        f.set_nis_gate(confidence=0.999999)
        f.set_noise(motion_sigma=[0.1, 0.11, 0.1, 0.09])
        f.stream_run(0, 30)
        f.remove_landmarks([149], b=0)                       # sizes differ: trajectory 0 has 149 landmarks, 3 has 148
        f.remove_landmarks([148, 149], b=3)
        f.set_tag_index({7: 0, 9: 1, 300: 2}, 1)
        f.flush()
        f.step([s[2][0] for s in streams], [s[3][0] for s in streams], [s[4][0][:2] for s in streams],
               [s[5][0][:2] for s in streams], [s[6][0][:2] for s in streams])       # 4 ranks are pending from here on

    def counters(f):
        import ctypes as C
        logged = C.c_longlong()
        assert lib.ekf_innovation_steps(f._h, C.byref(logged)) == 0
        return (f.gate_counts().copy(), int(logged.value), f.pose_steps, [np.array(x).copy() for x in f.noise()],
                [f.size(b) for b in range(4)], f.tag_index(1))

    # the flushed pre-call state comes from a twin driven through the identical sequence: the bank under test is neither
    # flushed nor downloaded between its last step() and the call
    with bank(sd, streams, run=False) as twin:
        prepare(twin)
        before = [twin.state(b) for b in range(4)]
    with bank(sd, streams, run=False) as f:
        prepare(f)
        f.profile_enable(True)                               # (synchronises; applies nothing)
        c0 = counters(f)
        assert f.profile_passes() == 0
        gate = [np.inf, np.inf, np.inf, chi2.ppf(0.99, 3)]
        res = f.update_direct([x[0] for x in fixes], [x[1] for x in fixes], [x[2] for x in fixes], gate=gate)
        assert f.profile_passes() == 2                       # the pass of what was pending, then the pass of the fixes
        assert list(res.applied) == [True, True, False, False] and list(res.dof) == [3, 32, 0, 3]
        assert res.nis[3] > gate[3]
        for b in range(4):
            check_against_model(f, b, before[b], fixes[b], res, gate[b])
        for b in (2, 3):
            after = f.state(b)
            assert np.array_equal(after[0], before[b][0]) and np.array_equal(after[1], before[b][1])
        c1 = counters(f)
        assert np.array_equal(c0[0], c1[0]) and c0[1:3] == c1[1:3] and c0[4:] == c1[4:]
        assert all(np.array_equal(a, b) for a, b in zip(c0[3], c1[3]))
        # the never-observed landmarks of trajectory 1: R (R + v)^-1 v in their own block, nothing else of their rows moved
        v = f.config.landmark_init_var
        t, z, R = fixes[1]
        mu1, P1 = f.state(1)
        for l in (130, 149):
            j = t.index(l)
            a = 3 + 2 * l
            Rl = R[j][:2, :2]
            want = Rl @ np.linalg.solve(Rl + v * np.eye(2), v * np.eye(2))
            assert np.abs(P1[a:a + 2, a:a + 2] - want).max() <= 32 * np.finfo(float).eps * v
            wm = before[1][0][a:a + 2] + v * np.linalg.solve(Rl + v * np.eye(2), z[j][:2] - before[1][0][a:a + 2])
            assert np.abs(mu1[a:a + 2] - wm).max() <= 1e-9 * max(1.0, np.abs(wm).max())
        never = [l for l in range(120, 150) if l not in (130, 149)]
        rows = np.array([3 + 2 * l + d for l in never for d in range(2)])
        assert np.array_equal(P1[rows, :], before[1][1][rows, :]) and np.array_equal(mu1[rows], before[1][0][rows])
        off = np.setdiff1d(np.arange(P1.shape[0]), [263, 264])
        assert np.array_equal(P1[np.ix_([263, 264], off)], before[1][1][np.ix_([263, 264], off)])


def test_large_state_across_the_column_panel(sd):
    """N = 2060 (n = 4123: two column panels): a pose fix, landmark 0, landmark 2059 (observed) and the never-observed 1000.

    |P|_F is 6e5 here, so the whole-matrix 1e-9 allows 6e-4 absolutely -- the size of the variances the update is about.  What
    judges the update is check_against_model's block-wise part: the pose and the 321 observed landmarks piece by piece at
    TIGHT, landmark 1000's block and mean (fixed first: its cross terms stay exact zeros), the other 1738 bit for bit."""
    s, t = dm.case_large()
    n = len(s[0])
    with bank(sd, [s]) as f:
        mu0 = f.mean(0)
        d = s[0][3 + 2 * 2059:5 + 2 * 2059] - mu0[:2]
        f.step(0.0, 0.0, [2059], [float(np.hypot(*d)) + 0.01], [float(orc.wrap_pi(np.arctan2(d[1], d[0]) - mu0[2])) + 0.01])
        before = f.state(0)
        rng = np.random.default_rng(5)
        z, R = dm.make_fixes(rng, before[0], before[1], t[:3])
        z1, R1 = dm.make_fixes(rng, before[0], np.diag(np.full(n, 0.01)), [1000])      # (a survey within decimetres of the prior mean)
        z, R = z + z1, R + R1
        res = f.update_direct(t, z, R)
        assert res.applied[0] and res.dof[0] == 9
        mu, P = check_against_model(f, 0, before, (t, z, R), res)
        v, a, Rl = f.config.landmark_init_var, 3 + 2 * 1000, R[3][:2, :2]
        want = Rl @ np.linalg.solve(Rl + v * np.eye(2), v * np.eye(2))
        # (the pass forms v - v^2 / (v + R): the cancellation leaves eps * v absolutely)
        assert np.abs(P[a:a + 2, a:a + 2] - want).max() <= 32 * np.finfo(float).eps * v
        wm = before[0][a:a + 2] + v * np.linalg.solve(Rl + v * np.eye(2), z[3][:2] - before[0][a:a + 2])
        assert np.abs(mu[a:a + 2] - wm).max() <= 1e-9 * max(1.0, np.abs(wm).max())
        off = np.setdiff1d(np.arange(n), [a, a + 1])
        assert np.array_equal(P[np.ix_([a, a + 1], off)], before[1][np.ix_([a, a + 1], off)])
        # everything of the other never-observed landmarks is bit-unchanged
        rows = np.array([3 + 2 * l + dd for l in range(320, 2059) if l != 1000 for dd in range(2)])
        assert np.array_equal(P[rows, :], before[1][rows, :]) and np.array_equal(mu[rows], before[0][rows])


def test_joint_equals_sequential(sd):
    s, t, z, R = dm.case_three()
    with bank(sd, [s, s]) as f:
        f.update_direct([t, []], [z, []], [R, []])
        for j in range(3):
            f.update_direct([[], [t[j]]], [[], [z[j]]], [[], [R[j]]])
        a, b = f.state(0), f.state(1)
        e = orc.rel_fro(a[0], b[0]), orc.rel_fro(a[1], b[1])
        print("joint against sequential: rel_fro mean %.2e cov %.2e" % e)
        assert max(e) <= TIGHT


@pytest.mark.parametrize("step_between", [False, True])
def test_life_goes_on(sd, step_between):
    """A bank of 2 at N = 150: 30 steps, a direct update, then 40 further steps of the same uploaded stream as fused cadences
    (with a step() in between in the second case), against the dense oracle continued from the model's post-update state."""
    streams = [orc.synthetic_stream(150, 70, 4, 60 + b) for b in range(2)]
    rng = np.random.default_rng(9)
    with bank(sd, streams, steps=30) as f:
        before = [f.state(b) for b in range(2)]
        fixes = []
        for b in range(2):
            t = [dm.POSE, 10 + b] if b == 0 else [dm.POSITION, 40]
            fixes.append((t,) + dm.make_fixes(rng, before[b][0], before[b][1], t))
        res = f.update_direct([x[0] for x in fixes], [x[1] for x in fixes], [x[2] for x in fixes])
        assert res.applied.all()
        c0 = f.cadence_counters()
        first = 30
        if step_between:
            f.step([s[2][30] for s in streams], [s[3][30] for s in streams], [s[4][30] for s in streams],
                   [s[5][30] for s in streams], [s[6][30] for s in streams])
            first = 31
        f.stream_run(first, 70 - first)
        f.sync()
        c1 = f.cadence_counters()
        print("cadences / steps before", c0, "after", c1)
        assert c1[0] > c0[0]
        if not step_between:
            assert c1[1] - c0[1] >= 40                       # every step of the piece ran inside a fused cadence
        else:
            # the step() leaves 8 ranks pending and a cadence only forms where nothing is pending: the per-step kernels run
            # until the pass is due -- 8 (s + 1) > 80 ranks, behind the step() and 9 stream steps -- and the other 30 of the
            # 39 steps run as fused cadences
            assert c1[1] - c0[1] >= 30
        cfg = orc.EkfConfig()
        for b, s in enumerate(streams):
            om, oP, _, _, _ = dm.direct_update(before[b][0], before[b][1], *fixes[b])
            for k in range(30, 70):
                om, oP = orc.ekf_step_dense(om, oP, s[2][k], s[3][k], s[4][k], s[5][k], s[6][k], cfg)
            mu, P = f.state(b)
            e = orc.rel_fro(mu, om), orc.rel_fro(P, oP)
            print("trajectory %d: rel_fro mean %.2e cov %.2e" % ((b,) + e))
            assert max(e) <= TIGHT
            err = pb.assert_filter_close(mu, P, om, oP, pb.active_of(oP, f.config.landmark_init_var), tol=TIGHT,
                                         what=f"trajectory {b}: ")
            print("trajectory %d: %s" % (b, pb.fmt(err)))


def test_two_anchors_fix_the_gauge(sd):
    s, survey = dm.case_gauge()
    A = list(dm.GAUGE_ANCHORS)
    with bank(sd, [s, s], config=sd.EkfConfig(**dm.gauge_config())) as f:
        f.fork(0, 1)
        res = f.anchor_landmarks(A, survey[A], np.eye(2) * dm.GAUGE_SIGMA ** 2, b=1)
        assert list(res.applied) == [False, True] and list(res.dof) == [0, 4]
        obs = dm.observed(s)
        inside = []
        for b in range(2):
            _, blocks = f.marginals(b)
            inside.append(dm.within_sigmas(f.mean(b), blocks, survey, obs))
        assert inside[1].all() and not inside[0].any()


def test_abi_refusals_leave_the_state_alone(sd):
    import ctypes as C
    from slam_duckietown_amd import ekf_bindings as eb
    s = orc.synthetic_stream(40, 6, 4, 3)
    lib = sd.load_library()
    with bank(sd, [s, s]) as f:
        before = [f.state(b) for b in range(2)]
        Rg = np.zeros((2, 4, 3, 3))
        Rg[:] = np.diag([0.01, 0.01, 0.001])
        zg = np.zeros((2, 4, 3))
        for b in range(2):
            zg[b, :, :] = before[b][0][:3]

        def call(b0=0, count=2, target=((-1, 2, 5, 0), (-2, 1, 0, 0)), z=zg, R=Rg, m=(3, 2), stride=4, gate=None, null=None):
            T, mm = eb._i32(np.array(target)), eb._i32(np.array(m))
            z, R = eb._f64(z), eb._f64(R)
            g = eb._f64(np.array(gate, dtype=float)) if gate is not None else None
            args = dict(target=eb._p(T, eb._ip), z=eb._p(z), R=eb._p(R), m=eb._p(mm, eb._ip))
            if null:
                args[null] = None
            return lib.ekf_update_direct(f._h, b0, count, args["target"], args["z"], args["R"], args["m"], stride,
                                         eb._p(g) if g is not None else None, None, None, None)

        bad_z, bad_R, npd = zg.copy(), Rg.copy(), Rg.copy()
        bad_z[1, 1, 0] = np.nan
        bad_R[0, 0, 0, 2] = np.inf
        npd[0, 1, :2, :2] = [[0.01, 0.02], [0.02, 0.01]]
        npd3 = Rg.copy()
        npd3[0, 0] = [[1.0, 0.0, 2.0], [0.0, 1.0, 0.0], [2.0, 0.0, 1.0]]
        refusals = [dict(b0=1, count=2), dict(b0=-1), dict(count=0), dict(stride=0), dict(stride=17), dict(m=(5, 2)), dict(m=(3, -1)),
                    dict(target=((-1, 2, 40, 0), (-2, 1, 0, 0))), dict(target=((-1, 2, -3, 0), (-2, 1, 0, 0))),
                    dict(target=((-1, 2, 2, 0), (-2, 1, 0, 0))), dict(target=((-1, 2, -2, 0), (-2, 1, 0, 0))),
                    dict(target=((-1, 2, -1, 0), (-2, 1, 0, 0))), dict(z=bad_z), dict(R=bad_R), dict(R=npd), dict(R=npd3),
                    dict(gate=(np.nan, 1.0)), dict(gate=(1.0, 0.0)), dict(gate=(-1.0, 1.0)),
                    dict(null="target"), dict(null="z"), dict(null="R"), dict(null="m")]
        for kw in refusals:
            assert call(**kw) == EKF_ERR_ARG, kw
            assert b"ekf_update_direct" in lib.ekf_last_error(f._h)
        for b in range(2):
            after = f.state(b)
            assert np.array_equal(after[0], before[b][0]) and np.array_equal(after[1], before[b][1])
        assert call(gate=(np.inf, 50.0)) == 0                # the handle is usable
        assert orc.rel_fro(f.state(0)[1], before[0][1]) > 1e-6
    with sd.EkfSlam(len(s[0])) as f:                         # EKF_FLAG_INTERNAL: the bounded wait of a single-launch step
        f.set_option("active_bound", 0)
        f.set_state_diag(s[0], s[1])
        f.step(s[2][0], s[3][0], s[4][0], s[5][0], s[6][0])
        f.sync()
        f.set_option("fused_step", 2)
        f.step(s[2][1], s[3][1], s[4][1], s[5][1], s[6][1])
        with pytest.raises(sd.EkfError, match="EKF_FLAG_INTERNAL"):
            f.fix_pose([0.0, 0.0, 0.0], np.eye(3) * 0.01)
        assert f.flags(0) & eb.EKF_FLAG_INTERNAL
