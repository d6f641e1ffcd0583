"""GPU: the hypothesis bank (ekf_hyp_*; EkfSlam.hypotheses -> HypothesisBank) -- K pose hypotheses localising on ONE frozen map.

The bank's promise is `localize`'s bits: every comparison of a hypothesis with a forked slot of a handle given the same calls is
np.array_equal on the pose mean, the pose block and P[0:3, :] (a slot's are read with mean() and covariance_block(0, 0, 3, n)).
The map copy is not exposed; it is judged through adopt, whose result is read raw (pbase / frozen_part) and, one SLAM step on,
against the dense model at the project's block bar of 1e-9.  The log-likelihood is compared with the same steps' innovation log
through evaluation.nis_consistency.  Small cases run with the source handle on the small-state path and on the general kernels
(both_paths), with the path asserted.

Measured on one MI355X (the figures this file prints with -s; profiles/hypotheses.txt keeps them): adopt + one SLAM step against
the dense model, largest piece corr_max 8.2e-16 (bar 1e-9); loglik against the innovation log, relative gap at most 2.2e-16
(bar 1e-9); the kidnapped robot: best = seed 41 with weight 0.999473, runner-up ratio 5.2e-4, pose NEES 0.092."""
import ctypes as C

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests import hypotheses_model as hm
from tests import localize_model as lm
from tests import streams
from tests.conftest import path_ran
from tests.gpu_support import pbase, sd  # noqa: F401
from tests.hyp_support import assert_same_bits, frozen_part, frozen_same
from tests.parity_blocks import assert_state_close, fmt_state

pytestmark = pytest.mark.gpu

TOL = 1e-9
INIT_VAR = 1e4
CFG = orc.EkfConfig()
SLAM_STEPS = 30
MMAX = 16


def wrap(a):
    return (a + np.pi) % (2 * np.pi) - np.pi


def observe(mean, lms, rng, noise=0.01):
    """Ranges and bearings of the landmarks `lms` as the mean itself sees them, plus a little noise."""
    lms = np.asarray(lms, dtype=np.int64)
    d = np.asarray(mean)[3:].reshape(-1, 2)[lms] - np.asarray(mean)[:2]
    zr = np.hypot(d[:, 0], d[:, 1]) + rng.normal(0.0, noise, len(lms))
    zb = wrap(np.arctan2(d[:, 1], d[:, 0]) - mean[2] + rng.normal(0.0, noise, len(lms)))
    return lms.astype(np.int32), zr, zb


def slot_pose_part(f, b):
    """(pose mean, P[0:3, :]) of trajectory b; the pose block comes mirrored from its stored upper triangle."""
    n = f.size(b)
    return f.mean(b)[:3].copy(), f.covariance_block(0, 0, 3, n, b)


def mapped_bank(sd, B, N=20, seed=11):
    """A handle of B slots whose slot 0 holds an N-landmark map from 30 SLAM steps (dense cross-covariances), flushed, and every
    other slot a fork of it."""
    _, lin, ang, idx, zr, zb, m = streams.wandering(N, B, SLAM_STEPS, 8, seed)
    worlds = [orc.synthetic_world(N, seed + 1 + t) for t in range(B)]
    f = sd.EkfSlam(3 + 2 * N, batch=B)
    for b in range(B):
        f.set_state_diag(worlds[b][2], worlds[b][3], b)
    f.stream_upload(lin, ang, idx, zr, zb, m)
    f.stream_run(0, SLAM_STEPS)
    f.flush()
    if B > 1:
        f.fork(0)
    return f


def bank_bits(bank):
    """Everything a refused call must leave alone, for every hypothesis."""
    pose, cov = bank.poses()
    return pose, cov, bank.loglik, bank.observed, bank.rejected, np.stack([bank.rows(k) for k in range(bank.count)])


def same_bank_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 1: bits against localize, m = 0 / 3 (one landmark twice) / 16, the gate on with a planted outlier -------------------------
def test_bits_against_localize(sd, both_paths):
    N, K = 20, 6
    rng = np.random.default_rng(5)
    with mapped_bank(sd, 3) as f:
        f.set_nis_gate(confidence=0.99)
        with f.hypotheses(3) as bank:
            for k in range(3):
                assert_same_bits(bank, k, f, k, f"seed, hypothesis {k}")
            for step in range(K):
                means = [f.mean(b) for b in range(3)]
                obs = [observe(means[0], [], rng),
                       observe(means[1], [(3 * step) % N, (3 * step + 7) % N, (3 * step) % N], rng),     # landmark 3 step twice
                       observe(means[2], (5 * step + np.arange(MMAX)) % N, rng)]
                if step == 2:
                    obs[2][1][5] += 5.0                                    # the planted outlier
                ang = 0.02 if step % 3 else 0.005
                f.localize(0.004, ang, [o[0] for o in obs], [o[1] for o in obs], [o[2] for o in obs])
                bank.step(0.004, ang, [o[0] for o in obs], [o[1] for o in obs], [o[2] for o in obs])
                for k in range(3):
                    assert_same_bits(bank, k, f, k, f"step {step}, hypothesis {k} (m = {(0, 3, 16)[k]})")
            counts = f.gate_counts()
            assert np.array_equal(bank.rejected, counts) and counts[2] >= 1 and counts[0] == 0, (bank.rejected, counts)
            assert np.array_equal(bank.observed, [0, 3 * K, MMAX * K])
            assert not bank.flags().any()
        assert path_ran(f, both_paths)


# ---- 2: shared observations = per-hypothesis rows carrying the same lists; a bank of 1 = its place in a bank of 65 --------------
def test_shared_lists_and_position_independence(sd, both_paths):
    N, K = 20, 65
    rng = np.random.default_rng(8)
    with mapped_bank(sd, 1) as f:
        mean = f.mean(0)
        seeds = sd.poses_on_circle(mean[3:5], 0.8, 0.3, K)
        cov = np.array([[0.02, 0.004, 0.0], [0.004, 0.03, 0.001], [0.0, 0.001, 0.01]])
        steps = [observe(mean, lms, rng) for lms in ([1, 5, 9, 5], (3 + np.arange(MMAX)) % N, [])]
        with f.hypotheses(K) as shared, f.hypotheses(K) as per:
            shared.set_nis_gate(confidence=0.9)
            per.set_nis_gate(confidence=0.9)
            shared.reset(seeds, cov)
            per.reset(seeds, cov)
            for o in steps:
                shared.step(0.004, 0.02, *o)
                per.step(np.full(K, 0.004), np.full(K, 0.02), [o[0]] * K, [o[1]] * K, [o[2]] * K)
            a, b = bank_bits(shared), bank_bits(per)
            assert same_bank_bits(a, b)
            assert np.isfinite(a[0]).all() and np.isfinite(a[2]).all() and a[4].sum() > 0 and len(np.unique(a[2])) > K // 2
            for k in (0, 37, 64):
                with f.hypotheses(1) as lone:
                    lone.set_nis_gate(confidence=0.9)
                    lone.reset(seeds[k], cov)
                    for o in steps:
                        lone.step(0.004, 0.02, *o)
                    c = bank_bits(lone)
                    assert all(np.array_equal(x[0], y[k]) for x, y in zip(c, a)), f"hypothesis {k} alone differs from its place in {K}"
        assert path_ran(f, both_paths)


# ---- 3: workgroup and layout edges ---------------------------------------------------------------------------------------------
def edge_case(sd, N, slam_lms, loc_lms, seed):
    """A 2-slot handle at N landmarks: slot 0 mapped by a few SLAM steps on `slam_lms` (observed from the mean), slot 1 its fork;
    then per entry of `loc_lms` one localisation step, hypothesis 0 / slot 0 on the list, hypothesis 1 / slot 1 on its reverse."""
    n = 3 + 2 * N
    rng = np.random.default_rng(seed)
    world = orc.synthetic_world(N, seed)
    with sd.EkfSlam(n, batch=2) as f:
        f.set_option("small_state", 0)
        for b in range(2):
            f.set_state_diag(world[2], world[3], b)
        for lms in slam_lms:
            o = observe(f.mean(0), lms, rng)
            f.step(0.004, 0.02, [o[0], []], [o[1], []], [o[2], []])
        f.flush()
        f.fork(0)
        slot_pose_part(f, 0)                                   # (a download mirrors the stored triangle: before the snapshot)
        frozen = frozen_part(sd, f, 0)
        with f.hypotheses(2) as bank:
            for i, lms in enumerate(loc_lms):
                o0, o1 = observe(f.mean(0), lms, rng), observe(f.mean(1), lms[::-1], rng)
                f.localize(0.004, 0.02, [o0[0], o1[0]], [o0[1], o1[1]], [o0[2], o1[2]])
                bank.step(0.004, 0.02, [o0[0], o1[0]], [o0[1], o1[1]], [o0[2], o1[2]])
                for k in range(2):
                    assert_same_bits(bank, k, f, k, f"N = {N}, step {i}, hypothesis {k}")
            rows = bank.rows(0)
        assert frozen_same(frozen_part(sd, f, 0), frozen)
        return rows


def test_row_group_edge(sd):
    """n = 263 crosses k_hyp_rows' 256-column group: landmark 126 sits on columns 255, 256.  The map knows landmarks up to 127
    (bound 259); landmark 129 (columns 261, 262) is observed for the first time in the second step, which raises the bound."""
    slam = [[0, 5, 125, 126, 127, 60], [1, 126, 127, 90, 30], [125, 127, 2, 64]]
    rows = edge_case(sd, 130, slam, [[5, 125, 126, 127], [126, 129, 3, 127]], 3)
    assert np.all(rows[:, 259:261] == 0.0) and np.all(rows[:, 261:263] != 0.0) and np.all(rows[:, 255:259] != 0.0)


def test_column_panel_layout(sd):
    """n = 4103 (ld > 4096: column panels): landmark 2046 sits on columns 4095, 4096."""
    slam = [[10, 2045, 2046, 2047, 2049], [2046, 2047, 11, 2049], [2045, 2046, 10]]
    rows = edge_case(sd, 2050, slam, [[10, 2046, 2047, 100], [2047, 2045, 2049, 2046]], 4)
    assert np.all(rows[:, 4093:4099] != 0.0)


# ---- 4: the map does not move: adopt ---------------------------------------------------------------------------------------------
def test_adopt(sd, both_paths):
    N = 20
    rng = np.random.default_rng(12)
    with mapped_bank(sd, 3) as f:
        start = f.state(0)
        with f.hypotheses(2) as bank:
            obs = []
            for step in range(2):
                o = [observe(start[0], [2, 9, 14], rng), observe(start[0], [(4 * step + j) % N for j in range(6)], rng)]
                bank.step(0.004, 0.02, [x[0] for x in o], [x[1] for x in o], [x[2] for x in o])
                obs.append(o[1])
            # a fresh fork of the source: adopted, its frozen part bit for bit what it was, its pose part the hypothesis's
            slot_pose_part(f, 1)                               # (a download mirrors the stored triangle: before the snapshot)
            frozen = frozen_part(sd, f, 1)
            bank.adopt(1, f, 1)
            assert frozen_same(frozen_part(sd, f, 1), frozen), "adopt moved the slot's map"
            assert_same_bits(bank, 1, f, 1, "adopted slot")
            # one landmark mean of slot 2 moved by one ulp: refused, the slot untouched
            mean2, cov2 = f.state(2)
            mean2[3 + 2 * 7] = np.nextafter(mean2[3 + 2 * 7], np.inf)
            f.set_state(mean2, cov2, 2)
            f.sync()
            before = pbase(sd, f, 2), f.mean(2)
            with pytest.raises(sd.EkfError, match="not the bank's map"):
                bank.adopt(0, f, 2)
            assert np.array_equal(pbase(sd, f, 2), before[0]) and np.array_equal(f.mean(2), before[1])
            # a following SLAM step on the adopted slot agrees with the dense model: literal_step twice, then the oracle's step
            model = start
            for o in obs:
                model = lm.literal_step(*model, 0.004, 0.02, *o, CFG)
            so = observe(model[0], [1, 6, 11, 16], rng)
            none = (np.zeros(0, dtype=np.int32), np.zeros(0), np.zeros(0))
            f.step(0.004, 0.02, [so[0], so[0], none[0]], [so[1], so[1], none[1]], [so[2], so[2], none[2]])
            model = orc.ekf_step_dense(*model, 0.004, 0.02, *so, CFG)
            err = assert_state_close((*f.state(1), f.tag_index(1), f.flags(1)), (model[0], 0.5 * (model[1] + model[1].T), f.tag_index(1)),
                                     INIT_VAR, tol=TOL, entry_tol=TOL, what="adopt + step: ")
            print(f"adopt + one SLAM step against the model: {fmt_state(err)}")
            # one more SLAM update has moved slot 0's map (the step above; flushed, so that pbase is what adopt finds): refused
            f.flush()
            f.sync()
            before = pbase(sd, f, 0), f.mean(0)
            with pytest.raises(sd.EkfError, match="not the bank's map"):
                bank.adopt(0, f, 0)
            assert np.array_equal(pbase(sd, f, 0), before[0]) and np.array_equal(f.mean(0), before[1])
        assert path_ran(f, both_paths)


# ---- 5: loglik ---------------------------------------------------------------------------------------------------------------
def test_loglik_against_the_innovation_log(sd, both_paths):
    from slam_duckietown_amd import evaluation as ev
    N, K = 20, 5
    rng = np.random.default_rng(21)
    with mapped_bank(sd, 3) as f:
        f.set_nis_gate(confidence=0.99)
        f.log_innovations(K)
        with f.hypotheses(3) as bank:
            for step in range(K):
                means = [f.mean(b) for b in range(3)]
                obs = [observe(means[0], [(2 * step + j) % N for j in range(4)], rng), observe(means[1], [step, step + 5], rng, noise=0.3),
                       observe(means[2], (7 * step + np.arange(MMAX)) % N, rng)]
                if step in (1, 3):
                    obs[0][1][2] += 6.0                                    # rejected: still part of the log-likelihood
                f.localize(0.004, 0.02, [o[0] for o in obs], [o[1] for o in obs], [o[2] for o in obs])
                bank.step(0.004, 0.02, [o[0] for o in obs], [o[1] for o in obs], [o[2] for o in obs])
            innov = f.innovations()
            want = ev.nis_consistency(innov).loglik
            got = bank.loglik
            gap = np.abs(got - want) / np.maximum(1.0, np.abs(want))
            print(f"loglik {got} against the innovation log {want}: relative gap {gap}")
            assert np.isfinite(got).all() and (gap <= 1e-9).all()
            rej = bank.rejected
            assert rej[0] >= 2 and np.array_equal(rej, f.gate_counts())
            assert np.array_equal(rej, (np.asarray(innov.rejected) == 1).sum(axis=(0, 2)))
            assert np.array_equal(bank.observed, [4 * K, 2 * K, MMAX * K])
            # the rejected observations' terms are in the sum: without them the sum is another number
            without = ev.nis_consistency(innov._replace(nis=np.where(np.asarray(innov.rejected) == 1, np.nan, innov.nis))).loglik
            assert abs(without[0] - got[0]) > 1.0
            # reset clears both
            bank.reset(f.mean(0)[:3], 0.01 * np.eye(3), k=0)
            assert bank.loglik[0] == 0.0 and bank.rejected[0] == 0 and bank.observed[0] == 0
            assert np.array_equal(bank.loglik[1:], got[1:]) and np.array_equal(bank.rejected[1:], rej[1:])
        assert path_ran(f, both_paths)


# ---- 6: reset against reset_pose + localize on a slot -------------------------------------------------------------------------
def test_reset_against_reset_pose(sd, both_paths):
    N = 20
    rng = np.random.default_rng(31)
    with mapped_bank(sd, 3) as f:
        mean = f.mean(0)
        poses = sd.poses_on_circle(mean[3 + 2 * 4:5 + 2 * 4], 0.9, -0.4, 3)
        cov = np.array([[0.03, 0.005, -0.002], [0.005, 0.02, 0.001], [-0.002, 0.001, 0.015]])
        with f.hypotheses(3) as bank:
            bank.step(0.004, 0.02, *observe(mean, [1, 2, 3], rng))         # a state, a log-likelihood and counters to clear
            f.reset_pose(poses, cov)
            bank.reset(poses, cov)
            assert np.array_equal(bank.loglik, np.zeros(3)) and not bank.observed.any()
            for k in range(3):
                assert_same_bits(bank, k, f, k, f"reset, hypothesis {k}")
                assert not bank.rows(k)[:, 3:].any()
            for step in range(2):
                obs = [observe(f.mean(b), [(5 * b + 3 * step + j) % N for j in range(5)], rng) for b in range(3)]
                f.localize(0.004, 0.02, [o[0] for o in obs], [o[1] for o in obs], [o[2] for o in obs])
                bank.step(0.004, 0.02, [o[0] for o in obs], [o[1] for o in obs], [o[2] for o in obs])
                for k in range(3):
                    assert_same_bits(bank, k, f, k, f"reset + step {step}, hypothesis {k}")
            # a range: hypothesis 1 alone
            before = bank_bits(bank)
            bank.reset(poses[1], cov, k=(1, 1))
            after = bank_bits(bank)
            assert all(np.array_equal(x[[0, 2]], y[[0, 2]]) for x, y in zip(before, after))
            assert np.array_equal(after[0][1], poses[1]) and np.array_equal(after[1][1], cov) and after[2][1] == 0.0
        assert path_ran(f, both_paths)


# ---- 7: the kidnapped robot, end to end ----------------------------------------------------------------------------------------
def test_kidnapped_robot(sd):
    """tests/hypotheses_model.py's scenario on the device; its CPU model holds NEES <= 8 and a runner-up weight <= 1e-3
    (tests/test_hypotheses_cpu.py), so what can fail here is the device."""
    from slam_duckietown_amd import evaluation as ev
    _, mean0, diag0, lin, ang, idx, zr, zb, m = hm.slam_stream()
    with sd.EkfSlam(3 + 2 * hm.N, batch=1, config=sd.EkfConfig(motion_sigma=hm.MOTION_SIGMA, meas_sigma=hm.MEAS_SIGMA)) as f:
        f.set_state_diag(mean0, diag0)
        f.stream_upload(lin, ang, idx, zr, zb, m)
        f.stream_run(0, hm.SLAM_STEPS)
        f.flush()
        case = hm.kidnapped_case(f.mean(0))
        with f.hypotheses(hm.K) as bank:
            bank.reset(case.seeds, hm.SEED_COV)
            for s in case.steps:
                bank.step(*s)
            res = ev.resolve_hypotheses(bank, confidence=0.99)
            pose, cov = bank.poses()
            nees = hm.pose_nees(pose[res.best], cov[res.best], case.truth)
            print(f"kidnapped robot: best {res.best} weight {res.weight:.6f}, runner-up {res.runner_up} ratio {res.ratio:.3e}, NEES {nees:.3f}")
            assert bank.best() == res.best
            assert hm.heading_gap(case.seeds[res.best, 2]) < case.spacing
            assert nees < hm.CHI2_3_999
            assert res.separated
            assert abs(bank.weights().sum() - 1.0) < 1e-12


# ---- 8: refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_hypothesis_alone(sd):
    N, K = 20, 4
    rng = np.random.default_rng(41)
    lib = sd.load_library()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    with mapped_bank(sd, 2) as f:
        mean = f.mean(0)
        bank = f.hypotheses(K)
        bank.step(0.004, 0.02, *observe(mean, [1, 8, 15], rng))
        before = bank_bits(bank)
        # m > EKF_MMAX at the C ABI (the binding would split the list)
        o = observe(mean, np.arange(MMAX + 1), rng)
        lin, ang, mm = np.array([0.004]), np.array([0.02]), np.array([MMAX + 1], dtype=np.int32)
        rc = lib.ekf_hyp_step(bank._h, lin.ctypes.data_as(dp), ang.ctypes.data_as(dp), 0, o[0].ctypes.data_as(ip), o[1].ctypes.data_as(dp),
                              o[2].ctypes.data_as(dp), mm.ctypes.data_as(ip), MMAX + 1, 0)
        assert rc == -1 and b"EKF_MMAX" in lib.ekf_hyp_last_error(bank._h)
        # an index outside the map, in a step and in an update, shared and per hypothesis
        with pytest.raises(sd.EkfError, match="outside the map"):
            bank.step(0.004, 0.02, [3, N], [1.0, 1.0], [0.0, 0.0])
        with pytest.raises(sd.EkfError, match="outside the map"):
            bank.update([[1], [2], [3], [-1]], [[1.0]] * K, [[0.0]] * K)
        # k out of range
        with pytest.raises(sd.EkfError, match="outside the bank"):
            bank.rows(K)
        with pytest.raises(sd.EkfError, match="outside the bank"):
            bank.reset(np.zeros(3), np.eye(3), k=K)
        with pytest.raises(sd.EkfError, match="outside the bank"):
            bank.reset(np.zeros(3), np.eye(3), k=(K - 1, 2))
        with pytest.raises(sd.EkfError, match="outside the bank"):
            bank.adopt(K, f, 1)
        with pytest.raises(sd.EkfError, match="outside the bank"):
            bank.adopt(-1, f, 1)
        with pytest.raises(sd.EkfError):
            bank.adopt(0, f, 2)                                            # a slot the handle does not have
        with pytest.raises(sd.EkfError, match="non-finite"):
            bank.reset(np.array([0.0, np.nan, 0.0]), np.eye(3))
        assert lib.ekf_hyp_set_nis_gate(bank._h, -1.0) == -1 and b"threshold" in lib.ekf_hyp_last_error(bank._h)
        assert same_bank_bits(bank_bits(bank), before)
        # a bank used after close()
        bank.close()
        for call in (lambda: bank.step(0.004, 0.02, [1], [1.0], [0.0]), bank.poses, lambda: bank.rows(0), lambda: bank.adopt(0, f, 1)):
            with pytest.raises(sd.EkfError, match="closed"):
                call()
        bank.close()
