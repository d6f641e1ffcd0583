"""GPU: the hypothesis bank's weights, systematic resampling and split on the device (ekf_hypotheses_weigh /
ekf_hypotheses_resample; HypothesisBank.ess / evidence / resample / resample_if).

The plan is judged against tests/resample_model.py with np.array_equal: tests/test_hyp_resample_cpu.py holds, for every case
here, that K C_k - u keeps 1e-7 from the nearest integer, 50 times what another summation order can move it.  A copy is judged
against forks of a handle's slots bit for bit, a split against keep * the values downloaded before it (one multiply: bit for
bit) and the model's pose at 1e-9.  Small cases run with the source handle on the small-state path and on the general kernels.

Measured on one MI355X (the figures this file prints with -s; profiles/hyp_resample.txt keeps them): ess and logmean against the
model, largest relative gap 4.4e-16 (K = 1025; bar 1e-9); split poses against the model 1.1e-16 (bar 1e-9); the kidnapped robot:
one resampling, behind step 0, final poses within 1.8e-15 of the model fleet's, mixture Mahalanobis^2 0.057."""
import ctypes as C

import numpy as np
import pytest

from tests import hyp_support as hs
from tests import hypotheses_model as hm
from tests import resample_model as rm
from tests.conftest import path_ran
from tests.gpu_support import sd  # noqa: F401

pytestmark = pytest.mark.gpu

TOL = 1e-9


def rel(a, b):
    return abs(a - b) / max(1.0, abs(b)) if np.isfinite(b) else (0.0 if a == b else np.inf)


def shaped_bank(f, K, d, flagged):
    """K hypotheses on f's slot 0, their log-likelihoods shaped by one update each (tests/resample_model.py: plan_cases)."""
    bank = f.hypotheses(K)
    idx, r0, b0 = hs.observe(f.mean(0), [rm.PLAN_LM])
    ranges = r0[0] + np.asarray(d, dtype=np.float64)
    ranges[list(flagged)] = np.nan
    bank.update([idx] * K, [[r] for r in ranges], [[b0[0]]] * K)
    return bank


SPREAD = 1.1 * np.array([0.0, 0.5, 1.0, 1.5, 2.0, 0.3, 2.5, 4.0])    # range offsets (m) that spread eight hypotheses' weights


def pick_u(before, singles):
    """The first offset of a fixed grid whose plan (the model's, from the device's own log-likelihoods) copies something --
    a dead slot and an ancestor with two or more offspring -- and, with `singles`, also leaves a single-offspring ancestor; the
    margin holds for it."""
    for u in np.arange(0.05, 1.0, 0.1):
        anc, off, _ = rm.plan(before.loglik, before.flags, u)
        if (off == 0).any() and (off >= 2).any() and ((off == 1).any() or not singles) and rm.margin(before.loglik, before.flags, u) >= rm.MARGIN:
            return float(u)
    raise AssertionError(f"no offset of the grid gives the case: weights {rm.weigh(before.loglik, before.flags).w}")


# ---- 1: the plan ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", rm.PLAN_KS)
def test_plan_against_the_model(sd, both_paths, K):
    worst = 0.0
    with hs.mapped_handle(sd, 1) as f:
        for name, _, d, u, flagged, dead in rm.plan_cases(K):
            what = f"K = {K}, {name}"
            with shaped_bank(f, K, d, flagged) as bank:
                before = hs.snapshot(bank)
                assert (before.flags[list(flagged)] & rm.NONFINITE).all() and not np.delete(before.flags, list(flagged)).any(), what
                anc, off, W = rm.plan(before.loglik, before.flags, u)
                assert rm.margin(before.loglik, before.flags, u) >= rm.MARGIN, what
                got = bank.ess(), bank.evidence(), bank.live()
                res = bank.resample(u=u)
                gaps = [rel(got[0], W.ess), rel(got[1], W.logmean), rel(res.ess, W.ess), rel(res.logmean, W.logmean)]
                worst = max(worst, *gaps)
                print(f"{what}: ess {got[0]:.6g} (model {W.ess:.6g}), logmean {got[1]:.12g}, live {got[2]}, largest gap {max(gaps):.2e}")
                assert max(gaps) <= TOL and got[2] == W.live, what
                assert np.array_equal(res.ancestors, anc) and np.array_equal(res.offspring, off), what
                after = hs.snapshot(bank)
                assert rm.judge(after, before, u, 0.0, None, res.logmean) is None, f"{what}: {rm.judge(after, before, u, 0.0, None, res.logmean)}"
                if W.live == 0 or name.startswith("uniform"):
                    assert hs.same_snapshot(after, before), f"{what}: the identity changed the bank"
                    assert np.array_equal(res.ancestors, np.arange(K)) and (res.offspring == 1).all()
                if W.live == 0:
                    assert res.ess == 0.0 and res.logmean == -np.inf and got[2] == 0
                if name == "one-hot":
                    assert (res.ancestors == K // 3).all() and res.offspring[K // 3] == K
                if W.live:
                    assert not res.offspring[list(dead) + list(flagged)].any(), what
        assert path_ran(f, both_paths)
    print(f"K = {K}: ess / logmean against the model, largest relative gap {worst:.2e} (bar {TOL:g})")


# ---- 2: the copy, bit for bit against forks -------------------------------------------------------------------------------------
def copy_against_forks(sd, f, N, rng):
    K = f.batch
    with f.hypotheses(K) as bank:
        def step(i):
            obs = [hs.observe(f.mean(b), [(3 * b + 5 * i + j) % N for j in range(3)], rng) for b in range(K)]
            if i == 0:
                for b in range(K):
                    obs[b][1][0] += SPREAD[b]                                 # (what makes the weights uneven)
            args = (0.004, 0.02, [o[0] for o in obs], [o[1] for o in obs], [o[2] for o in obs])
            f.localize(*args)
            bank.step(*args)
        for i in range(2):
            step(i)
        for k in range(K):
            hs.assert_same_bits(bank, k, f, k, f"before the resampling, hypothesis {k}")
        before = hs.snapshot(bank)
        u = pick_u(before, False)
        res = bank.resample(u=u)
        assert (res.offspring == 0).any() and (res.offspring >= 2).any(), res.offspring       # (the case copies something)
        assert np.array_equal(res.ancestors, rm.plan(before.loglik, before.flags, u)[0])
        dead = np.nonzero(res.ancestors != np.arange(K))[0]
        f.copy_from(f, res.ancestors[dead], dead)
        after = hs.snapshot(bank)
        assert (after.loglik == res.logmean).all()
        assert np.array_equal(after.n_obs, before.n_obs[res.ancestors]) and np.array_equal(bank.observed, after.n_obs)
        assert np.array_equal(bank.rejected, before.n_rej[res.ancestors])
        for i in range(2, 5):
            step(i)
        for k in range(K):
            hs.assert_same_bits(bank, k, f, k, f"three steps behind the resampling, hypothesis {k} (ancestor {res.ancestors[k]})")


def test_copy_against_forks(sd, both_paths):
    with hs.mapped_handle(sd, 8) as f:
        copy_against_forks(sd, f, 20, np.random.default_rng(3))
        assert path_ran(f, both_paths)


@pytest.mark.parametrize("N, slam", [(130, [[0, 5, 125, 126, 127, 60], [1, 126, 127, 90, 30], [125, 127, 2, 64, 129]]),
                                     (2050, [[10, 2045, 2046, 2047, 2049], [2046, 2047, 11, 2049], [2045, 2046, 10, 0, 1, 2]])])
def test_copy_against_forks_at_the_layout_edges(sd, N, slam):
    """n = 263: ldx = 512, exactly one column group of k_hyp_copy; n = 4103: ldx = 4160, nine groups, the last of 64 columns, and
    the handle's column panels on the forks' side."""
    with hs.sparse_handle(sd, 8, N, slam, 4) as f:
        copy_against_forks(sd, f, 3, np.random.default_rng(5))


# ---- 3: the split --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [20, 2050])
def test_split(sd, N):
    K, s = 8, 0.6
    rng = np.random.default_rng(9)
    z = rng.standard_normal((K, 3))
    slam = [[10, 2045, 2046, 2047, 2049], [2046, 2047, 11, 2049], [2045, 2046, 10, 0, 1, 2]]
    with (hs.mapped_handle(sd, 1) if N == 20 else hs.sparse_handle(sd, 1, N, slam, 4)) as f, f.hypotheses(K) as bank:
        mean = f.mean(0)
        # hypotheses 0 .. 2 with a zero variance: all zero, x alone, heading alone
        cov = np.array([[0.02, 0.004, 0.0], [0.004, 0.03, 0.001], [0.0, 0.001, 0.01]])
        bank.reset(mean[:3], np.zeros((3, 3)), k=0)
        bank.reset(mean[:3], np.diag([0.0, 0.02, 0.01]), k=1)
        bank.reset(mean[:3], np.diag([0.02, 0.03, 0.0]), k=2)
        bank.reset(mean[:3] + [0.01, -0.01, 0.002], cov, k=3)
        lms = [0, 1, 2] if N > 20 else [0, 7, 13]
        obs = [hs.observe(mean, lms, rng) for k in range(K)]
        for k in range(K):
            obs[k][1][0] += SPREAD[(k + 3) % K]                               # (uneven weights; the zero-variance ones among the heavy)
        bank.update([o[0] for o in obs], [o[1] for o in obs], [o[2] for o in obs])
        before = hs.snapshot(bank)
        u = pick_u(before, True)
        res = bank.resample(u=u, split=s, z=z)
        after = hs.snapshot(bank)
        anc, off, _ = rm.plan(before.loglik, before.flags, u)
        assert np.array_equal(res.ancestors, anc) and np.array_equal(res.offspring, off)
        moved = off[anc] >= 2
        assert moved.any() and not moved.all(), off                           # (both kinds of slot are there)
        keep = 1.0 - s * s
        assert np.array_equal(after.blk[moved], keep * before.blk[anc][moved]) and np.array_equal(after.rows[moved], keep * before.rows[anc][moved])
        assert np.array_equal(after.blk[~moved], before.blk[anc][~moved]) and np.array_equal(after.rows[~moved], before.rows[anc][~moved])
        assert np.array_equal(after.pose[~moved], before.pose[anc][~moved])
        want, _ = rm.resample(before, u, s, z)
        gap = np.abs(after.pose - want.pose).max()
        print(f"N = {N}: split poses against the model, largest gap {gap:.2e} (bar {TOL:g}); offspring {off}")
        assert gap <= TOL and rm.judge(after, before, u, s, z, res.logmean) is None, rm.judge(after, before, u, s, z, res.logmean)
        assert np.abs(after.pose[moved] - before.pose[anc][moved]).max() > 1e-4 or not before.blk[anc][moved].any()
        # the bank still steps
        bank.step(0.004, 0.02, *hs.observe(mean, lms, rng))
        pose, blk = bank.poses()
        assert np.isfinite(pose).all() and np.isfinite(blk).all() and np.isfinite(bank.loglik).all() and not bank.flags().any()
        for k in range(K):
            assert np.linalg.eigvalsh(blk[k]).min() >= -1e-12 * max(1.0, np.abs(blk[k]).max()), (k, blk[k])


def test_split_moves_a_zero_variance_block_nowhere(sd):
    """A bank whose every pose block is zero, one hypothesis taking every offspring: the factor's columns are all zeroed, so the
    split moves no pose and keeps zeros."""
    K = 4
    with hs.mapped_handle(sd, 1) as f, f.hypotheses(K) as bank:
        bank.reset(f.mean(0)[:3], np.zeros((3, 3)))
        idx, r0, b0 = hs.observe(f.mean(0), [rm.PLAN_LM])
        bank.update([idx] * K, [[r0[0] + d] for d in (rm.DEAD, 0.0, rm.DEAD, rm.DEAD)], [[b0[0]]] * K)
        before = hs.snapshot(bank)
        res = bank.resample(u=0.5, split=0.5, z=np.ones((K, 3)))
        after = hs.snapshot(bank)
        assert (res.ancestors == 1).all() and not before.blk.any()
        assert rm.judge(after, before, 0.5, 0.5, np.ones((K, 3)), res.logmean) is None
        assert np.array_equal(after.pose, np.repeat(before.pose[1:2], K, axis=0)) and not after.blk.any() and not after.rows.any()


# ---- 4: the asynchronous form ----------------------------------------------------------------------------------------------------
def test_asynchronous_form_gives_the_blocking_form_s_bits(sd):
    K, u, s = 65, 0.37, 0.4
    d = rm.plan_cases(K)[0][2]
    z = np.random.default_rng(2).standard_normal((K, 3))
    lib = sd.load_library()
    dp = C.POINTER(C.c_double)
    with hs.mapped_handle(sd, 1) as f, shaped_bank(f, K, d, ()) as a, shaped_bank(f, K, d, ()) as b:
        obs = hs.observe(f.mean(0), [2, 9, 14])
        a.resample(u=u, split=s, z=z)
        assert lib.ekf_hypotheses_weigh(b._h, None, None, None) == 0
        assert lib.ekf_hypotheses_resample(b._h, u, s, z.ctypes.data_as(dp), None, None, None, None) == 0
        z[:] = 0.0                                                             # (the draws were staged by the call)
        a.step(0.004, 0.02, *obs)
        b.step(0.004, 0.02, *obs)
        assert hs.same_snapshot(hs.snapshot(a), hs.snapshot(b))
        assert len(np.unique(hs.snapshot(a).pose[:, 0])) > K // 4


# ---- 5: refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_hypothesis_alone(sd):
    K = 5
    d = rm.plan_cases(65)[0][2][:K]
    z = np.random.default_rng(1).standard_normal((K, 3))
    lib = sd.load_library()
    dp = C.POINTER(C.c_double)
    with hs.mapped_handle(sd, 1) as f, shaped_bank(f, K, d, ()) as bank:
        before = hs.snapshot(bank)
        for u, why in ((1.0, "u must be"), (-1e-9, "u must be"), (np.nan, "u must be"), (np.inf, "u must be")):
            with pytest.raises(sd.EkfError, match=why):
                bank.resample(u=u)
        for s in (1.0, -0.1, np.nan, 1.5):
            with pytest.raises(sd.EkfError, match="split must be"):
                bank.resample(u=0.5, split=s, z=z)
        bad = z.copy()
        bad[K - 1, 2] = np.inf
        with pytest.raises(sd.EkfError, match="non-finite z"):
            bank.resample(u=0.5, split=0.5, z=bad)
        assert lib.ekf_hypotheses_resample(bank._h, 0.5, 0.5, None, None, None, None, None) == -1
        assert b"needs z" in lib.ekf_hyp_last_error(bank._h)
        assert lib.ekf_hypotheses_resample(bank._h, 0.5, 0.0, z.ctypes.data_as(dp), None, None, None, None) == -1
        assert b"split == 0" in lib.ekf_hyp_last_error(bank._h)
        assert hs.same_snapshot(hs.snapshot(bank), before)
        bank.close()
        for call in (bank.ess, bank.evidence, lambda: bank.resample(u=0.5), bank.resample_if):
            with pytest.raises(sd.EkfError, match="closed"):
                call()


# ---- 6: the kidnapped robot with resampling ------------------------------------------------------------------------------------
def test_kidnapped_robot_with_resampling(sd):
    """tests/hypotheses_model.py's scenario with resample_if(0.5, split = 0.5) behind every step, on the device and in the model
    fleet; the CPU test holds the margin of every resampling and that the model's mixture lies inside the truth's 3 sigma."""
    from slam_duckietown_amd import evaluation as ev
    _, mean0, diag0, lin, ang, idx, zr, zb, m = hm.slam_stream()
    us, zs = rm.kidnapped_draws(hm.K, hm.STEPS)
    with sd.EkfSlam(3 + 2 * hm.N, batch=1, config=sd.EkfConfig(motion_sigma=hm.MOTION_SIGMA, meas_sigma=hm.MEAS_SIGMA)) as f:
        f.set_state_diag(mean0, diag0)
        f.stream_upload(lin, ang, idx, zr, zb, m)
        f.stream_run(0, hm.SLAM_STEPS)
        f.flush()
        mean, cov = f.state(0)
        case = hm.kidnapped_case(mean)
        poses, blocks, ll, events = rm.run_fleet_resampling(mean, cov, case, us, zs)
        assert events and all(e[3] >= rm.MARGIN for e in events)
        with f.hypotheses(hm.K) as bank:
            bank.reset(case.seeds, hm.SEED_COV)
            seen = []
            for i, s in enumerate(case.steps):
                bank.step(*s)
                res = bank.resample_if(rm.FRACTION, split=rm.SPLIT, u=us[i], z=zs[i])
                if res is not None:
                    seen.append((i, res.ancestors, res.offspring))
            assert [e[0] for e in seen] == [e[0] for e in events], "the device resampled at other steps than the model"
            for (i, anc, off), e in zip(seen, events):
                assert np.array_equal(anc, e[1]) and np.array_equal(off, e[2]), f"step {i}"
            got, gblk = bank.poses()
            gap = np.abs(got - poses).max()
            mix = ev.mixture_pose(bank)
            err = mix.mean - case.truth
            err[2] = hm.wrap(err[2])
            maha = float(err @ np.linalg.solve(mix.cov, err))
            print(f"kidnapped robot with resampling: resampled at steps {[e[0] for e in seen]}, poses against the model {gap:.2e} "
                  f"(bar {TOL:g}), mixture Mahalanobis^2 {maha:.3f}, evidence {bank.evidence():.6f}")
            assert gap <= TOL and np.abs(bank.loglik - ll).max() <= TOL * max(1.0, np.abs(ll).max())
            assert (np.abs(err) <= 3.0 * np.sqrt(np.diag(mix.cov))).all()
