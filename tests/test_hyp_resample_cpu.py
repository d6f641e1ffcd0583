"""CPU: the hypothesis bank's resampling where no GPU is needed -- the properties of the plan in tests/resample_model.py, the
margin every case of tests/test_gpu_hyp_resample.py relies on, the split's moments and its identity with a Schmidt-Kalman update
in tests/localize_model.py's dense algebra, the judge of the GPU test against three wrong implementations, `mixture_pose`, the
host plan under the sanitizers (tests/hyp_resample_plan_check.cpp) and the C ABI (header, export, binding, NULL bank, closed bank)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import host_check
from tests import hypotheses_model as hm
from tests import resample_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ekf_hypotheses_weigh", "ekf_hypotheses_resample"]


@pytest.fixture(scope="module")
def sd():
    import __graft_entry__ as ge
    import slam_duckietown_amd as sd
    if not os.path.exists(sd.library_path()):
        ge.build()
    return sd


@pytest.fixture(scope="module")
def kidnapped():
    mean, cov = hm.model_map()
    case = hm.kidnapped_case(mean)
    us, zs = rm.kidnapped_draws(hm.K, hm.STEPS)
    return case, rm.run_fleet_resampling(mean, cov, case, us, zs)


# ---- the plan ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 64, 65, 1025, 4096])
def test_plan_properties_on_random_log_likelihoods(K):
    rng = np.random.default_rng(K)
    worst, ran = np.inf, 0
    for scale in (0.2, 1.0, 5.0, 30.0):
        for trial in range(12):
            ll = rng.normal(0.0, scale, K)
            ll[rng.random(K) < 0.1] = -np.inf
            ll[rng.random(K) < 0.02] = np.nan
            flags = (rng.random(K) < 0.1).astype(np.uint32)
            u = [0.0, rm.U_LAST, rng.random()][trial % 3]
            anc, off, W = rm.plan(ll, flags, u)
            if W.live == 0:
                assert np.array_equal(anc, np.arange(K)) and (off == 1).all() and W.ess == 0.0 and W.logmean == -np.inf
                continue
            ran += 1
            wn = W.w / W.w.sum()
            assert off.sum() == K and (off >= 0).all()
            assert np.array_equal(np.bincount(anc, minlength=K), off)
            assert np.array_equal(anc[off >= 1], np.nonzero(off >= 1)[0])          # survivors stay in place
            # |offspring - K w| < 1, that is floor(K w) <= offspring <= ceil(K w), with K w known to a few ulps only: a weight of
            # 1e-23 that the point at u = 0 falls into has K w = 2.5e-23 and one offspring, and its neighbour K w = 2 - 2.5e-23,
            # which float64 rounds to 2, has one too
            x = K * wn
            assert (off >= np.floor(x * (1.0 - 1e-15))).all() and (off <= np.ceil(x * (1.0 + 1e-15))).all()
            assert not off[W.w == 0.0].any() and not off[flags != 0].any() and not off[~np.isfinite(ll)].any()
            assert 1.0 - 1e-12 <= W.ess <= W.live + 1e-9
            # dead slots take the surplus offspring in ascending order
            dead = np.nonzero(off == 0)[0]
            assert np.array_equal(anc[dead], np.repeat(np.arange(K), np.maximum(off - 1, 0))) and (np.diff(anc[dead]) >= 0).all()
            # the evidence against a direct sum
            ok = np.isfinite(ll) & (flags == 0)
            assert abs(W.logmean - np.log(np.exp(ll[ok] - ll[ok].max()).sum() / K) - ll[ok].max()) < 1e-12
            worst = min(worst, rm.margin(ll, flags, u))
    print(f"K = {K}: {ran} plans, smallest margin {worst:.3g}")
    assert ran >= 24 or K == 1


def test_plan_by_hand():
    # four equal weights, u = 0.5: the points (j + 0.5) / 4 fall one into each interval
    anc, off, W = rm.plan(np.zeros(4), None, 0.5)
    assert np.array_equal(anc, [0, 1, 2, 3]) and np.array_equal(off, [1, 1, 1, 1]) and W.ess == 4.0 and W.logmean == 0.0
    # weights 0.5, 0.25, 0.25, 0 (and a flagged hypothesis that would have taken everything)
    ll = np.log([0.5, 0.25, 0.25, 1e-300, 100.0])           # (the last: flagged)
    ll[3] = -np.inf
    fl = np.array([0, 0, 0, 0, 1], dtype=np.uint32)
    anc, off, W = rm.plan(ll, fl, 0.25)                    # points 0.05, 0.25, 0.45 | 0.65 | 0.85
    assert np.array_equal(off, [3, 1, 1, 0, 0]) and np.array_equal(anc, [0, 1, 2, 0, 0]) and W.live == 3 and W.last == 2
    assert abs(W.ess - 1.0 / (0.25 + 0.0625 + 0.0625)) < 1e-12 and abs(W.logmean - np.log(0.5 * 2.0 / 5.0)) < 1e-12
    anc, off, _ = rm.plan(ll, fl, 0.9)                     # points 0.18, 0.38 | 0.58 | 0.78, 0.98
    assert np.array_equal(off, [2, 1, 2, 0, 0]) and np.array_equal(anc, [0, 1, 2, 0, 2])
    # the existing host weights are left as they were: a flagged hypothesis still weighs there
    from slam_duckietown_amd.ekf_bindings import HypothesisBank
    assert HypothesisBank.weights_of(ll)[4] > 0.99


def test_margin_of_every_gpu_plan_case():
    """Every case of the GPU test's table, none left out, with the log-likelihoods the dense model gives the device's update: K C_k
    - u keeps 1e-7 from the nearest integer, 50 times the K^2 2^-53 = 1.9e-9 (K = 4096) another summation order can move it."""
    mean, cov = rm.plan_map()
    worst, count = np.inf, 0
    for K in rm.PLAN_KS:
        names = set()
        for name, _, d, u, flagged, dead in rm.plan_cases(K):
            ll = rm.plan_case_logliks(mean, cov, d)
            flags = np.zeros(K, dtype=np.uint32)
            flags[list(flagged)] = rm.NONFINITE
            mg = rm.margin(ll, flags, u)
            assert mg >= rm.MARGIN, f"K = {K}, {name}: margin {mg:.3g}"
            W = rm.weigh(ll, flags)
            assert not W.w[list(dead)].any(), f"K = {K}, {name}: an offset of {rm.DEAD} m does not underflow"
            if name == "typical" and K >= 65:
                assert 0.4 * K < W.ess < 0.6 * K                               # ESS about K / 2
            if name.startswith("uniform"):
                assert mg == 0.5 and rm.margin(ll, flags, 0.0) == 0.0 or K == 1   # (why the identity case uses u = 0.5)
            worst, count = min(worst, mg), count + 1
            names.add(name.split(" at ")[0])
        assert {"typical", "u = 0", "u = 1 - 2^-53", "uniform, the identity", "one-hot", "degenerate: all flagged"} <= names
        assert K < 2 or {"nothing weighs", "a flagged hypothesis"} <= names
    print(f"{count} GPU plan cases, smallest margin {worst:.3g} (bar {rm.MARGIN:g})")
    assert K * K * 2.0 ** -53 * 50 < rm.MARGIN


def test_kidnapped_robot_with_resampling_in_the_model(kidnapped):
    """The GPU test's last scenario on the CPU first: the policy resamples (each time with the margin), the fleet stays finite,
    and the mixture's mean lies inside the truth's 3 sigma."""
    from slam_duckietown_amd import evaluation as ev
    case, (poses, blocks, ll, events) = kidnapped
    assert events and all(mg >= rm.MARGIN for _, _, _, mg in events)
    assert all(off.sum() == hm.K and (off >= 2).any() for _, _, off, _ in events)
    assert np.isfinite(poses).all() and np.isfinite(blocks).all() and np.isfinite(ll).all()
    mix = ev.mixture_pose((poses, blocks), rm.weigh(ll).w)
    err = mix.mean - case.truth
    err[2] = hm.wrap(err[2])
    print(f"resampled at steps {[e[0] for e in events]}; mixture error {err}, sigma {np.sqrt(np.diag(mix.cov))}")
    assert (np.abs(err) <= 3.0 * np.sqrt(np.diag(mix.cov))).all()
    assert float(err @ np.linalg.solve(mix.cov, err)) < hm.CHI2_3_999


# ---- the split -----------------------------------------------------------------------------------------------------------------
def test_split_is_moment_exact():
    """20 000 children of one parent: their mixture -- mean of the displaced means, keep * P plus the scatter of the means -- is
    the parent's pose mean and block within sampling error (5 standard errors of each entry)."""
    rng = np.random.default_rng(17)
    A = rng.normal(size=(3, 3))
    P = A @ A.T * 0.01 + np.diag([1e-4, 1e-4, 1e-5])
    pose, s, M = np.array([0.3, -0.2, 1.1]), 0.6, 20000
    L = rm.chol3(P)
    assert np.abs(L @ L.T - P).max() < 1e-15 and np.abs(L - np.linalg.cholesky(P)).max() < 1e-15
    z = rng.standard_normal((M, 3))
    means = pose + s * (z @ L.T)
    keep = 1.0 - s * s
    mix_mean = means.mean(axis=0)
    d = means - mix_mean
    mix_cov = keep * P + d.T @ d / M
    se_mean = s * np.sqrt(np.diag(P) / M)
    assert (np.abs(mix_mean - pose) <= 5.0 * se_mean).all()
    # an entry of the sample scatter of N(0, s^2 P) has variance s^4 (P_ii P_jj + P_ij^2) / M
    se_cov = s * s * np.sqrt((np.outer(np.diag(P), np.diag(P)) + P * P) / M)
    assert (np.abs(mix_cov - P) <= 5.0 * se_cov).all()
    print(f"mixture of {M} children: mean off by {np.abs(mix_mean - pose).max():.2e}, block by {np.abs(mix_cov - P).max():.2e}")


def test_split_is_a_schmidt_update_with_a_fictitious_pose_fix():
    """keep * X, keep * P_pp and the displaced mean are what the dense Schmidt-Kalman update of tests/localize_model.py's
    algebra -- the gain's landmark rows zeroed, the Joseph form on the whole matrix -- leaves for H = [I_3 0], R = P_pp (1 - s^2) /
    s^2 and a fix drawn at pose + L z / s: to 1e-12, the landmarks' block and means bit for bit."""
    mean, cov = hm.model_map()
    n = len(mean)
    rng = np.random.default_rng(4)
    for s in (0.3, 0.5, 0.9):
        z = rng.standard_normal(3)
        Ppp = cov[:3, :3]
        H = np.zeros((3, n))
        H[:, :3] = np.eye(3)
        R = Ppp * (1.0 - s * s) / (s * s)
        S = H @ cov @ H.T + R                                                  # = P_pp / s^2
        Kg = cov @ H.T @ np.linalg.inv(S)
        Kg[3:] = 0.0                                                           # the landmarks' gain: the map is frozen
        y = rm.chol3(Ppp) @ z / s                                              # fix - pose, drawn from N(0, S)
        want_mean = mean + Kg @ y
        IKH = np.eye(n) - Kg @ H
        want_cov = IKH @ cov @ IKH.T + Kg @ R @ Kg.T
        got_mean, got_cov = rm.split_dense(mean, cov, s, z)
        scale = np.abs(cov).max()
        assert np.abs(got_mean - want_mean).max() <= 1e-12 and np.abs(got_cov - want_cov).max() <= 1e-12 * max(1.0, scale)
        assert np.array_equal(got_cov[3:, 3:], cov[3:, 3:]) and np.array_equal(got_mean[3:], mean[3:])
        assert np.array_equal(got_cov[:3, 3:], (1.0 - s * s) * cov[:3, 3:]) and np.array_equal(got_cov[:3, :3], (1.0 - s * s) * Ppp)


def test_factor_zeroes_the_column_of_a_bad_pivot():
    assert not rm.chol3(np.zeros((3, 3))).any()
    L = rm.chol3(np.diag([0.0, 0.04, 0.01]))
    assert np.array_equal(L, np.diag([0.0, 0.2, 0.1]))
    L = rm.chol3(np.array([[0.04, 0.0, 0.02], [0.0, -1.0, 0.0], [0.02, 0.0, 0.05]]))
    assert L[1, 1] == 0.0 and L[2, 1] == 0.0 and L[0, 0] == 0.2 and abs(L[2, 2] ** 2 - (0.05 - 0.01)) < 1e-15
    assert not rm.chol3(np.diag([np.inf, np.nan, -0.0])).any()


# ---- the GPU test's judge catches wrong implementations --------------------------------------------------------------------------
def model_bank(K, n, rng):
    A = rng.normal(size=(K, 3, 3))
    blk = A @ A.transpose(0, 2, 1) * 0.01 + 1e-4 * np.eye(3)
    rows = rng.normal(size=(K, 3, n)) * 0.01
    rows[:, :, :3] = blk
    return rm.Bank(rng.normal(size=(K, 3)), blk, rows, rng.normal(0.0, 2.0, K), rng.integers(0, 50, K), rng.integers(0, 5, K),
                   np.zeros(K, dtype=np.uint32))


@pytest.mark.parametrize("mutant", ["loglik", "block", "single"])
def test_judge_catches_a_mutant(mutant):
    rng = np.random.default_rng(23)
    bank = model_bank(8, 43, rng)
    z, u, s = rng.standard_normal((8, 3)), 0.3, 0.5
    anc, off, W = rm.plan(bank.loglik, bank.flags, u)
    assert (off == 0).any() and (off >= 2).any() and (off == 1).any()          # copies, split slots and single-offspring slots
    good, _ = rm.resample(bank, u, s, z)
    assert rm.judge(good, bank, u, s, z) is None and rm.judge(good, bank, u, s, z, W.logmean) is None
    bad, _ = rm.resample(bank, u, s, z, mutant=mutant)
    assert rm.judge(bad, bank, u, s, z) is not None, f"the judge let the mutant '{mutant}' pass"
    # ... and a copy that loses a counter, a pose off by more than the bar, an evidence that is off
    for name in ("n_obs", "n_rej"):
        worse = good.copy()
        getattr(worse, name)[np.nonzero(off == 0)[0][0]] += 1
        assert rm.judge(worse, bank, u, s, z) is not None
    worse = good.copy()
    worse.pose[np.nonzero(off[anc] >= 2)[0][0], 1] += 1e-8
    assert rm.judge(worse, bank, u, s, z) is not None
    worse = good.copy()
    worse.loglik[:] = W.logmean + 1e-6
    assert rm.judge(worse, bank, u, s, z, W.logmean + 1e-6) is not None


# ---- mixture_pose ----------------------------------------------------------------------------------------------------------------
def test_mixture_pose():
    from slam_duckietown_amd import evaluation as ev
    P = np.diag([0.01, 0.02, 0.03])
    one = ev.mixture_pose((np.array([[1.0, 2.0, 0.5]]), P[None]))
    assert np.allclose(one.mean, [1.0, 2.0, 0.5], atol=1e-15) and np.allclose(one.cov, P, atol=1e-15)
    # two headings either side of pi average to pi, not to 0
    poses = np.array([[0.0, 0.0, np.pi - 0.1], [2.0, 0.0, -np.pi + 0.1]])
    mix = ev.mixture_pose((poses, np.stack([P, P])), [0.5, 0.5])
    assert abs(abs(mix.mean[2]) - np.pi) < 1e-12 and abs(mix.mean[0] - 1.0) < 1e-15
    assert abs(mix.cov[0, 0] - (0.01 + 1.0)) < 1e-12 and abs(mix.cov[2, 2] - (0.03 + 0.01)) < 1e-12
    assert abs(abs(mix.cov[0, 2]) - 0.1) < 1e-12                               # x and heading move together across the two
    # a bank: weights from loglik, a flagged hypothesis (holding NaN) weighs nothing
    bank = type("Bank", (), {"loglik": np.array([0.0, np.log(3.0), 50.0]), "flags": lambda self: np.array([0, 0, 1]),
                             "poses": lambda self: (np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [np.nan] * 3]), np.stack([P, P, P * np.nan]))})()
    mix = ev.mixture_pose(bank)
    assert np.allclose(mix.weights, [0.25, 0.75, 0.0]) and abs(mix.mean[0] - 3.0) < 1e-12 and abs(mix.cov[0, 0] - (0.01 + 3.0)) < 1e-12
    with pytest.raises(ValueError):
        ev.mixture_pose((np.zeros((0, 3)), np.zeros((0, 3, 3))))
    with pytest.raises(ValueError):
        ev.mixture_pose((poses, np.stack([P, P])), [0.0, 0.0])


# ---- the host plan and the ABI ---------------------------------------------------------------------------------------------------
def test_host_plan_under_the_sanitizers(tmp_path):
    """plan_hyp_resample and the grids (csrc/ekf_host_plan.h) with plain g++ under AddressSanitizer + UndefinedBehaviorSanitizer
    through tests/hyp_resample_plan_check.cpp; and the API takes every shape from them."""
    host_check.run_under_sanitizers("hyp_resample_plan_check", tmp_path, 300)
    api = open(os.path.join(ROOT, "slam-duckietown_amd", "csrc", "ekf_api.hip")).read()
    for fn in ("plan_hyp_resample", "hyp_plan_chunk", "hyp_resample_ints"):
        assert re.search(r"\b%s\(" % fn, api), fn
        assert not re.search(r"^(static|inline)[^\n;]*\b%s\(" % fn, api, flags=re.M), fn
    kernels = open(os.path.join(ROOT, "slam-duckietown_amd", "csrc", "ekf_hypotheses.hip")).read()
    launchers = kernels[kernels.index("void launch_hyp_weigh("):kernels.index("void launch_hyp_solve(")]
    assert launchers.count("hipLaunchKernelGGL") == 5 and not re.search(r"\b(if|for|while)\s*\((?!nt\))", launchers)   # launchers only launch


def test_abi_declares_exports_and_types_both_entry_points(sd):
    from slam_duckietown_amd import ekf_bindings as eb
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ekfslam_hip.h")).read(), flags=re.S)
    symbols = host_check.exported_symbols(sd.library_path())
    lib = sd.load_library()
    for name in NAMES:
        assert symbols.get(name) == "T", f"{name} is not an exported function"
        assert name in eb.ABI and hasattr(lib, name) and eb.ABI[name][0] is C.c_int
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text).group(1)
        assert len(decl.split(",")) == len(eb.ABI[name][1]), name              # one ctypes type per declared argument
        assert not name.startswith("ekf_hyp_")
    assert "HypothesisResampling" in dir(sd) and eb.HypothesisResampling._fields == ("ancestors", "offspring", "ess", "logmean")


def test_null_bank_is_refused_before_any_device_work(sd):
    lib = sd.load_library()
    d, i = (C.c_double * 3)(), (C.c_int * 1)()
    assert lib.ekf_hypotheses_weigh(None, d, d, i) == -1
    assert lib.ekf_hypotheses_weigh(None, None, None, None) == -1
    assert lib.ekf_hypotheses_resample(None, 0.5, 0.0, None, i, i, d, d) == -1
    assert lib.ekf_hypotheses_resample(None, 0.5, 0.5, d, None, None, None, None) == -1


def test_a_closed_bank_refuses_the_new_calls(sd):
    from slam_duckietown_amd import ekf_bindings as eb
    bank = eb.HypothesisBank(sd.load_library(), C.c_void_p(), 4, 43)
    bank.close()
    for call in (bank.ess, bank.evidence, bank.live, lambda: bank.resample(u=0.5), lambda: bank.resample(split=0.5),
                 bank.resample_if, lambda: bank.resample_if(0.9, u=0.1)):
        with pytest.raises(eb.EkfError, match="closed"):
            call()


def test_binding_draws_what_it_is_not_given(sd):
    """`resample` with the library's call stubbed: u and z come from `rng` where they are not given, z goes up only with a split,
    and `resample_if` asks for the effective sample size first."""
    from slam_duckietown_amd import ekf_bindings as eb
    seen = []

    class Stub:
        ess = 1.0

        def ekf_hypotheses_weigh(self, h, ess, logmean, live):
            ess._obj.value, logmean._obj.value, live._obj.value = self.ess, -2.0, 3
            return 0

        def ekf_hypotheses_resample(self, h, u, split, z, anc, off, ess, logmean):
            seen.append((u, split, None if z is None else [z[i] for i in range(9)]))
            for k in range(3):
                anc[k], off[k] = k, 1
            ess._obj.value, logmean._obj.value = 1.5, -2.0
            return 0

    bank = eb.HypothesisBank(Stub(), C.c_void_p(1), 3, 43)
    res = bank.resample(u=0.25)
    assert seen == [(0.25, 0.0, None)] and np.array_equal(res.ancestors, [0, 1, 2]) and (res.ess, res.logmean) == (1.5, -2.0)
    seen.clear()
    bank.resample(split=0.5, rng=np.random.default_rng(7))
    rng = np.random.default_rng(7)
    u = rng.random()
    assert seen == [(u, 0.5, list(rng.standard_normal((3, 3)).ravel()))]
    seen.clear()
    bank.resample(u=0.5, split=0.5, z=[1.0, 2.0, 3.0])                          # one draw for all
    assert seen == [(0.5, 0.5, [1.0, 2.0, 3.0] * 3)]
    seen.clear()
    assert bank.ess() == 1.0 and bank.evidence() == -2.0 and bank.live() == 3
    assert bank.resample_if(0.5, u=0.1) is not None and seen == [(0.1, 0.0, None)]   # 1.0 < 0.5 * 3
    Stub.ess = 2.0
    assert bank.resample_if(0.5, u=0.1) is None and len(seen) == 1
    bank._h = C.c_void_p()                                                      # (nothing to destroy)
