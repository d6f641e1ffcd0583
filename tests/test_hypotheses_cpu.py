"""CPU: the hypothesis bank's surface that needs no GPU -- the kidnapped-robot fleet through the dense model with the margins the
GPU test relies on, `frontend.poses_on_circle`, the weights and `evaluation.resolve_hypotheses` on hand-made log-likelihoods, the
C ABI (header, export, binding, NULL handles) and the host plan under the sanitizers (tests/hyp_plan_check.cpp)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import host_check
from tests import hypotheses_model as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HYP_NAMES = ["ekf_hyp_create", "ekf_hyp_destroy", "ekf_hyp_reset", "ekf_hyp_step", "ekf_hyp_update", "ekf_hyp_download",
             "ekf_hyp_download_rows", "ekf_hyp_set_nis_gate", "ekf_hyp_adopt", "ekf_hyp_sync", "ekf_hyp_last_error"]


@pytest.fixture(scope="module")
def sd():
    import __graft_entry__ as ge
    import slam_duckietown_amd as sd
    if not os.path.exists(sd.library_path()):
        ge.build()
    return sd


@pytest.fixture(scope="module")
def fleet():
    mean, cov = hm.model_map()
    case = hm.kidnapped_case(mean)
    return case, hm.run_fleet(mean, cov, case)


def test_model_fleet_finds_the_robot_with_margin(fleet):
    """The scenario of tests/test_gpu_hypotheses.py through localize_model.literal_step: the hypothesis seeded next to the truth
    wins, NEES <= 8 where the GPU test asks for 16.27, runner-up weight <= 1e-3 where it asks for a ratio below 0.01."""
    from slam_duckietown_amd import evaluation as ev
    from slam_duckietown_amd.ekf_bindings import HypothesisBank
    case, (poses, blocks, ll) = fleet
    res = ev.resolve_hypotheses(ll, confidence=0.99)
    w = HypothesisBank.weights_of(ll)
    nees = hm.pose_nees(poses[res.best], blocks[res.best], case.truth)
    print(f"model fleet: best {res.best} weight {res.weight:.6f}, runner-up {res.runner_up} weight {w[res.runner_up]:.3e}, NEES {nees:.3f}")
    assert hm.heading_gap(case.seeds[res.best, 2]) < case.spacing
    assert nees <= hm.NEES_BAR < hm.CHI2_3_999
    assert w[res.runner_up] <= hm.RUNNER_UP_BAR and res.separated
    assert np.isfinite(ll).all() and np.isfinite(poses).all()


def test_poses_on_circle_reproduce_the_sighting():
    from slam_duckietown_amd import frontend
    rng = np.random.default_rng(3)
    for count in (1, 2, 7, 64, 1000):
        lm = rng.normal(size=2)
        r, b = float(rng.uniform(0.2, 3.0)), float(rng.uniform(-np.pi, np.pi))
        poses = frontend.poses_on_circle(lm, r, b, count)
        assert poses.shape == (count, 3)
        d = lm - poses[:, :2]
        assert np.abs(np.hypot(d[:, 0], d[:, 1]) - r).max() < 1e-12
        assert np.abs(hm.wrap(np.arctan2(d[:, 1], d[:, 0]) - poses[:, 2] - b)).max() < 1e-12
        # headings evenly spaced over [-pi, pi)
        assert poses[0, 2] == -np.pi and (poses[:, 2] < np.pi).all()
        if count > 1:
            assert np.abs(np.diff(poses[:, 2]) - 2.0 * np.pi / count).max() < 1e-12
    with pytest.raises(ValueError):
        frontend.poses_on_circle([0.0, 0.0], 1.0, 0.0, 0)


def test_weights_and_resolution_on_hand_made_log_likelihoods():
    from slam_duckietown_amd import evaluation as ev
    from slam_duckietown_amd.ekf_bindings import HypothesisBank
    wo = HypothesisBank.weights_of
    w = wo([-3.0, -1.0, -2.0])
    e = np.exp(np.array([-2.0, 0.0, -1.0]))
    assert np.allclose(w, e / e.sum(), rtol=1e-15) and abs(w.sum() - 1.0) < 1e-15
    assert np.array_equal(wo([-1e6, -1e6 - 800.0]), [1.0, 0.0])                   # (no overflow, no NaN far from zero)
    assert np.array_equal(wo([5.0, 5.0, 5.0, 5.0]), [0.25] * 4)                  # all equal
    assert np.array_equal(wo([-np.inf, -2.0, -np.inf]), [0.0, 1.0, 0.0])         # -inf weighs nothing
    assert np.array_equal(wo([np.nan, -2.0]), [0.0, 1.0])                        # a NaN weighs nothing
    assert np.array_equal(wo([-np.inf, -np.inf]), [0.5, 0.5])                    # nothing finite: shared
    assert np.array_equal(wo([np.inf, 3.0, np.inf]), [0.5, 0.0, 0.5])            # +inf takes everything
    r = ev.resolve_hypotheses([-10.0, 0.0, -4.0], confidence=0.99)
    assert (r.best, r.runner_up, r.separated) == (1, 2, False) and abs(r.ratio - np.exp(-4.0)) < 1e-15   # e^-4 = 0.018 > 0.01
    r = ev.resolve_hypotheses([-10.0, 0.0, -5.0], confidence=0.99)
    assert (r.best, r.runner_up, r.separated) == (1, 2, True)                      # e^-5 = 0.0067 < 0.01
    assert not ev.resolve_hypotheses([-10.0, 0.0, -5.0], confidence=0.999).separated
    r = ev.resolve_hypotheses([2.0, 2.0, 2.0])
    assert r.best == 0 and not r.separated and r.ratio == 1.0 and abs(r.weight - 1.0 / 3.0) < 1e-15
    r = ev.resolve_hypotheses([-np.inf, -1.0, -np.inf])
    assert r.best == 1 and r.weight == 1.0 and r.separated and r.ratio == 0.0
    assert not ev.resolve_hypotheses([-np.inf, -np.inf]).separated
    assert not ev.resolve_hypotheses([np.inf, np.inf, 0.0]).separated
    r = ev.resolve_hypotheses([-7.0])
    assert (r.best, r.weight, r.separated, r.runner_up) == (0, 1.0, True, -1)
    # anything with a .loglik is a bank
    assert ev.resolve_hypotheses(type("Bank", (), {"loglik": np.array([0.0, -9.0])})()).separated
    with pytest.raises(ValueError):
        ev.resolve_hypotheses([])
    with pytest.raises(ValueError):
        ev.resolve_hypotheses([0.0, 1.0], confidence=1.0)


def test_abi_declares_exports_and_types_every_entry_point(sd):
    from slam_duckietown_amd import ekf_bindings as eb
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ekfslam_hip.h")).read(), flags=re.S)
    assert "typedef struct ekf_hypotheses ekf_hypotheses;" in text
    declared = sorted(set(re.findall(r"\b(ekf_hyp_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(HYP_NAMES)
    symbols = host_check.exported_symbols(sd.library_path())
    lib = sd.load_library()
    for name in HYP_NAMES:
        assert symbols.get(name) == "T", f"{name} is not an exported function"
        assert name in eb.ABI and hasattr(lib, name)
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text).group(1)
        assert len(decl.split(",")) == len(eb.ABI[name][1]), name               # one ctypes type per declared argument
    assert eb.ABI["ekf_hyp_last_error"][0] is C.c_char_p
    assert all(eb.ABI[n][0] is C.c_int for n in HYP_NAMES if n != "ekf_hyp_last_error")


def test_null_handles_are_refused_before_any_device_work(sd):
    lib = sd.load_library()
    hy, d, i = C.c_void_p(), (C.c_double * 12)(), (C.c_int * 4)()
    ll, u = (C.c_longlong * 1)(), (C.c_uint * 1)()
    assert lib.ekf_hyp_create(None, 0, 4, C.byref(hy)) == -1 and not hy.value
    assert lib.ekf_hyp_destroy(None) == -1
    assert lib.ekf_hyp_reset(None, 0, 1, d, d) == -1
    assert lib.ekf_hyp_step(None, d, d, 0, i, d, d, i, 1, 0) == -1
    assert lib.ekf_hyp_update(None, i, d, d, i, 1, 0) == -1
    assert lib.ekf_hyp_download(None, 0, 1, d, d, d, ll, ll, u) == -1
    assert lib.ekf_hyp_download_rows(None, 0, d, 3) == -1
    assert lib.ekf_hyp_set_nis_gate(None, 5.99) == -1
    assert lib.ekf_hyp_adopt(None, 0, None, 0) == -1
    assert lib.ekf_hyp_sync(None) == -1
    assert isinstance(lib.ekf_hyp_last_error(None), bytes)


def test_a_closed_bank_refuses_every_call(sd):
    """`HypothesisBank` after close(): every method raises before it reaches the library (no device needed: the bank is made
    around a NULL handle, which is what close() leaves)."""
    from slam_duckietown_amd import ekf_bindings as eb
    bank = eb.HypothesisBank(sd.load_library(), C.c_void_p(), 4, 43)
    bank.close()                                                              # (idempotent)
    calls = [lambda: bank.step(0.004, 0.02, [0], [1.0], [0.1]), lambda: bank.update([0], [1.0], [0.1]),
             lambda: bank.reset(np.zeros(3), np.eye(3)), bank.poses, lambda: bank.loglik, lambda: bank.rejected, lambda: bank.rows(0),
             bank.weights, bank.best, lambda: bank.adopt(0, None), lambda: bank.set_nis_gate(confidence=0.99), bank.sync]
    for call in calls:
        with pytest.raises(eb.EkfError, match="closed"):
            call()


def test_binding_splits_long_lists_and_picks_the_stride_modes(sd):
    """What `HypothesisBank.step` hands to the library, with the library's calls stubbed: scalars and one list give stride
    modes 0 / 0 and one call; 20 shared observations a step of 16 and an update of 4; per-hypothesis lists mode 1."""
    from slam_duckietown_amd import ekf_bindings as eb
    seen = []

    class Stub:
        def ekf_hyp_step(self, h, lin, ang, ms, idx, r, b, m, stride, os_):
            seen.append(("step", ms, os_, stride, [m[k] for k in range(3 if os_ else 1)], [idx[k] for k in range(stride)]))
            return 0

        def ekf_hyp_update(self, h, idx, r, b, m, stride, os_):
            seen.append(("update", os_, stride, [m[k] for k in range(3 if os_ else 1)], [idx[k] for k in range(stride)]))
            return 0

    bank = eb.HypothesisBank(Stub(), C.c_void_p(1), 3, 43)
    bank.step(0.004, 0.02, [4, 5], [1.0, 2.0], [0.1, 0.2])
    assert seen == [("step", 0, 0, 2, [2], [4, 5])]
    seen.clear()
    bank.step(0.004, 0.02, list(range(20)), np.ones(20), np.zeros(20))
    assert seen == [("step", 0, 0, 16, [16], list(range(16))), ("update", 0, 4, [4], [16, 17, 18, 19])]
    seen.clear()
    bank.step([0.1, 0.2, 0.3], 0.02, [[], [7, 8, 9], [1]], [[], [1.0, 1.0, 1.0], [2.0]], [[], [0.0, 0.0, 0.0], [0.5]])
    assert seen == [("step", 1, 1, 3, [0, 3, 1], [0, 0, 0])]
    seen.clear()
    bank.update([3], [1.0], [0.0])
    assert seen == [("update", 0, 1, [1], [3])]
    with pytest.raises(ValueError):
        bank.step(0.0, 0.0, [[1], [2]], [[1.0], [1.0]], [[0.0], [0.0]])           # two lists for three hypotheses
    bank._h = C.c_void_p()                                                      # (nothing to destroy)


def test_host_plan_under_the_sanitizers(tmp_path):
    """plan_hyp_* and fill_hyp_records (csrc/ekf_host_plan.h) compiled with plain g++ under AddressSanitizer +
    UndefinedBehaviorSanitizer and run through tests/hyp_plan_check.cpp: argument checks in both stride modes, the bound of
    EKF_MMAX observations, the index bounds, the grids at n = 3, 258, 259, 4103 and K = 1, 65, 4096, the bytes per hypothesis."""
    host_check.run_under_sanitizers("hyp_plan_check", tmp_path, 300)
    api = open(os.path.join(ROOT, "slam-duckietown_amd", "csrc", "ekf_api.hip")).read()
    for fn in ("plan_hyp_create", "plan_hyp_range", "plan_hyp_step", "fill_hyp_records", "plan_hyp_reset", "hyp_fill_groups",
               "hyp_compare_groups", "hyp_adopt_groups"):
        assert re.search(r"\b%s\(" % fn, api), fn                                # called from the API ...
        assert not re.search(r"^(static|inline)[^\n;]*\b%s\(" % fn, api, flags=re.M), fn   # ... and defined only in the header
