"""CPU: the C-ABI surface of ekf_predict_linear (header, library export, binding), the NumPy reference's two formulations on the
input sets the GPU tests use -- with 0, 8 and 80 ranks pending --, the reference against the oracle's built-in prediction,
compose()'s Jacobians, and plan_predict_linear's refusals under the sanitizers (no device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests import direct_model as dm
from tests import host_check
from tests import motion_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS_TOL = 1e-11
PENDING = (0, 8, 80)


def test_header_library_and_binding_declare_the_same_call():
    text = open(os.path.join(ROOT, "include", "ekfslam_hip.h")).read()
    decl = re.search(r"int\s+ekf_predict_linear\s*\(([^)]*)\)\s*;", text)
    assert decl, "ekf_predict_linear is not declared in include/ekfslam_hip.h"
    params = [" ".join(p.split()) for p in re.sub(r"/\*.*?\*/", "", decl.group(1)).split(",")]
    assert params == ["ekf_handle *h", "int b0", "int count", "const double *pose", "const double *F", "const double *Q",
                      "const int *apply"]
    from slam_duckietown_amd import ekf_bindings as eb
    res, args = eb.ABI["ekf_predict_linear"]
    assert res is C.c_int
    assert args == [C.c_void_p, C.c_int, C.c_int, eb._dp, eb._dp, eb._dp, eb._ip]
    for name in ("predict_linear", "predict_odometry", "predict_custom"):
        assert callable(getattr(eb.EkfSlam, name))
    import slam_duckietown_amd as sd
    assert sd.compose_pose is eb.compose_pose
    makefile = open(os.path.join(ROOT, "slam-duckietown_amd", "csrc", "Makefile")).read()
    assert "ekf_predict_linear.hip" in makefile
    lib = eb.library_path()
    if not os.path.exists(lib):
        pytest.skip("the library is not built")
    assert host_check.exported_symbols(lib).get("ekf_predict_linear") == "T"


def forms_agree(mean, cov, pose, F, Q, seed=0):
    """The dense form against the delta form with 0, 8 and 80 ranks pending (the covariance both start from is what the
    deferred representation stands for)."""
    out = None
    for kb in PENDING:
        Pb, W, V, dacc = mm.defer(cov, kb, 1000 * seed + kb)
        cur = mm.materialize(Pb, W, V, dacc)
        wm, wP = mm.predict_linear(mean, cur, pose, F, Q)
        nb = mm.predict_linear_deferred(Pb, W, V, dacc, F, Q)
        assert np.isnan(nb[np.tril_indices(len(nb), -1)]).all()        # nothing below the diagonal was read or written
        got = mm.materialize(nb, W, V, dacc)
        # (the whole matrix, as the GPU tests measure, and the three rows the call changes on their own: never-observed
        #  landmarks carry landmark_init_var = 1e4 on the diagonal and dominate the norm of the whole)
        e, e3 = orc.rel_fro(got, wP), orc.rel_fro(got[:3], wP[:3])
        print("dense against deferred, %2d ranks pending: rel_fro cov %.2e, rows 0..2 %.2e" % (kb, e, e3))
        assert e <= FORMS_TOL and e3 <= FORMS_TOL, (kb, e, e3)
        assert np.array_equal(got[3:, 3:], cur[3:, 3:])                # P(a, b), a, b >= 3: bit for bit
        assert np.array_equal(wm[:3], np.asarray(pose)) and np.array_equal(wm[3:], np.asarray(mean)[3:])
        if kb == 0:
            out = wm, wP
    return out


@pytest.mark.parametrize("kind", mm.KINDS)
def test_the_forms_agree_on_the_small_cases(kind):
    s, rng = mm.case_small(kind=kind)
    om, oP = dm.dense_of(s, dm.SMALL_STEPS)
    pose, F, Q = mm.draw(rng, om, oP, kind)
    assert np.linalg.matrix_rank(Q) == {"full": 3, "rank1": 1, "zero": 0}[kind]
    if kind != "zero":
        assert np.trace(Q) / 3 == pytest.approx(np.trace(oP[:3, :3]) / 3)
    forms_agree(om, oP, pose, F, Q, seed=1)


def test_the_forms_agree_on_the_bank_case():
    streams, rng = mm.case_bank()
    for b in range(4):
        _, om, oP = dm.run_dense(150, 30, 4, 20 + b)
        pose, F, Q = mm.draw(rng, om, oP)
        forms_agree(om, oP, pose, F, Q, seed=2 + b)
    assert len(streams) == 4 and mm.BANK_APPLY == [1, 1, 0, 1]


def test_the_forms_agree_on_states_shaped_like_the_large_cases():
    """The column-panel case and the chained case at sizes the dense oracle can afford (N = 300 and N = 120)."""
    from tests import linear_model as lm
    s, low, high, _, _ = lm.case_panel(N=300, high=296)
    om, oP = dm.dense_of(s, lm.PANEL_STEPS)
    forms_agree(om, oP, *mm.draw(np.random.default_rng(3), om, oP), seed=7)
    s, rng = mm.case_chain(N=120)
    om, oP = dm.dense_of(s, 20)
    forms_agree(om, oP, *mm.draw(rng, om, oP), seed=8)


@pytest.mark.parametrize("branch", ["arc", "straight"])
def test_the_model_reproduces_the_built_in_prediction(branch):
    s = dm.small_stream()
    om, oP = dm.dense_of(s, dm.SMALL_STEPS)
    cfg = orc.EkfConfig()
    lin, ang, pose, G, Qd = mm.builtin_inputs(om, branch, cfg)
    assert (abs(ang) > cfg.arc_threshold) == (branch == "arc") and G[0, 2] != 0.0
    got = mm.predict_linear(om, oP, pose, G, Qd)
    want = orc.predict_dense(om, oP, lin, ang, cfg)
    e = orc.rel_fro(got[0], want[0]), orc.rel_fro(got[1], want[1])
    print("%s: rel_fro mean %.2e cov %.2e" % ((branch,) + e))
    assert max(e) <= 1e-14


def test_compose_jacobians_match_central_differences():
    rng = np.random.default_rng(5)
    for _ in range(20):
        pose = np.array([rng.normal(), rng.normal(), rng.uniform(-3.0, 3.0)])
        delta = np.array([rng.normal() * 0.3, rng.normal() * 0.3, rng.uniform(-0.1, 0.1)])
        new, Fp, Fd = mm.compose(pose, delta)
        assert -np.pi <= new[2] < np.pi
        t = 1e-6
        for c in range(3):
            e = np.zeros(3)
            e[c] = t
            dp = mm.compose(pose + e, delta)[0] - mm.compose(pose - e, delta)[0]
            dd = mm.compose(pose, delta + e)[0] - mm.compose(pose, delta - e)[0]
            dp[2], dd[2] = orc.wrap_pi(dp[2]), orc.wrap_pi(dd[2])
            assert np.allclose(dp / (2 * t), Fp[:, c], atol=1e-8) and np.allclose(dd / (2 * t), Fd[:, c], atol=1e-8)
    from slam_duckietown_amd import ekf_bindings as eb
    for a, b in zip(eb.compose_pose(pose, delta), mm.compose(pose, delta)):     # the binding's helper is the same function
        assert np.array_equal(a, b)
    pose, u = np.array([0.3, -0.2, 0.7]), mm.SLIP_U
    J = mm.slip_jacobian(pose, u)
    for c in range(3):
        e = np.zeros(3)
        e[c] = 1e-6
        assert np.allclose((mm.slip_model(pose + e, u) - mm.slip_model(pose - e, u)) / 2e-6, J[:, c], atol=1e-8)


def test_identity_and_zero_noise_return_the_input_bit_for_bit():
    s, _ = mm.case_small()
    om, oP = dm.dense_of(s, dm.SMALL_STEPS)
    wm, wP = mm.predict_linear(om, oP, om[:3], np.eye(3), np.zeros((3, 3)))
    assert np.array_equal(wm, om) and np.array_equal(wP, oP)
    for kb in PENDING:
        Pb, W, V, dacc = mm.defer(oP, kb, kb)
        nb = mm.predict_linear_deferred(Pb, W, V, dacc, np.eye(3), np.zeros((3, 3)))
        assert np.array_equal(nb, Pb, equal_nan=True)


def test_plan_predict_linear_under_the_sanitizers(tmp_path):
    host_check.run_under_sanitizers("predict_plan_check", tmp_path, 300)
    # the cases' own inputs are accepted: every kind of Q on the small case, the bank's, the built-in model's on both branches
    calls = []
    for kind in mm.KINDS:
        s, rng = mm.case_small(kind=kind)
        om, oP = dm.dense_of(s, dm.SMALL_STEPS)
        calls.append(mm.draw(rng, om, oP, kind))
    streams, rng = mm.case_bank()
    for b in range(4):
        _, om, oP = dm.run_dense(150, 30, 4, 20 + b)
        calls.append(mm.draw(rng, om, oP))
    for branch in mm.BUILTIN:
        calls.append(mm.builtin_inputs(om, branch)[2:])
    path = tmp_path / "calls.txt"
    with open(path, "w") as fp:
        for pose, F, Q in calls:
            fp.write(" ".join(repr(float(v)) for v in np.concatenate([pose, np.ravel(F), np.ravel(Q)])) + "\n")
    run = host_check.run_under_sanitizers("predict_plan_check", tmp_path, 300, args=[str(path)])      # (built above)
    assert int(run.stdout.split()[0]) == 3 * len(calls)
    api = open(os.path.join(ROOT, "slam-duckietown_amd", "csrc", "ekf_api.hip")).read()
    assert re.search(r"\bplan_predict_linear\(", api) and not re.search(r"^(static|inline)[^\n;]*\bplan_predict_linear\(", api, flags=re.M)
