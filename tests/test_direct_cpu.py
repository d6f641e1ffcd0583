"""CPU: the C-ABI surface of ekf_update_direct (header, library export, binding), the NumPy reference's three forms on every
input set the GPU tests use, and plan_direct's refusals under the sanitizers (no device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests import direct_model as dm
from tests import host_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS_TOL = 1e-11


def test_header_library_and_binding_declare_the_same_call():
    text = open(os.path.join(ROOT, "include", "ekfslam_hip.h")).read()
    assert re.search(r"#define\s+EKF_DIRECT_POSE\s+\(-1\)", text) and re.search(r"#define\s+EKF_DIRECT_POSITION\s+\(-2\)", text)
    decl = re.search(r"int\s+ekf_update_direct\s*\(([^)]*)\)\s*;", text)
    assert decl, "ekf_update_direct is not declared in include/ekfslam_hip.h"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["ekf_handle *h", "int b0", "int count", "const int *target", "const double *z", "const double *R",
                      "const int *m", "int stride", "const double *gate", "double *nis", "int *dof", "int *applied"]
    from slam_duckietown_amd import ekf_bindings as eb
    assert (eb.EKF_DIRECT_POSE, eb.EKF_DIRECT_POSITION) == (-1, -2) == (dm.POSE, dm.POSITION)
    res, args = eb.ABI["ekf_update_direct"]
    assert res is C.c_int
    assert args == [C.c_void_p, C.c_int, C.c_int, eb._ip, eb._dp, eb._dp, eb._ip, C.c_int, eb._dp, eb._dp, eb._ip, eb._ip]
    assert eb.DirectUpdate._fields == ("nis", "dof", "applied")
    lib = eb.library_path()
    if not os.path.exists(lib):
        pytest.skip("the library is not built")
    assert host_check.exported_symbols(lib).get("ekf_update_direct") == "T"


def forms_agree(mean, cov, t, z, R):
    a = dm.direct_update(mean, cov, t, z, R)
    j = dm.direct_update_joseph(mean, cov, t, z, R)
    q = dm.direct_update_sequential(mean, cov, t, z, R)
    errs = [orc.rel_fro(j[1], a[1]), orc.rel_fro(q[1], a[1]), orc.rel_fro(j[0], a[0]), orc.rel_fro(q[0], a[0])]
    assert max(errs) <= FORMS_TOL, errs
    assert j[2] == pytest.approx(a[2], rel=1e-9) and a[3] == len(dm.rows_of(t))
    return a


def test_the_three_forms_agree_on_the_small_and_three_fix_cases():
    for s, t, z, R in (dm.case_small(), dm.case_three()):
        om, oP = dm.dense_of(s, 30)
        forms_agree(om, oP, t, z, R)
    s, t, _, _ = dm.case_small()
    assert len(s[0]) == 43 and 17 in t and 17 not in dm.observed(s) and dm.observed(s).max() == 15


def test_the_three_forms_agree_on_the_bank_case_and_its_gate():
    from scipy.stats import chi2
    streams, fixes = dm.case_bank()
    for b, (t, z, R) in enumerate(fixes):
        _, om, oP = dm.run_dense(150, 30, 4, 20 + b)
        a = forms_agree(om, oP, t, z, R)
        assert a[3] == [3, 32, 0, 3][b]
        if b == 3:                                            # 10 sigma off: far beyond the gate the GPU test sets
            assert a[2] > 10 * chi2.ppf(0.99, 3)
            g = dm.direct_update(om, oP, t, z, R, chi2.ppf(0.99, 3))
            assert not g[4] and np.array_equal(g[0], om) and np.array_equal(g[1], oP)
        if b == 1:
            obs = dm.observed(streams[1])
            assert 130 not in obs and 149 not in obs and 130 in t and 149 in t


def test_the_three_forms_agree_on_a_state_shaped_like_the_large_case():
    """The large case's state at a size the dense Joseph form can afford (N = 300 instead of 2060): 40 steps of m = 8, the
    last landmark observed once more, a pose fix, landmark 0, the last landmark and a never-observed one."""
    N = 300
    s, om, oP = dm.run_dense(N, 20, 8, 3)
    cfg = orc.EkfConfig()
    d = om[3 + 2 * (N - 1):5 + 2 * (N - 1)] - om[:2]
    om, oP = orc.ekf_step_dense(om, oP, 0.0, 0.0, [N - 1], [np.hypot(*d) + 0.01], [orc.wrap_pi(np.arctan2(d[1], d[0]) - om[2]) + 0.01], cfg)
    oP = (oP + oP.T) / 2
    rng = np.random.default_rng(5)
    t = [dm.POSE, 0, N - 1, 250]
    z, R = dm.make_fixes(rng, om, oP, t[:3])
    z1, R1 = dm.make_fixes(rng, om, np.diag(np.full(len(om), 0.01)), [250])
    a = forms_agree(om, oP, t, z + z1, R + R1)
    v, Rl, blk = cfg.landmark_init_var, R1[0][:2, :2], slice(3 + 2 * 250, 5 + 2 * 250)
    want = Rl @ np.linalg.solve(Rl + v * np.eye(2), v * np.eye(2))
    assert np.abs(a[1][blk, blk] - want).max() <= 32 * np.finfo(float).eps * v


def test_the_gauge_case_separates_the_forks_on_the_oracle():
    s, survey = dm.case_gauge()
    cfg = orc.EkfConfig(**dm.gauge_config())
    om, oP = s[0].copy(), np.diag(s[1])
    for k in range(dm.GAUGE_STEPS):
        om, oP = orc.ekf_step_dense(om, oP, s[2][k], s[3][k], s[4][k], s[5][k], s[6][k], cfg)
    oP = (oP + oP.T) / 2
    A = list(dm.GAUGE_ANCHORS)
    a = forms_agree(om, oP, A, [survey[j] for j in A], [np.eye(2) * dm.GAUGE_SIGMA ** 2] * 2)
    blocks = lambda P: [P[3 + 2 * j:5 + 2 * j, 3 + 2 * j:5 + 2 * j] for j in range(dm.GAUGE_N)]
    obs = dm.observed(s)
    assert dm.within_sigmas(a[0], blocks(a[1]), survey, obs).all()
    assert not dm.within_sigmas(om, blocks(oP), survey, obs).any()


def test_plan_direct_under_the_sanitizers(tmp_path):
    host_check.run_under_sanitizers("direct_plan_check", tmp_path, 300)
    api = open(os.path.join(ROOT, "slam-duckietown_amd", "csrc", "ekf_api.hip")).read()
    assert re.search(r"\bplan_direct\(", api) and not re.search(r"^(static|inline)[^\n;]*\bplan_direct\(", api, flags=re.M)
