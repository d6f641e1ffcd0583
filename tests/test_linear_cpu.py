"""CPU: the C-ABI surface of ekf_update_linear (header, library export, binding), the NumPy reference's two forms on every
input set the GPU tests use, the reference against direct_model where H is a selection, and plan_linear's refusals under
the sanitizers (no device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests import direct_model as dm
from tests import host_check
from tests import linear_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS_TOL = 1e-11


def test_header_library_and_binding_declare_the_same_call():
    text = open(os.path.join(ROOT, "include", "ekfslam_hip.h")).read()
    assert re.search(r"#define\s+EKF_LINEAR_LMAX\s+16\b", text) and re.search(r"#define\s+EKF_LINEAR_ROWS\s+32\b", text)
    decl = re.search(r"int\s+ekf_update_linear\s*\(([^)]*)\)\s*;", text)
    assert decl, "ekf_update_linear is not declared in include/ekfslam_hip.h"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["ekf_handle *h", "int b0", "int count", "const int *landmarks", "const int *k", "int lstride",
                      "const double *H", "const double *r", "const double *R", "const int *d", "int dstride", "int innovation",
                      "const double *gate", "double *nis", "int *applied"]
    from slam_duckietown_amd import ekf_bindings as eb
    assert (eb.EKF_LINEAR_LMAX, eb.EKF_LINEAR_ROWS) == (16, 32)
    res, args = eb.ABI["ekf_update_linear"]
    assert res is C.c_int
    assert args == [C.c_void_p, C.c_int, C.c_int, eb._ip, eb._ip, C.c_int, eb._dp, eb._dp, eb._dp, eb._ip, C.c_int, C.c_int,
                    eb._dp, eb._dp, eb._ip]
    assert eb.LinearUpdate._fields == ("nis", "dof", "applied")
    for name in ("update_linear", "constrain_landmarks", "update_custom"):
        assert callable(getattr(eb.EkfSlam, name))
    makefile = open(os.path.join(ROOT, "slam-duckietown_amd", "csrc", "Makefile")).read()
    assert "ekf_linear.hip" in makefile
    lib = eb.library_path()
    if not os.path.exists(lib):
        pytest.skip("the library is not built")
    assert host_check.exported_symbols(lib).get("ekf_update_linear") == "T"


def forms_agree(mean, cov, lms, H, R, r, innovation=False):
    a = lm.linear_update(mean, cov, lms, H, R, r, innovation)
    j = lm.linear_update_joseph(mean, cov, lms, H, R, r, innovation)
    errs = [orc.rel_fro(j[1], a[1]), orc.rel_fro(j[0], a[0])]
    print("simple against Joseph: rel_fro cov %.2e mean %.2e" % tuple(errs))
    assert max(errs) <= FORMS_TOL, errs
    assert j[2] == pytest.approx(a[2], rel=1e-9) and a[3] == len(r)
    return a


def test_the_forms_agree_on_the_small_cases():
    s, lms, H, R, z = lm.case_small()
    om, oP = dm.dense_of(s, dm.SMALL_STEPS)
    assert H.shape == (7, 9) and all(l in dm.observed(s) for l in lms)
    forms_agree(om, oP, lms, H, R, z)
    # the hook case: the reference's own observation of one landmark, as an innovation
    s, l, zr, zb = lm.case_hook()
    xs = om[lm.sub_indices([l])]
    h, J = lm.range_bearing(xs)
    y = np.array([zr - h[0], orc.wrap_pi(zb - h[1])])
    cfg = orc.EkfConfig()
    a = forms_agree(om, oP, [l], J, np.diag(cfg.meas_noise_diag()), y, innovation=True)
    want = orc.update_dense(om, oP, [l], [zr], [zb], cfg)
    assert orc.rel_fro(a[0], want[0]) <= 1e-9 and orc.rel_fro(a[1], want[1]) <= 1e-9
    # the custom case
    s, pair, z, R = lm.case_custom()
    h, J, _ = lm.distance_model(om[lm.sub_indices(pair)])
    forms_agree(om, oP, pair, J, R, z - h, innovation=True)


def test_a_selection_reproduces_the_direct_model():
    s, t, z, R = lm.case_selection()
    om, oP = dm.dense_of(s, dm.SMALL_STEPS)
    lms, H, RR, zz = lm.selection_of(t, z, R)
    assert H.shape == (6, 7) and (H.sum(axis=1) == 1.0).all() and lms == [5, 17]
    a = forms_agree(om, oP, lms, H, RR, zz)
    d = dm.direct_update(om, oP, t, z, R)
    assert orc.rel_fro(a[0], d[0]) <= 1e-13 and orc.rel_fro(a[1], d[1]) <= 1e-13
    assert a[2] == pytest.approx(d[2], rel=1e-12) and a[3] == d[3] == 6 and a[4] and d[4]


def test_the_forms_agree_on_the_bank_case_and_its_gate():
    from scipy.stats import chi2
    streams, meas, draw = lm.case_bank()
    for b, (lms, H, R) in enumerate(meas):
        _, om, oP = dm.run_dense(150, 30, 4, 20 + b)
        y = lm.bank_innovation(b, meas, draw, om, oP)
        a = forms_agree(om, oP, lms, H, R, y, innovation=True)
        assert a[3] == [1, 32, 0, 2][b]
        if b == 1:
            obs = dm.observed(streams[1])
            assert len(lms) == 16 and len(set(lms)) == 16 and all(l in lms and l not in obs for l in lm.BANK_NEVER)
        if b == 3:                                            # 10 sigma off on both rows: far beyond the gate the GPU test sets
            assert a[2] > 5 * chi2.ppf(0.99, 2)
            g = lm.linear_update(om, oP, lms, H, R, y, True, chi2.ppf(0.99, 2))
            assert not g[4] and np.array_equal(g[0], om) and np.array_equal(g[1], oP)


def test_the_forms_agree_on_the_constraint_and_the_merge():
    s, i, j, offset, cov = lm.case_constraint()
    om, oP = dm.dense_of(s, dm.SMALL_STEPS)
    lms, H, R, z = lm.constraint_rows(i, j, offset, cov)
    a = forms_agree(om, oP, lms, H, R, z)
    # far below the map's uncertainty, and the posterior separation is the offset to within its own sigma
    si, sj = slice(3 + 2 * i, 5 + 2 * i), slice(3 + 2 * j, 5 + 2 * j)
    prior = oP[sj, sj] + oP[si, si] - oP[sj, si] - oP[si, sj]
    assert np.linalg.eigvalsh(prior).min() > 100 * lm.CONSTRAINT_SIGMA ** 2
    d = a[0][sj] - a[0][si]
    Pd = a[1][sj, sj] + a[1][si, si] - a[1][sj, si] - a[1][si, sj]
    g = d / np.hypot(*d)
    assert abs(np.hypot(*d) - np.hypot(*offset)) <= np.sqrt(g @ Pd @ g)
    # the merge: a zero offset with the same covariance
    forms_agree(om, oP, lms, H, R, np.zeros(2))


def test_the_forms_agree_on_a_state_shaped_like_the_panel_case():
    """The panel case at a size the dense Joseph form can afford (N = 300 instead of 2050): diagonal start, 5 steps of
    m = 8, a constraint between a never-observed high landmark and the first observed one."""
    s, low, high, offset, cov = lm.case_panel(N=300, high=296)
    om, oP = dm.dense_of(s, lm.PANEL_STEPS)
    assert high not in dm.observed(s) and low in dm.observed(s)
    lms, H, R, z = lm.constraint_rows(low, high, offset, cov)
    forms_agree(om, oP, lms, H, R, z)
    s, low, high, _, _ = lm.case_panel()
    assert (3 + 2 * high, 4 + 2 * high) == (4095, 4096) and len(s[0]) == 4103 and high not in dm.observed(s)


def test_plan_linear_under_the_sanitizers(tmp_path):
    host_check.run_under_sanitizers("linear_plan_check", tmp_path, 300)
    api = open(os.path.join(ROOT, "slam-duckietown_amd", "csrc", "ekf_api.hip")).read()
    assert re.search(r"\bplan_linear\(", api) and not re.search(r"^(static|inline)[^\n;]*\bplan_linear\(", api, flags=re.M)
