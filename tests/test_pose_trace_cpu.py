"""CPU: the pose log's C-ABI surface, and `evaluation.pose_nees_series` / `evaluation.trajectory_ate` on drawn data (no device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_library_and_binding_declare_the_pose_log():
    text = open(os.path.join(ROOT, "include", "ekfslam_hip.h")).read()
    want = {
        "ekf_log_poses": ["ekf_handle *h", "int capacity"],
        "ekf_pose_steps": ["ekf_handle *h", "long long *logged"],
        "ekf_download_poses": ["ekf_handle *h", "long long first", "int count", "double *pose", "double *cov"],
    }
    from slam_duckietown_amd import ekf_bindings as eb
    types = {
        "ekf_log_poses": [C.c_void_p, C.c_int],
        "ekf_pose_steps": [C.c_void_p, C.POINTER(C.c_longlong)],
        "ekf_download_poses": [C.c_void_p, C.c_longlong, C.c_int, eb._dp, eb._dp],
    }
    lib = C.CDLL(eb.build_library())                        # (dlopen only: no device is touched)
    for name, params in want.items():
        decl = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert decl, f"{name} is not declared in include/ekfslam_hip.h"
        assert [p.strip() for p in decl.group(1).split(",")] == params
        res, args = eb.ABI[name]
        assert res is C.c_int and args == types[name]
        assert hasattr(lib, name), f"{name} is not exported by the library"
    # the two counters are independent, and the header says so
    assert "INDEPENDENT of the innovation log" in text


def _trace(T, B, scale=1.0, seed=0):
    """Errors e ~ N(0, P) with random SPD P per step and trajectory around a drawn truth; the trace reports scale * e."""
    from slam_duckietown_amd.ekf_bindings import PoseTrace
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(T, B, 3, 3)) * 0.3
    P = A @ np.swapaxes(A, -1, -2) + 0.05 * np.eye(3)
    e = (np.linalg.cholesky(P) @ rng.normal(size=(T, B, 3, 1)))[..., 0]
    truth = np.stack([rng.normal(size=(T, B)), rng.normal(size=(T, B)), rng.uniform(-np.pi, np.pi, size=(T, B))], axis=-1)
    mean = truth + scale * e
    return PoseTrace(0, mean, P), truth, scale * e


def test_consistent_pose_errors_land_inside_the_bounds():
    from slam_duckietown_amd.evaluation import chi2_bounds, nees, pose_nees_series
    trace, truth, e = _trace(200, 64)
    r = pose_nees_series(trace, truth)
    assert r.nees.shape == (200, 64) and r.anees.shape == (200,)
    assert (r.lower, r.upper) == pytest.approx(chi2_bounds(3, 64, 0.95))
    assert r.inside >= 0.90
    np.testing.assert_allclose(r.anees, r.nees.mean(axis=1), rtol=0, atol=0)
    # theta errors are wrapped: the same NEES as evaluation.nees on the wrapped errors and the same blocks
    from slam_duckietown_amd.evaluation import wrap_angle
    ew = e.copy()
    ew[..., 2] = wrap_angle(ew[..., 2])
    ref = nees(ew.reshape(-1, 3), trace.cov.reshape(-1, 3, 3)).reshape(200, 64)
    np.testing.assert_allclose(r.nees, ref, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("scale,side", [(1.5, "above"), (1.0 / 1.5, "below")])
def test_mis_scaled_pose_errors_land_outside(scale, side):
    from slam_duckietown_amd.evaluation import pose_nees_series
    trace, truth, _ = _trace(200, 64, scale=scale)
    r = pose_nees_series(trace, truth)
    assert r.inside <= 0.05
    if side == "above":
        assert np.median(r.anees) > r.upper
    else:
        assert np.median(r.anees) < r.lower


def test_pose_nees_series_takes_a_shared_truth():
    from slam_duckietown_amd.evaluation import pose_nees_series
    trace, truth, _ = _trace(20, 4, seed=2)
    shared = truth[:, 0]
    a = pose_nees_series(trace, shared)
    b = pose_nees_series(trace, np.repeat(shared[:, None], 4, axis=1))
    np.testing.assert_array_equal(a.nees, b.nees)
    with pytest.raises(ValueError):
        pose_nees_series(trace, truth[:-1])


def test_trajectory_ate_is_ate_rmse_per_trajectory():
    from slam_duckietown_amd.evaluation import ate_rmse, trajectory_ate
    trace, truth, _ = _trace(50, 5, seed=1)
    for align in (False, True):
        got = trajectory_ate(trace, truth[..., :2], align=align)
        assert got.shape == (5,)
        want = [ate_rmse(trace.mean[:, b, :2], truth[:, b, :2], align=align) for b in range(5)]
        np.testing.assert_allclose(got, want, rtol=0, atol=0)
    shared = truth[:, 0, :2]
    np.testing.assert_array_equal(trajectory_ate(trace, shared), trajectory_ate(trace, np.repeat(shared[:, None], 5, axis=1)))
    with pytest.raises(ValueError):
        trajectory_ate(trace, truth[:-1, :, :2])
