"""CPU: the innovation log's C-ABI surface and `evaluation.nis_consistency` on seeded Gaussian innovations (no device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_declare_the_innovation_log():
    text = open(os.path.join(ROOT, "include", "ekfslam_hip.h")).read()
    want = {
        "ekf_log_innovations": ["ekf_handle *h", "int capacity"],
        "ekf_innovation_steps": ["ekf_handle *h", "long long *logged"],
        "ekf_download_innovations": ["ekf_handle *h", "long long first", "int count", "int *m", "int *idx", "double *y",
                                     "double *S", "double *nis"],
    }
    from slam_duckietown_amd import ekf_bindings as eb
    types = {
        "ekf_log_innovations": [C.c_void_p, C.c_int],
        "ekf_innovation_steps": [C.c_void_p, C.POINTER(C.c_longlong)],
        "ekf_download_innovations": [C.c_void_p, C.c_longlong, C.c_int, eb._ip, eb._ip, eb._dp, eb._dp, eb._dp],
    }
    for name, params in want.items():
        decl = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert decl, f"{name} is not declared in include/ekfslam_hip.h"
        assert [p.strip() for p in decl.group(1).split(",")] == params
        res, args = eb.ABI[name]
        assert res is C.c_int and args == types[name]


def _log(K, B, W, scale=1.0, seed=3, pad=True):
    """A stand-in log: K steps x B trajectories x up to W updates, y ~ N(0, S_true), reported S = scale * S_true; entries
    beyond each step's m NaN (as EkfSlam.innovations() pads them)."""
    from slam_duckietown_amd.ekf_bindings import Innovations
    rng = np.random.default_rng(seed)
    m = rng.integers(0 if pad else W, W + 1, size=(K, B)).astype(np.int32)
    A = rng.normal(size=(K, B, W, 2, 2)) * 0.4
    S_true = A @ np.swapaxes(A, -1, -2) + 0.3 * np.eye(2)
    L = np.linalg.cholesky(S_true)
    y = (L @ rng.normal(size=(K, B, W, 2, 1)))[..., 0]
    S = scale * S_true
    nis = np.einsum("...i,...i->...", y, np.linalg.solve(S, y[..., None])[..., 0])
    on = np.arange(W)[None, None, :] < m[..., None]
    idx = np.where(on, rng.integers(0, 50, size=(K, B, W)), -1).astype(np.int32)
    y = np.where(on[..., None], y, np.nan)
    S = np.where(on[..., None, None], S, np.nan)
    nis = np.where(on, nis, np.nan)
    return Innovations(np.arange(K), m, idx, y, S, nis)


def test_consistent_innovations_land_inside_the_bounds():
    from slam_duckietown_amd.evaluation import nis_consistency
    innov = _log(400, 16, 8)
    r = nis_consistency(innov)
    assert r.updates == int(innov.m.sum())
    # the averages over the whole run sit inside bounds of the whole run (the per-step / per-trajectory ones: ~95 % inside)
    from slam_duckietown_amd.evaluation import chi2_bounds
    lo, hi = chi2_bounds(2 * r.updates, 1)
    assert lo <= r.traj_anis.sum() * 400 <= hi            # the sum of every NIS of the run
    inside_t = (r.traj_anis >= r.traj_bounds[:, 0]) & (r.traj_anis <= r.traj_bounds[:, 1])
    assert inside_t.mean() >= 0.8
    steps = np.isfinite(r.step_anis)
    inside_s = (r.step_anis >= r.step_bounds[:, 0]) & (r.step_anis <= r.step_bounds[:, 1])
    assert inside_s[steps].mean() >= 0.9
    assert abs(r.above_gate - 0.05) < 0.02
    assert r.gate == pytest.approx(-2.0 * np.log(0.05))   # the chi2_2 quantile in closed form


@pytest.mark.parametrize("scale,side", [(0.25, "above"), (4.0, "below")])
def test_mis_scaled_covariances_land_outside(scale, side):
    from slam_duckietown_amd.evaluation import nis_consistency
    r = nis_consistency(_log(200, 8, 8, scale=scale))
    if side == "above":                                     # S too small: over-confident, NIS x 4
        assert (r.traj_anis > r.traj_bounds[:, 1]).all()
        assert r.above_gate > 0.3
    else:                                                   # S too large: conservative, NIS / 4
        assert (r.traj_anis < r.traj_bounds[:, 0]).all()
        assert r.above_gate < 0.01
    steps = np.isfinite(r.step_anis)
    out = (r.step_anis > r.step_bounds[:, 1]) if side == "above" else (r.step_anis < r.step_bounds[:, 0])
    assert out[steps].mean() > 0.9


def test_log_likelihood_is_the_gaussian_logpdf_summed():
    from scipy.stats import multivariate_normal
    from slam_duckietown_amd.evaluation import nis_consistency
    innov = _log(30, 3, 5, scale=1.7, seed=11)
    r = nis_consistency(innov)
    for b in range(3):
        want = 0.0
        for k in range(30):
            for j in range(int(innov.m[k, b])):
                want += multivariate_normal.logpdf(innov.y[k, b, j], mean=np.zeros(2), cov=innov.S[k, b, j])
        assert r.loglik[b] == pytest.approx(want, rel=1e-12, abs=1e-9)


def test_nan_padding_is_ignored():
    from slam_duckietown_amd.evaluation import nis_consistency
    from slam_duckietown_amd.ekf_bindings import Innovations
    innov = _log(20, 4, 6, seed=7)
    r = nis_consistency(innov)
    # the same log with twice the width, the extra entries NaN, gives the same statistics
    wide = Innovations(innov.steps, innov.m, np.concatenate([innov.idx, -np.ones_like(innov.idx)], axis=2),
                       np.concatenate([innov.y, np.full_like(innov.y, np.nan)], axis=2),
                       np.concatenate([innov.S, np.full_like(innov.S, np.nan)], axis=2),
                       np.concatenate([innov.nis, np.full_like(innov.nis, np.nan)], axis=2))
    w = nis_consistency(wide)
    assert w.updates == r.updates == int(innov.m.sum())
    for a, b in zip(r, w):
        np.testing.assert_allclose(np.asarray(a, dtype=float), np.asarray(b, dtype=float), rtol=1e-13, equal_nan=True)
    # a step where nothing was observed anywhere: NaN average and NaN bounds, no effect on the rest
    empty = innov.m.copy()
    empty[3] = 0
    nis = innov.nis.copy()
    nis[3] = np.nan
    S = innov.S.copy()
    S[3] = np.nan
    e = nis_consistency(Innovations(innov.steps, empty, innov.idx, innov.y, S, nis))
    assert np.isnan(e.step_anis[3]) and np.isnan(e.step_bounds[3]).all()
    assert np.isfinite(e.loglik).all()
