"""ctypes bindings of libekfslam_hip.so -- the module the reference's empty ``src/ekf_bindings.py`` stands for.

Call surface:

* ``EKF_pose_estimation(ang, lin, mean, cov, delta_t, detections, TAG_INDEX)``
  drop-in for ``src/replay_no_ros.py:269-482`` (same arguments, same return triple, ``TAG_INDEX``
  mutated the same way).  Association stays on the host (``frontend.associate``); augmentation,
  prediction and the sequential update run on the GPU.
* ``EkfSlam(n_max, batch=1, ...)`` with ``predict / update / step / run_stream`` keeps the state
  resident in HBM -- this is the fast path.
* ``predict(state, covariance, control, dt)`` / ``update(state, covariance, observation,
  landmark_pos)``: the 3-state prototype surface of ``src/EKF-SLAM.py:29-84``.

There is NO CPU fallback: if the shared library or a gfx950 device is missing, calls raise
``EkfError``.  Host code is NumPy + ctypes only (no PyTorch, no CuPy).
"""
from __future__ import annotations

import collections
import ctypes as C
import dataclasses
import math
import os
import subprocess
import threading
import typing
import warnings
import weakref
from typing import Optional, Sequence

import numpy as np

from .frontend import associate, associate_known, fit_transform, joint_compatibility, remap_tag_index, resolve_associations

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libekfslam_hip.so"
EKF_MMAX = 16
EKF_JMAX = 64                     # landmarks per trajectory in one joint() query
EKF_DIRECT_POSE = -1              # update_direct target: x, y, theta (3 rows)
EKF_DIRECT_POSITION = -2          # update_direct target: x, y (2 rows); a target l >= 0 is landmark l's x, y
EKF_LINEAR_LMAX = 16              # update_linear: landmarks of the sub-state
EKF_LINEAR_ROWS = 32              # update_linear: measurement rows per trajectory
EKF_FLAG_NONFINITE = 1
EKF_FLAG_ASSOC = 2
EKF_FLAG_INTERNAL = 4             # a bounded wait of a single-launch step timed out: sync()/state()/mean() raise EkfError
EKF_N_MAX_LIMIT = 21823           # largest n_max (one covariance stays below 4 GiB: 32-bit byte offsets in the kernels)
EKF_DMAX = 256                    # detections per window the device front end takes
EKF_AMAX = 32                     # distinct tags per window the device front end takes (two update passes of EKF_MMAX)
EKF_TAGMAX = 1024


class EkfError(RuntimeError):
    """A C-ABI call returned a non-zero status (message from ``ekf_last_error``)."""


class _CConfig(C.Structure):
    _fields_ = [("motion_sigma", C.c_double), ("meas_sigma", C.c_double), ("arc_threshold", C.c_double),
                ("landmark_init_var", C.c_double), ("enable_measurement_model", C.c_int),
                ("enable_circular_interpolation", C.c_int), ("disable_motion_model", C.c_int),
                ("reserved", C.c_int)]


@dataclasses.dataclass
class EkfConfig:
    """The reference's module constants (src/replay_no_ros.py:15-36) as explicit fields."""
    motion_sigma: float = 0.1                  # MOTION_MODEL_VARIANCE
    meas_sigma: float = 0.7                    # MEASUREMENT_MODEL_VARIANCE
    arc_threshold: float = 1e-2                # :376
    landmark_init_var: float = 10000.0         # :356
    enable_measurement_model: bool = True      # ENABLE_MEASUREMENT_MODEL
    enable_circular_interpolation: bool = True  # ENABLE_CIRCULAR_INTERPOLATION
    disable_motion_model: bool = False         # DISABLE_MOTION_MODEL
    gate_range: float = 1.5                    # :289 (host side)
    ignore_tags: tuple = ()                    # IGNORE_TAGS (host side)

    def _c(self) -> _CConfig:
        return _CConfig(self.motion_sigma, self.meas_sigma, self.arc_threshold, self.landmark_init_var,
                        int(self.enable_measurement_model), int(self.enable_circular_interpolation),
                        int(self.disable_motion_model), 0)


def library_path() -> str:
    """The in-tree library."""
    if os.environ.get("EKFSLAM_HIP_VARIANT"):
        raise EkfError("EKFSLAM_HIP_VARIANT is set, but diagnostic builds of the library no longer exist: "
                       "unset it to load the product library")
    return os.path.join(_HERE, _LIB_NAME)


def build_library(force: bool = False) -> str:
    """Compile the HIP sources for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    path = library_path()
    srcdir = os.path.join(_HERE, "csrc")
    if force:
        subprocess.run(["make", "-C", srcdir, "clean"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", srcdir, "-j4"], check=True, stdout=subprocess.DEVNULL)
    if not os.path.exists(path):
        raise EkfError("build did not produce " + path)
    return path


_lib = None
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)

# name -> (restype, argtypes): every symbol include/ekfslam_hip.h declares
ABI = {
    "ekf_config_default": (C.c_int, [C.POINTER(_CConfig)]),
    "ekf_device_count": (C.c_int, [_ip]),
    "ekf_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(_CConfig), C.POINTER(C.c_void_p)]),
    "ekf_destroy": (C.c_int, [C.c_void_p]),
    "ekf_upload_state": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, C.c_int]),
    "ekf_upload_state_diag": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, C.c_int]),
    "ekf_download_state": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, C.c_int]),
    "ekf_download_mean": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_int]),
    "ekf_download_block": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp]),
    "ekf_download_marginals": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, C.c_int, _ip]),
    "ekf_associate": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _ip, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp, C.c_int]),
    "ekf_download_joint": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _ip, _ip, C.c_int, _dp, _dp]),
    "ekf_factor": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _ip]),
    "ekf_factor_solve": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp]),
    "ekf_factor_multiply": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, C.c_int, C.c_int, _dp]),
    "ekf_download_factor": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_int]),
    "ekf_factor_release": (C.c_int, [C.c_void_p]),
    "ekf_update_direct": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _ip, _dp, _dp, _ip, C.c_int, _dp, _dp, _ip, _ip]),
    "ekf_update_linear": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _ip, _ip, C.c_int, _dp, _dp, _dp, _ip, C.c_int, C.c_int, _dp, _dp, _ip]),
    "ekf_state_size": (C.c_int, [C.c_void_p, C.c_int, _ip]),
    "ekf_log_innovations": (C.c_int, [C.c_void_p, C.c_int]),
    "ekf_innovation_steps": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)]),
    "ekf_download_innovations": (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, _ip, _ip, _dp, _dp, _dp]),
    "ekf_log_poses": (C.c_int, [C.c_void_p, C.c_int]),
    "ekf_pose_steps": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)]),
    "ekf_download_poses": (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, _dp, _dp]),
    "ekf_set_nis_gate": (C.c_int, [C.c_void_p, C.c_double]),
    "ekf_download_gate_counts": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_longlong)]),
    "ekf_download_innovation_rejections": (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, _ip]),
    "ekf_set_noise": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp]),
    "ekf_get_noise": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp]),
    "ekf_add_landmarks": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, C.c_int]),
    "ekf_remove_landmarks": (C.c_int, [C.c_void_p, C.c_int, _ip, C.c_int]),
    "ekf_copy_trajectories": (C.c_int, [C.c_void_p, _ip, C.c_void_p, _ip, C.c_int]),
    "ekf_join_maps": (C.c_int, [C.c_void_p, _ip, C.c_void_p, _ip, C.c_int, _dp, _dp, _ip, _ip, C.c_int]),
    "ekf_transform": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp]),
    "ekf_predict": (C.c_int, [C.c_void_p, _dp, _dp]),
    "ekf_predict_linear": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, _ip]),
    "ekf_update": (C.c_int, [C.c_void_p, _ip, _dp, _dp, _ip, C.c_int]),
    "ekf_step": (C.c_int, [C.c_void_p, _dp, _dp, _ip, _dp, _dp, _ip, C.c_int]),
    "ekf_localize_step": (C.c_int, [C.c_void_p, _dp, _dp, _ip, _dp, _dp, _ip, C.c_int]),
    "ekf_localize_update": (C.c_int, [C.c_void_p, _ip, _dp, _dp, _ip, C.c_int]),
    "ekf_localize_run": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "ekf_host_alloc": (C.c_void_p, [C.c_size_t]),
    "ekf_host_free": (None, [C.c_void_p]),
    "ekf_step_fetch": (C.c_int, [C.c_void_p, _dp, _dp, _ip, _dp, _dp, _ip, C.c_int, C.c_int, _dp, _dp, C.c_int]),
    "ekf_set_association": (C.c_int, [C.c_void_p, C.c_double, _ip, C.c_int]),
    "ekf_step_detections": (C.c_int, [C.c_void_p, _dp, _dp, _ip, _ip, _dp, _dp, C.c_int]),
    "ekf_download_tags": (C.c_int, [C.c_void_p, C.c_int, _ip, _ip, _ip, _dp, _dp, _dp, _dp, _dp]),
    "ekf_download_tag_index": (C.c_int, [C.c_void_p, C.c_int, _ip, C.c_int, _ip]),
    "ekf_upload_tag_index": (C.c_int, [C.c_void_p, C.c_int, _ip, C.c_int]),
    "ekf_localize_detections": (C.c_int, [C.c_void_p, _dp, _dp, _ip, _ip, _dp, _dp, C.c_int]),
    "ekf_download_unmatched": (C.c_int, [C.c_void_p, C.c_int, _ip, _ip, C.c_int]),
    "ekf_hyp_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "ekf_hyp_destroy": (C.c_int, [C.c_void_p]),
    "ekf_hyp_reset": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp]),
    "ekf_hyp_step": (C.c_int, [C.c_void_p, _dp, _dp, C.c_int, _ip, _dp, _dp, _ip, C.c_int, C.c_int]),
    "ekf_hyp_update": (C.c_int, [C.c_void_p, _ip, _dp, _dp, _ip, C.c_int, C.c_int]),
    "ekf_hyp_download": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong),
                                   C.POINTER(C.c_uint)]),
    "ekf_hyp_download_rows": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_int]),
    "ekf_hyp_set_nis_gate": (C.c_int, [C.c_void_p, C.c_double]),
    "ekf_hyp_adopt": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "ekf_hyp_sync": (C.c_int, [C.c_void_p]),
    "ekf_hyp_last_error": (C.c_char_p, [C.c_void_p]),
    "ekf_hypotheses_weigh": (C.c_int, [C.c_void_p, _dp, _dp, _ip]),
    "ekf_hypotheses_resample": (C.c_int, [C.c_void_p, C.c_double, C.c_double, _dp, _ip, _ip, _dp, _dp]),
    "ekf_hypotheses_stream_upload": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, C.c_int, _ip, _dp, _dp, _ip, C.c_int, C.c_int]),
    "ekf_hypotheses_run": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, _dp, _dp]),
    "ekf_hypotheses_mixture": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _dp, _ip, _ip]),
    "ekf_hypotheses_log": (C.c_int, [C.c_void_p, C.c_int]),
    "ekf_hypotheses_log_steps": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)]),
    "ekf_hypotheses_download_log": (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, _ip]),
    "ekf_hypotheses_set_association": (C.c_int, [C.c_void_p, C.c_double, _ip, C.c_int]),
    "ekf_hypotheses_step_detections": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_int, _ip, _dp, _dp]),
    "ekf_hypotheses_detections_upload": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _ip, _ip, _dp, _dp, C.c_int]),
    "ekf_hypotheses_download_tags": (C.c_int, [C.c_void_p, C.c_int, _ip, _ip, _ip, _dp, _dp, _dp, _ip, _ip, C.POINTER(C.c_uint)]),
    "ekf_hypotheses_associate": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp, C.c_int]),
    "ekf_hypotheses_step_unlabelled": (C.c_int, [C.c_void_p, _dp, _dp, C.c_int, _dp, _dp, C.c_int, C.c_double, C.c_double]),
    "ekf_hypotheses_update_unlabelled": (C.c_int, [C.c_void_p, _dp, _dp, C.c_int, C.c_double, C.c_double]),
    "ekf_hypotheses_download_assignment": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _ip]),
    "ekf_stream_upload": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _ip, _dp, _dp, _ip, C.c_int]),
    "ekf_stream_run": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "ekf_run_stream": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _ip, _dp, _dp, _ip, C.c_int]),
    "ekf_predict_dense": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp]),
    "ekf_flush": (C.c_int, [C.c_void_p]),
    "ekf_sync": (C.c_int, [C.c_void_p]),
    "ekf_status_flags": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint)]),
    "ekf_last_error": (C.c_char_p, [C.c_void_p]),
    "ekf_timer_begin": (C.c_int, [C.c_void_p]),
    "ekf_timer_end": (C.c_int, [C.c_void_p, _dp]),
    "ekf_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "ekf_profile_read": (C.c_int, [C.c_void_p, _dp, C.POINTER(C.c_longlong)]),
    "ekf_profile_passes": (C.c_longlong, [C.c_void_p]),
    "ekf_profile_read_class": (C.c_int, [C.c_void_p, C.c_int, _dp, C.POINTER(C.c_longlong)]),
    "ekf_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "ekf_last_pass": (C.c_int, [C.c_void_p, _ip, _ip, _ip]),
    # diagnostics (the header's last section)
    "ekf_debug_cadences": (C.c_int, [C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "ekf_debug_lookaheads": (C.c_long, [C.c_void_p]),
    "ekf_debug_chained": (C.c_long, [C.c_void_p]),
    "ekf_debug_assoc_fallbacks": (C.c_long, [C.c_void_p]),
    "ekf_debug_w_from_v": (C.c_long, [C.c_void_p]),
    "ekf_debug_last_pass_wv": (C.c_int, [C.c_void_p]),
    "ekf_debug_note_assoc_fallback": (None, [C.c_void_p]),
    "ekf_debug_last_pass_shares": (C.c_int, [C.c_void_p]),
    "ekf_debug_small_launches": (C.c_long, [C.c_void_p]),
    "ekf_debug_fused_fetches": (C.c_long, [C.c_void_p]),
    "ekf_debug_dense_packs": (C.c_long, [C.c_void_p]),
    "ekf_debug_fetch_retries": (C.c_long, [C.c_void_p]),
    "ekf_debug_cad": (C.c_long, [C.c_void_p, C.c_int, C.c_void_p, C.c_long]),
    "ekf_debug_snapshot": (C.c_long, [C.c_void_p, C.c_int, C.c_int, _dp, C.c_long]),
    "ekf_debug_pass_units": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _ip, C.c_int]),
    "ekf_debug_pass_shares": (C.c_int, [C.c_int, C.c_int, C.c_int, _ip]),
    "ekf_debug_hyp_score_time": (C.c_int, [C.c_void_p, _dp, _dp, C.c_int, C.c_int, _dp]),
}


def load_library():
    """dlopen the in-tree library and type every entry point.  Raises EkfError if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise EkfError(f"{path} not found: build it with __graft_entry__.build() or `make -C "
                       f"{os.path.join(_HERE, 'csrc')}` -- there is no CPU fallback")
    try:
        lib = C.CDLL(path)
    except OSError as e:
        raise EkfError(f"cannot load {path}: {e}") from e
    for name, (res, args) in ABI.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def device_count() -> int:
    """Number of HIP devices visible to this process (0 without a GPU)."""
    n = C.c_int(0)
    load_library().ekf_device_count(C.byref(n))
    return n.value


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != tuple(shape):
        raise ValueError(f"expected shape {shape}, got {a.shape}")
    return a


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _p(a, typ=_dp):
    return a.ctypes.data_as(typ)


def _pack_windows(windows):
    """Windows of raw detections -- each the reference's ``[(timestamp, [tag, ...])]`` list -- with their frames concatenated in
    order, into the arrays the detection entries take: (count (W,), tag ids (W, stride), pose_t (W, stride, 3), pose_err
    (W, stride), stride), padded to the longest window (stride >= 1)."""
    flat = [[tag for _stamp, tags in win for tag in tags] for win in windows]
    count = np.array([len(w) for w in flat], dtype=np.int32)
    stride = max(1, int(count.max())) if len(flat) else 1
    ids = np.zeros((len(flat), stride), dtype=np.int32)
    pt = np.zeros((len(flat), stride, 3))
    pe = np.zeros((len(flat), stride))
    for b, w in enumerate(flat):
        for i, tag in enumerate(w):
            ids[b, i] = tag.tag_id
            pt[b, i] = np.asarray(tag.pose_t, dtype=np.float64).ravel()[:3]
            pe[b, i] = tag.pose_err
    return count, ids, pt, pe, stride


def compose_pose(pose, delta):
    """``pose (+) delta``: the pose after a motion increment ``delta = (dx, dy, dtheta)`` given in the robot frame of ``pose =
    (x, y, theta)`` -- what wheel or visual odometry reports --, theta wrapped to [-pi, pi) (``evaluation.wrap_angle``'s
    convention).  Returns ``(new pose (3,), F (3, 3), J (3, 3))`` with ``F = d(new pose)/d(pose)`` and ``J = d(new pose)/d(delta)
    = diag(R(theta), 1)``: the process noise of an increment with covariance ``cov`` is ``J cov J^T``."""
    x, y, th = (float(v) for v in np.asarray(pose, dtype=np.float64).reshape(3))
    dx, dy, dth = (float(v) for v in np.asarray(delta, dtype=np.float64).reshape(3))
    c, s = math.cos(th), math.sin(th)
    new = np.array([x + c * dx - s * dy, y + s * dx + c * dy, (th + dth + np.pi) % (2.0 * np.pi) - np.pi])
    F = np.array([[1.0, 0.0, -s * dx - c * dy], [0.0, 1.0, c * dx - s * dy], [0.0, 0.0, 1.0]])
    J = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return new, F, J


_SMALL_OUT_N = 131        # (PACK_SMALL_N of csrc/ekf_api.hip: states the library hands over through one pinned buffer)


class _PinnedPool:
    """Recycled pinned host buffers behind the LARGE arrays handed to the caller (covariances beyond 131 x 131).

    The reference's loop gets a fresh covariance from every call (src/replay_no_ros.py:229-237).  A fresh ``np.empty`` of
    128 MB (N = 2000) is 32 768 untouched pages: the download faults them in and pins them (5 ms on top of 2.3 ms of PCIe
    time) and dropping the previous array unmaps as many (another 5 ms).  Here the array is a view of a buffer from
    ``ekf_host_alloc``; the buffer comes back to the pool when the LAST view of it is gone (the ctypes object every view's
    ``base`` chain ends in is what the finaliser watches), and is handed out again for the next array of that size.
    Beyond ``LIMIT`` bytes of live buffers -- a caller that keeps every covariance -- arrays are ordinary ``np.empty``."""
    LIMIT = 2 << 30
    KEEP = 2                      # free buffers kept per size (the loop holds one array while the next is filled)

    def __init__(self):
        self.free = collections.OrderedDict()      # size -> free buffers of that size, least recently used size first
        self.live = 0                              # bytes allocated (handed out + free)
        # handles may be driven from several host threads (one each); finalisers run wherever the last reference dies,
        # possibly inside empty() of the same thread: a re-entrant lock
        self.lock = threading.RLock()

    def _evict(self, need):
        """(under the lock) Free buffers, least recently used size first, until `need` more bytes fit LIMIT; returns the
        pointers to free -- outside the lock: hipHostFree synchronises the device."""
        out = []
        for size in list(self.free):
            while self.free[size] and self.live + need > self.LIMIT:
                out.append(self.free[size].pop())
                self.live -= size
            if not self.free[size]:
                del self.free[size]
            if self.live + need <= self.LIMIT:
                break
        return out

    def empty(self, lib, shape):
        count = int(np.prod(shape))
        nbytes = 8 * count
        ptr, evicted = None, []
        with self.lock:
            kept = self.free.get(nbytes)
            if kept:
                ptr = kept.pop()
                self.free.move_to_end(nbytes)
            else:
                # buffers of OTHER sizes stay (two handles of different size, a map that grows a landmark at a time): they
                # go only when this allocation would not fit LIMIT otherwise
                if self.live + nbytes > self.LIMIT:
                    evicted = self._evict(nbytes)
                if self.live + nbytes <= self.LIMIT:
                    self.live += nbytes                # (reserved; the allocation itself happens outside the lock)
                    ptr = -1
        for q in evicted:
            lib.ekf_host_free(q)
        if ptr == -1:
            ptr = lib.ekf_host_alloc(nbytes)
            if not ptr:
                with self.lock:
                    self.live -= nbytes
        if not ptr:
            return np.empty(shape)
        buf = (C.c_double * count).from_address(ptr)
        weakref.finalize(buf, self._release, lib, ptr, nbytes).atexit = False
        return np.frombuffer(buf, dtype=np.float64).reshape(shape)

    def _release(self, lib, ptr, nbytes):
        drop = False
        with self.lock:
            kept = self.free.setdefault(nbytes, [])
            self.free.move_to_end(nbytes)
            if len(kept) < self.KEEP:
                kept.append(ptr)
            else:
                drop = True
                self.live -= nbytes
        if drop:
            lib.ekf_host_free(ptr)


_pinned = _PinnedPool()


class Innovations(typing.NamedTuple):
    """What ``EkfSlam.innovations()`` returns: K logged steps of a bank of B trajectories, W entries per step (NaN / -1
    beyond a step's m)."""
    steps: np.ndarray     # (K,)        step numbers since the log was switched on
    m: np.ndarray         # (K, B)      landmark updates each step applied (its true count, even beyond EKF_AMAX)
    idx: np.ndarray       # (K, B, W)   landmark index of each update, in application order
    y: np.ndarray         # (K, B, W, 2)     innovation
    S: np.ndarray         # (K, B, W, 2, 2)  innovation covariance
    nis: np.ndarray       # (K, B, W)   y^T S^-1 y
    rejected: Optional[np.ndarray] = None   # (K, B, W) 1: the NIS gate rejected the update, 0: applied, -1 beyond m


class PoseTrace(typing.NamedTuple):
    """What ``EkfSlam.poses()`` returns: T logged steps of a bank of B trajectories, each row the state AFTER its step."""
    first: int            # step number of row 0 since the log was switched on
    mean: np.ndarray      # (T, B, 3)     x, y, theta
    cov: np.ndarray       # (T, B, 3, 3)  the pose block P[0:3, 0:3], exactly symmetric


class Associations(typing.NamedTuple):
    """What ``EkfSlam.associate()`` returns for a bank of B trajectories with up to S observations each (rows beyond a
    trajectory's m, and trajectories without landmarks: -1 / NaN)."""
    cand: np.ndarray      # (B, S, 2)  int32: the landmarks of the two smallest scores d = NIS + ln det S, best first
    nis: np.ndarray       # (B, S, 2)  their NIS = y^T S^-1 y
    logdet: np.ndarray    # (B, S, 2)  their ln det S
    min_nis: np.ndarray   # (B, S)     the smallest NIS over ALL landmarks
    all_nis: Optional[np.ndarray] = None      # (B, S, N_hi)  with full=True: every landmark's NIS (NaN beyond the map)
    all_logdet: Optional[np.ndarray] = None   # (B, S, N_hi)  ... and ln det S


class HypothesisAssociations(typing.NamedTuple):
    """What ``HypothesisBank.associate()`` returns for K hypotheses and one list of m observations (-1 / NaN where the map is
    empty or every score is NaN)."""
    cand: np.ndarray      # (K, m, 2)  int32: the landmarks of the two smallest scores d = NIS + ln det S, best first
    nis: np.ndarray       # (K, m, 2)  their NIS = y^T S^-1 y
    logdet: np.ndarray    # (K, m, 2)  their ln det S
    min_nis: np.ndarray   # (K, m)     the smallest NIS over ALL landmarks
    all_nis: Optional[np.ndarray] = None      # (K, m, N)  with full=True: every landmark's NIS
    all_logdet: Optional[np.ndarray] = None   # (K, m, N)  ... and ln det S


class DirectUpdate(typing.NamedTuple):
    """What ``update_direct`` reports per trajectory of the bank: the joint NIS y^T S^-1 y of its fixes, their stacked row
    count D (the NIS's degrees of freedom) and whether they were applied (False: rejected by the gate or a singular S, or
    the trajectory brought no fix)."""
    nis: np.ndarray        # (B,)
    dof: np.ndarray        # (B,) int32
    applied: np.ndarray    # (B,) bool


class LinearUpdate(typing.NamedTuple):
    """What ``update_linear`` reports per trajectory of the bank: the joint NIS y^T S^-1 y of its rows, their number D (the
    NIS's degrees of freedom) and whether they were applied (False: rejected by the gate or a singular S, or the trajectory
    brought no row)."""
    nis: np.ndarray        # (B,)
    dof: np.ndarray        # (B,) int32
    applied: np.ndarray    # (B,) bool


class MapJoin(typing.NamedTuple):
    """What ``EkfSlam.join`` reports per pair (scalars and one row for a single pair given as ints): the landmark index of the
    first appended landmark, the number appended, and per source landmark the destination landmark that already carried
    its tag (-1: none -- the appended landmark then keeps the tag)."""
    first: np.ndarray      # (k,) int32
    count: np.ndarray      # (k,) int32
    twins: np.ndarray      # (k, N_B hi) int32, -1 beyond a source's landmarks


class HypothesisResampling(typing.NamedTuple):
    """What ``HypothesisBank.resample`` reports: per slot the hypothesis it now holds (``ancestors[k] == k``: a survivor, in
    place) and per hypothesis its number of offspring, the effective sample size of the weights that were resampled and the
    bank's evidence ``logmean`` (every hypothesis's log-likelihood afterwards)."""
    ancestors: np.ndarray  # (count,) int32
    offspring: np.ndarray  # (count,) int32
    ess: float
    logmean: float


class HypothesisMixture(typing.NamedTuple):
    """What ``HypothesisBank.mixture`` returns: ``evaluation.MixturePose``'s mean and covariance, formed on the device (the
    weights stay there), and what the weights say of the bank.  A bank in which nothing weighs: NaN, ess 0, evidence -inf,
    best -1."""
    mean: np.ndarray       # (3,) the weighted mean pose, the heading averaged on the circle
    cov: np.ndarray        # (3, 3) sum w (P_k + d_k d_k^T), exactly symmetric
    ess: float
    evidence: float
    live: int
    best: int              # the first hypothesis with the largest log-likelihood that weighs


class HypothesisTrace(typing.NamedTuple):
    """What ``HypothesisBank.trace`` returns: T logged steps of ``run``, each row the bank's mixture behind the step's update
    and BEFORE its resampling -- the exact posterior summary; a resampling keeps it only in expectation."""
    mean: np.ndarray       # (T, 3)
    cov: np.ndarray        # (T, 3, 3)
    ess: np.ndarray        # (T,)
    evidence: np.ndarray   # (T,)
    live: np.ndarray       # (T,) int32
    best: np.ndarray       # (T,) int32
    resampled: np.ndarray  # (T,) bool: the step's resampling acted
    first: int = 0         # step number of row 0 since the log was switched on


EKF_FACTOR_RHS = 16       # (include/ekfslam_hip.h)


class CovFactor:
    """The Cholesky factor P = U^T U of a range of trajectories, as ``EkfSlam.factor`` left it on the device: a snapshot,
    which later filter calls neither change nor invalidate.  ``logdet`` (count,) = ln det P, ``info`` (count,) as LAPACK
    dpotrf (0: positive definite; i > 0: the leading minor of order i is not -- every result of that trajectory is NaN),
    ``n`` (count,) the state sizes and ``means`` the means at factor time.  Made for one trajectory (``factor(b)``) the
    methods take and return that trajectory's arrays without the leading axis.

    A newer ``factor()`` or ``release_factor()`` of the same filter replaces the factor on the device: every method of
    this object then raises ``EkfError``."""

    def __init__(self, owner, generation, b0, count, single, logdet, info, n, means):
        self._owner, self._generation, self._b0, self._count, self._single = owner, generation, b0, count, single
        self.logdet, self.info, self.n, self.means = logdet, info, n, means

    def _live(self):
        if self._owner._factor_generation != self._generation:
            raise EkfError("this CovFactor has been replaced by a newer factor() or release_factor() of its filter")

    def _apply(self, x, which):
        """x: (count, k, n_hi) (or (count, n_hi); one trajectory: (k, n) or (n,)) -> the same shape through ekf_factor_solve
        (`which` = "white" / "quad") or ekf_factor_multiply ("mul"), EKF_FACTOR_RHS columns per call."""
        self._live()
        o = self._owner
        x = np.asarray(x, dtype=np.float64)
        if self._single:
            x = x[None]
        vec = x.ndim == 2
        if vec:
            x = x[:, None, :]
        stride = int(self.n.max())
        if x.ndim != 3 or x.shape[0] != self._count or x.shape[2] != stride:
            raise ValueError(f"expected {self._count} trajectories of vectors of length {stride}, got {x.shape}")
        k = x.shape[1]
        out = np.empty((self._count, k) if which == "quad" else x.shape)
        for k0 in range(0, k, EKF_FACTOR_RHS):
            part = np.ascontiguousarray(x[:, k0:k0 + EKF_FACTOR_RHS])
            nr = part.shape[1]
            res = np.empty(part.shape)
            if which == "mul":
                o._check(o._lib.ekf_factor_multiply(o._h, self._b0, self._count, _p(part), nr, stride, _p(res)))
            else:
                quad = np.empty((self._count, nr))
                o._check(o._lib.ekf_factor_solve(o._h, self._b0, self._count, _p(part), nr, stride,
                                                 _p(res) if which == "white" else None, _p(quad)))
                if which == "quad":
                    res = quad
            out[:, k0:k0 + nr] = res
        if vec:
            out = out[:, 0]
        return out[0] if self._single else out

    def whiten(self, e):
        """U^-T e: white noise of unit covariance if e ~ N(0, P).  Entries beyond a trajectory's n are NaN."""
        return self._apply(e, "white")

    def mahalanobis(self, e):
        """e^T P^-1 e per trajectory (and per vector)."""
        return self._apply(e, "quad")

    def multiply(self, z):
        """U^T z: covariance P for z ~ N(0, I)."""
        return self._apply(z, "mul")

    def upper(self, b: int = 0) -> np.ndarray:
        """U of trajectory b (an index of the bank), n x n, zeros below the diagonal."""
        self._live()
        o = self._owner
        if not self._b0 <= b < self._b0 + self._count:
            raise ValueError("trajectory outside the factored range")
        n = int(self.n[b - self._b0])
        out = np.empty((n, n))
        o._check(o._lib.ekf_download_factor(o._h, int(b), _p(out), n))
        return out

    def sample(self, k: int, rng=None):
        """k draws from N(mean, P) per trajectory: mean + U^T z, (count, k, n_hi) with NaN beyond a trajectory's n (one
        trajectory: (k, n))."""
        self._live()
        rng = np.random.default_rng() if rng is None else rng
        stride = int(self.n.max())
        z = rng.standard_normal((self._count, int(k), stride))
        means = np.full((self._count, 1, stride), np.nan)
        for bi in range(self._count):
            means[bi, 0, :self.n[bi]] = self.means[bi]
        draws = (z[0] if self._single else z)
        out = self.multiply(draws)
        return out + (means[0] if self._single else means)


class HypothesisBank:
    """``count`` pose hypotheses localising on ONE frozen map (``EkfSlam.hypotheses``; ``ekf_hyp_*``): the map -- a snapshot of a
    slot's landmark means and of every P[a, b] with a, b >= 3 -- is stored once, a hypothesis is its pose mean, pose block and
    pose rows P[0:3, :].  Every hypothesis steps with ``EkfSlam.localize``'s arithmetic and ends with ``localize``'s bits;
    each accumulates the log-likelihood of its innovations on the device.  Stepping calls are asynchronous on the bank's stream;
    the reads block.  Close it (or use it as a context manager) to release the device memory."""

    def __init__(self, lib, handle, count: int, n: int):
        self._lib, self._h = lib, handle
        self.count, self.n = int(count), int(n)

    # -- plumbing ------------------------------------------------------------------------------
    def _live(self):
        if not (getattr(self, "_h", None) and self._h.value):
            raise EkfError("the hypothesis bank has been closed")
        return self._h

    def _check(self, rc: int):
        if rc != 0:
            raise EkfError(f"status {rc}: {self._lib.ekf_hyp_last_error(self._h).decode()}")

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.ekf_hyp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _motion(self, lin, ang):
        """(lin, ang, motion_stride): scalars are shared by every hypothesis, arrays of ``count`` give one pair each."""
        lin, ang = np.atleast_1d(_f64(lin)).ravel(), np.atleast_1d(_f64(ang)).ravel()
        if len(lin) == 1 and len(ang) == 1:
            return lin, ang, 0
        lin, ang = np.broadcast_to(lin, (self.count,)).copy(), np.broadcast_to(ang, (self.count,)).copy()
        return lin, ang, 1

    def _obs(self, idx, ranges, bearings):
        """(idx, ranges, bearings, m, obs_stride) as padded 2-D arrays: one flat list is shared by every hypothesis; a list of
        ``count`` lists (or [count, m] arrays) gives one list each."""
        shared = len(idx) == 0 or np.ndim(idx[0]) == 0
        lists = [(idx, ranges, bearings)] if shared else list(zip(idx, ranges, bearings))
        if not shared and len(lists) != self.count:
            raise ValueError(f"observations: one list for all, or {self.count} lists expected")
        lens = [len(i) for i, _, _ in lists]
        I = np.zeros((len(lists), max(1, max(lens))), dtype=np.int32)
        R, B = np.zeros(I.shape), np.zeros(I.shape)
        for k, (i, r, b) in enumerate(lists):
            if len(r) != lens[k] or len(b) != lens[k]:
                raise ValueError("idx / ranges / bearings lengths differ")
            I[k, :lens[k]], R[k, :lens[k]], B[k, :lens[k]] = i, r, b
        return I, R, B, np.asarray(lens, dtype=np.int32), 0 if shared else 1

    def _passes(self, I, R, B, m):
        """The padded lists cut into passes of at most EKF_MMAX observations (the library takes one pass per call)."""
        for lo in range(0, max(1, int(m.max())), EKF_MMAX):
            mp = np.clip(m - lo, 0, EKF_MMAX).astype(np.int32)
            w = max(1, int(mp.max()))
            yield (np.ascontiguousarray(I[:, lo:lo + w]), np.ascontiguousarray(R[:, lo:lo + w]),
                   np.ascontiguousarray(B[:, lo:lo + w]), mp, w)

    # -- the filter ----------------------------------------------------------------------------
    def step(self, lin, ang, idx, ranges, bearings):
        """``EkfSlam.localize`` for every hypothesis.  ``lin`` / ``ang``: scalars (one motion for all) or ``count`` values;
        observations: one flat list for all (tags carry their ids: the common case) or one list per hypothesis.  More than
        EKF_MMAX observations run as a step plus update-only calls, as ``localize`` runs them."""
        h = self._live()
        lin, ang, ms = self._motion(lin, ang)
        I, R, B, m, os_ = self._obs(idx, ranges, bearings)
        for p, (Ip, Rp, Bp, mp, w) in enumerate(self._passes(I, R, B, m)):
            if p == 0:
                self._check(self._lib.ekf_hyp_step(h, _p(lin), _p(ang), ms, _p(Ip, _ip), _p(Rp), _p(Bp), _p(mp, _ip), w, os_))
            else:
                self._check(self._lib.ekf_hyp_update(h, _p(Ip, _ip), _p(Rp), _p(Bp), _p(mp, _ip), w, os_))

    def update(self, idx, ranges, bearings):
        """``EkfSlam.localize_update`` for every hypothesis (observations as for ``step``)."""
        h = self._live()
        I, R, B, m, os_ = self._obs(idx, ranges, bearings)
        for Ip, Rp, Bp, mp, w in self._passes(I, R, B, m):
            self._check(self._lib.ekf_hyp_update(h, _p(Ip, _ip), _p(Rp), _p(Bp), _p(mp, _ip), w, os_))

    def reset(self, poses, cov, k=None):
        """``EkfSlam.reset_pose`` for hypotheses: pose means ``poses`` ((count, 3), or one for all), pose blocks ``cov`` ((3, 3)
        for all, or (count, 3, 3)), every pose-landmark cross term dropped, log-likelihood and counters cleared.  ``k`` None:
        the whole bank; an int: that hypothesis; (k0, count): a range."""
        h = self._live()
        k0, cnt = (0, self.count) if k is None else ((int(k), 1) if np.ndim(k) == 0 else (int(k[0]), int(k[1])))
        poses = np.ascontiguousarray(np.broadcast_to(_f64(poses), (max(cnt, 0), 3)))
        cov = np.ascontiguousarray(np.broadcast_to(_f64(cov), (max(cnt, 0), 3, 3)))
        self._check(self._lib.ekf_hyp_reset(h, k0, cnt, _p(poses), _p(cov)))

    def _download(self):
        h = self._live()
        K = self.count
        pose, cov, ll = np.empty((K, 3)), np.empty((K, 3, 3)), np.empty(K)
        nobs, nrej, fl = np.empty(K, dtype=np.int64), np.empty(K, dtype=np.int64), np.empty(K, dtype=np.uint32)
        self._check(self._lib.ekf_hyp_download(h, 0, K, _p(pose), _p(cov), _p(ll), _p(nobs, C.POINTER(C.c_longlong)),
                                               _p(nrej, C.POINTER(C.c_longlong)), _p(fl, C.POINTER(C.c_uint))))
        return pose, cov, ll, nobs, nrej, fl

    def poses(self):
        """(mean (count, 3), cov (count, 3, 3)) of every hypothesis."""
        pose, cov = self._download()[:2]
        return pose, cov

    @property
    def loglik(self) -> np.ndarray:
        """Per hypothesis, the Gaussian log-likelihood of every innovation it has seen since its seed or last reset, gated out
        or not: the sum ``evaluation.nis_consistency`` forms from an innovation log."""
        return self._download()[2]

    @property
    def observed(self) -> np.ndarray:
        return self._download()[3]

    @property
    def rejected(self) -> np.ndarray:
        """Per hypothesis, the observations the NIS gate rejected (``EkfSlam.gate_counts`` of a slot)."""
        return self._download()[4]

    def flags(self) -> np.ndarray:
        return self._download()[5]

    def rows(self, k: int) -> np.ndarray:
        """Hypothesis k's P[0:3, :] (3, n): the pose block, then the pose-landmark cross terms."""
        out = np.empty((3, self.n))
        self._check(self._lib.ekf_hyp_download_rows(self._live(), int(k), _p(out), self.n))
        return out

    @staticmethod
    def weights_of(loglik) -> np.ndarray:
        """exp(loglik - max), normalised: the posterior weights of hypotheses with equal priors.  -inf and NaN weigh nothing;
        with no finite log-likelihood (or a +inf) the weight is shared equally among the largest."""
        ll = np.asarray(loglik, dtype=np.float64)
        ll = np.where(np.isnan(ll), -np.inf, ll)
        top = ll.max() if ll.size else 0.0
        w = (ll == top).astype(np.float64) if np.isinf(top) else np.exp(ll - top)
        return w / w.sum() if ll.size else w

    def weights(self) -> np.ndarray:
        return self.weights_of(self.loglik)

    def best(self) -> int:
        """The hypothesis with the largest log-likelihood (the first of equals)."""
        return int(np.argmax(self.weights()))

    # -- weights and resampling on the device ---------------------------------------------------
    def _weigh(self):
        ess, logmean, live = C.c_double(), C.c_double(), C.c_int()
        self._check(self._lib.ekf_hypotheses_weigh(self._live(), C.byref(ess), C.byref(logmean), C.byref(live)))
        return ess.value, logmean.value, live.value

    def ess(self) -> float:
        """The effective sample size (sum w)^2 / sum w^2 of the weights, formed on the device (``ekf_hypotheses_weigh``): unlike
        ``weights``, a hypothesis whose sticky non-finite flag is set weighs nothing.  0 where nothing weighs."""
        return self._weigh()[0]

    def evidence(self) -> float:
        """max + ln sum exp(loglik - max) - ln count: the log of the mean likelihood, the bank's evidence under equal priors
        (-inf where nothing weighs)."""
        return self._weigh()[1]

    def live(self) -> int:
        """The hypotheses with a weight above zero."""
        return self._weigh()[2]

    def resample(self, u=None, split: float = 0.0, z=None, rng=None) -> HypothesisResampling:
        """Systematic resampling on the device (``ekf_hypotheses_resample``) with the offset ``u`` in [0, 1): survivors stay in
        place, dead slots take the surplus offspring's pose, block, rows and counters bit for bit, and every log-likelihood
        becomes the bank's evidence.  ``split`` = s in (0, 1) spreads the copies: every slot of an ancestor with two or more
        offspring moves its pose by ``s L z[k]`` (L L^T = its pose block) and keeps ``1 - s^2`` of its block and rows, so that
        the children's mixture has the ancestor's pose marginal.  ``u`` and ``z`` ((count, 3) standard normal) are drawn from
        ``rng`` (default ``np.random.default_rng()``) where they are not given.  Blocking."""
        h = self._live()
        split = float(split)
        if (u is None or (split > 0.0 and z is None)) and rng is None:
            rng = np.random.default_rng()
        u = float(rng.random()) if u is None else float(u)
        if z is not None:                                  # (given without a split: the library refuses it)
            z = np.ascontiguousarray(np.broadcast_to(_f64(z), (self.count, 3)))
        elif split > 0.0:
            z = rng.standard_normal((self.count, 3))
        anc, off = np.empty(self.count, dtype=np.int32), np.empty(self.count, dtype=np.int32)
        ess, logmean = C.c_double(), C.c_double()
        self._check(self._lib.ekf_hypotheses_resample(h, u, split, None if z is None else _p(z), _p(anc, _ip), _p(off, _ip),
                                                      C.byref(ess), C.byref(logmean)))
        return HypothesisResampling(anc, off, ess.value, logmean.value)

    def resample_if(self, fraction: float = 0.5, **kw) -> Optional[HypothesisResampling]:
        """``resample(**kw)`` when the effective sample size has fallen below ``fraction * count``; else None."""
        if self.ess() < float(fraction) * self.count:
            return self.resample(**kw)
        return None

    # -- an uploaded stream, run with the resampling decided on the device ------------------------
    def _pack_stream(self, lin, ang, idx, ranges, bearings):
        """``step``'s arguments per step into ``ekf_hypotheses_stream_upload``'s arrays: (lin, ang, motion_stride, idx, ranges,
        bearings, m, stride, obs_stride), the observation lists padded to the longest.  Every step must agree on shared or
        per-hypothesis motion and observations."""
        steps = len(idx)
        if not (len(lin) == len(ang) == len(ranges) == len(bearings) == steps):
            raise ValueError("upload_stream: lin, ang, idx, ranges and bearings must hold one entry per step")
        motions = [self._motion(l, a) for l, a in zip(lin, ang)]
        obs = [self._obs(i, r, b) for i, r, b in zip(idx, ranges, bearings)]
        if len({mo[2] for mo in motions}) > 1 or len({o[4] for o in obs}) > 1:
            raise ValueError("upload_stream: every step must give its motion, and every step its observations, the same way: "
                             "shared by the bank, or one per hypothesis")
        ms, os_ = (motions[0][2], obs[0][4]) if steps else (0, 0)
        lists, w = (self.count if os_ else 1), max([1] + [o[0].shape[1] for o in obs])
        L, A = np.zeros((steps, self.count if ms else 1)), np.zeros((steps, self.count if ms else 1))
        I, m = np.zeros((steps, lists, w), dtype=np.int32), np.zeros((steps, lists), dtype=np.int32)
        R, B = np.zeros(I.shape), np.zeros(I.shape)
        for s in range(steps):
            L[s], A[s] = motions[s][0], motions[s][1]
            Is, Rs, Bs, m[s], _ = obs[s]
            I[s, :, :Is.shape[1]], R[s, :, :Is.shape[1]], B[s, :, :Is.shape[1]] = Is, Rs, Bs
        return L, A, ms, I, R, B, m, w, os_

    def upload_stream(self, lin, ang, idx, ranges, bearings):
        """A whole recorded run into device memory (``ekf_hypotheses_stream_upload``; blocking): per step the arguments of ``step`` --
        ``lin[s]`` / ``ang[s]`` scalars or ``count`` values, ``idx[s]`` / ``ranges[s]`` / ``bearings[s]`` one flat list or one
        list per hypothesis, at most EKF_MMAX observations --, every step the same way.  A new upload replaces the old one; no
        steps frees it.  The map is frozen, so the stream stays runnable whatever the bank does between runs."""
        h = self._live()
        L, A, ms, I, R, B, m, w, os_ = self._pack_stream(lin, ang, idx, ranges, bearings)
        self._check(self._lib.ekf_hypotheses_stream_upload(h, len(L), _p(L), _p(A), ms, _p(I, _ip), _p(R), _p(B), _p(m, _ip), w, os_))
        self._stream_steps = len(L)

    def run(self, first: int = 0, count: Optional[int] = None, fraction: float = 0.5, split: float = 0.0, u=None, z=None, rng=None):
        """Steps [first, first + count) of the uploaded stream (default: to its end), back to back and asynchronous
        (``ekf_hypotheses_run``): each is ``step`` followed by ``resample_if(fraction, u=u[s], split=split, z=z[s])`` with the
        decision taken on the device from the same effective sample size -- the same bits, and no host round trip.
        ``fraction`` 0: no resampling.  ``u`` (count,) and ``z`` (count, K, 3) are drawn from ``rng`` where they are needed and
        not given.  With the log on (``log``) every step writes a row of ``trace()``."""
        h = self._live()
        first, fraction, split = int(first), float(fraction), float(split)
        count = getattr(self, "_stream_steps", 0) - first if count is None else int(count)
        if ((fraction > 0.0 and u is None) or (split > 0.0 and z is None)) and rng is None:
            rng = np.random.default_rng()
        if u is not None:                                  # (given without a fraction: the library refuses it)
            u = np.ascontiguousarray(np.broadcast_to(_f64(u), (max(count, 0),)))
        elif fraction > 0.0:
            u = rng.random(max(count, 0))
        if z is not None:
            z = np.ascontiguousarray(np.broadcast_to(_f64(z), (max(count, 0), self.count, 3)))
        elif split > 0.0:
            z = rng.standard_normal((max(count, 0), self.count, 3))
        self._check(self._lib.ekf_hypotheses_run(h, first, count, fraction, split, None if u is None else _p(u), None if z is None else _p(z)))

    # -- windows of raw detections: one association on the device for every hypothesis -----------
    def set_association(self, gate_range: float = 1.5, ignore_tags: Sequence[int] = ()):
        """``EkfSlam.set_association`` for the bank (``ekf_hypotheses_set_association``), which took the filter's settings when it
        was made: for later ``step_detections`` and ``upload_detections``.  An uploaded stream is not associated again."""
        ig = _i32(list(ignore_tags)) if len(ignore_tags) else None
        self._check(self._lib.ekf_hypotheses_set_association(self._live(), float(gate_range), _p(ig, _ip) if ig is not None else None,
                                                             len(ignore_tags)))

    @staticmethod
    def _pack_detections(windows):
        """``EkfSlam.localize_detections``' windows through its packer.  A bank has NO host fallback, unlike ``EkfSlam``: a window
        beyond the device's limits -- more than EKF_DMAX detections, a tag id outside [0, 1024) -- raises ``ValueError``."""
        for s, win in enumerate(windows):
            tags = [tag for _stamp, frame in win for tag in frame]
            if len(tags) > EKF_DMAX:
                raise ValueError(f"window {s}: {len(tags)} detections, more than EKF_DMAX = {EKF_DMAX}; a bank has no host association")
            bad = [int(t.tag_id) for t in tags if not 0 <= int(t.tag_id) < EKF_TAGMAX]
            if bad:
                raise ValueError(f"window {s}: tag id {bad[0]} outside [0, {EKF_TAGMAX}); a bank has no host association")
        return _pack_windows(windows)

    def step_detections(self, lin, ang, detections):
        """``EkfSlam.localize_detections`` for every hypothesis (``ekf_hypotheses_step_detections``): ONE window -- the reference's
        ``[(timestamp, [tag, ...])]`` list -- and one motion ``lin`` / ``ang`` for the whole bank.  The window is associated once
        on the device against the bank's tag table (the source slot's at ``EkfSlam.hypotheses``): ignore list, gate, per-tag
        averaging; a tag the map does not hold is skipped and reported by ``unmatched_tags``.  Every hypothesis then takes
        ``step`` with the lists ``tags()`` reports, bit for bit.  Asynchronous.  Unlike ``EkfSlam`` there is no silent host
        route: a window beyond the device's limits raises ``ValueError`` (``_pack_detections``)."""
        h = self._live()
        count, ids, pt, pe, _ = self._pack_detections([detections])
        self._check(self._lib.ekf_hypotheses_step_detections(h, float(lin), float(ang), int(count[0]), _p(ids, _ip), _p(pt), _p(pe)))

    def upload_detections(self, lin, ang, windows):
        """A recorded run of windows into device memory (``ekf_hypotheses_detections_upload``; blocking): ``lin[s]``, ``ang[s]``
        and ``windows[s]`` as ``step_detections`` takes them.  Every window is associated at the upload, in one launch; ``run``
        then runs the stream as it runs an index stream, and ``tags(step=s)`` / ``unmatched_tags(step=s)`` report step s.
        Replaces an earlier stream of either kind; no windows frees it.  ``ValueError`` as for ``step_detections``."""
        h = self._live()
        L, A = np.atleast_1d(_f64(lin)).ravel(), np.atleast_1d(_f64(ang)).ravel()
        if not (len(L) == len(A) == len(windows)):
            raise ValueError("upload_detections: lin, ang and windows must hold one entry per step")
        count, ids, pt, pe, stride = self._pack_detections(windows)
        self._check(self._lib.ekf_hypotheses_detections_upload(h, len(windows), _p(L), _p(A), _p(count, _ip), _p(ids, _ip), _p(pt), _p(pe),
                                                               stride))
        self._stream_steps = len(windows)

    def _window(self, step):
        m, nu, fl = C.c_int(), C.c_int(), C.c_uint()
        idx, tid, un = (np.zeros(EKF_AMAX, dtype=np.int32) for _ in range(3))
        err, rng, brg = (np.zeros(EKF_AMAX) for _ in range(3))
        self._check(self._lib.ekf_hypotheses_download_tags(self._live(), -1 if step is None else int(step), C.byref(m), _p(idx, _ip),
                                                           _p(tid, _ip), _p(err), _p(rng), _p(brg), C.byref(nu), _p(un, _ip), C.byref(fl)))
        return m.value, idx, tid, err, rng, brg, nu.value, un, fl.value

    def tags(self, step: Optional[int] = None) -> dict:
        """The matched tags of the last ``step_detections`` window (``step`` None) or of step ``step`` of the uploaded detection
        stream, in update order: {landmark: (tag_id, err, range, bearing)} (``ekf_hypotheses_download_tags``; blocking)."""
        m, idx, tid, err, rng, brg = self._window(step)[:6]
        return {int(idx[i]): (int(tid[i]), float(err[i]), float(rng[i]), float(brg[i])) for i in range(m)}

    def unmatched_tags(self, step: Optional[int] = None) -> list:
        """The distinct tag ids of that window the map does not hold, in order of first appearance (the first EKF_AMAX)."""
        w = self._window(step)
        return [int(t) for t in w[7][:min(w[6], EKF_AMAX)]]

    def window_flags(self, step: Optional[int] = None) -> int:
        """That window's flag: EKF_FLAG_ASSOC where a tag id was outside [0, 1024) or more than EKF_AMAX distinct tags matched."""
        return int(self._window(step)[8])

    # -- unlabelled observations -----------------------------------------------------------------
    @staticmethod
    def _unlabelled(ranges, bearings):
        """One flat list of at most EKF_MMAX (range, bearing) pairs as two float64 arrays."""
        R, B = np.atleast_1d(_f64(ranges)).ravel(), np.atleast_1d(_f64(bearings)).ravel()
        if np.ndim(ranges) > 1 or np.ndim(bearings) > 1 or len(R) != len(B):
            raise ValueError("unlabelled observations: ONE flat list of ranges and one of bearings, of equal length, for every hypothesis")
        if len(R) > EKF_MMAX:
            raise ValueError(f"unlabelled observations: at most {EKF_MMAX} in one call")
        return R, B

    def associate(self, ranges, bearings, full: bool = False, k=None) -> HypothesisAssociations:
        """``EkfSlam.associate`` per hypothesis (``ekf_hypotheses_associate``; blocking, changes nothing): ONE list of unlabelled
        range/bearing observations scored against every landmark of the map from each hypothesis's own pose, pose block and
        pose rows -- the scores ``associate`` gives on a slot that adopted the hypothesis, bit for bit.  ``k`` None: the whole
        bank; an int: that hypothesis; (k0, count): a range.  ``full=True`` adds the (K, m, N) matrices of NIS and ln det S.
        ``frontend.resolve_associations`` turns one hypothesis's rows into an assignment; ``step_unlabelled`` does all of it
        on the device."""
        h = self._live()
        k0, cnt = (0, self.count) if k is None else ((int(k), 1) if np.ndim(k) == 0 else (int(k[0]), int(k[1])))
        R, B = self._unlabelled(ranges, bearings)
        m, K = len(R), max(cnt, 0)
        cand = np.empty((K, m, 2), dtype=np.int32)
        nis, logdet, mn = np.empty((K, m, 2)), np.empty((K, m, 2)), np.empty((K, m))
        all_nis = all_ld = None
        cap = 0
        if full:
            cap = (self.n - 3) // 2
            big = K * m * cap > 0
            all_nis = _pinned.empty(self._lib, (K, m, cap)) if big else np.empty((K, m, cap))
            all_ld = _pinned.empty(self._lib, (K, m, cap)) if big else np.empty((K, m, cap))
        self._check(self._lib.ekf_hypotheses_associate(h, k0, cnt, _p(R), _p(B), m, _p(cand, _ip), _p(nis), _p(logdet), _p(mn),
                                                       _p(all_nis) if full else None, _p(all_ld) if full else None, cap))
        return HypothesisAssociations(cand, nis, logdet, mn, all_nis, all_ld)

    def step_unlabelled(self, lin, ang, ranges, bearings, accept: float = 9.21, miss: float = 0.0):
        """A localisation step from observations WITHOUT ids (``ekf_hypotheses_step_unlabelled``; asynchronous, no host round
        trip): the prediction (``lin`` / ``ang`` as for ``step``), then per hypothesis ``associate``'s scores,
        ``frontend.resolve_associations`` with no new landmarks -- an observation whose candidate's NIS exceeds ``accept`` is
        dropped --, and ``update`` with what was accepted: the bits of that sequence run on the host.  ``miss``: the
        log-likelihood every dropped observation adds to its hypothesis (``evaluation.clutter_loglik`` gives a default; 0:
        a hypothesis that matches nothing is never penalised).  ``assignments()`` reports what was matched."""
        h = self._live()
        lin, ang, ms = self._motion(lin, ang)
        R, B = self._unlabelled(ranges, bearings)
        self._check(self._lib.ekf_hypotheses_step_unlabelled(h, _p(lin), _p(ang), ms, _p(R), _p(B), len(R), float(accept), float(miss)))
        self._unlabelled_m = len(R)

    def update_unlabelled(self, ranges, bearings, accept: float = 9.21, miss: float = 0.0):
        """``step_unlabelled`` without the prediction (``ekf_hypotheses_update_unlabelled``)."""
        h = self._live()
        R, B = self._unlabelled(ranges, bearings)
        self._check(self._lib.ekf_hypotheses_update_unlabelled(h, _p(R), _p(B), len(R), float(accept), float(miss)))
        self._unlabelled_m = len(R)

    def assignments(self) -> np.ndarray:
        """(K, m) int32: per hypothesis the landmark of every observation of the last ``step_unlabelled`` /
        ``update_unlabelled`` that was accepted, -1 for the dropped ones (``ekf_hypotheses_download_assignment``; blocking).
        ``EkfError`` before the first unlabelled step."""
        out = np.empty((self.count, EKF_MMAX), dtype=np.int32)
        self._check(self._lib.ekf_hypotheses_download_assignment(self._live(), 0, self.count, _p(out, _ip)))
        return out[:, :getattr(self, "_unlabelled_m", EKF_MMAX)].copy()

    def mixture(self) -> HypothesisMixture:
        """The bank's pose mixture formed on the device (``ekf_hypotheses_mixture``; blocking): ``evaluation.mixture_pose``'s mean and
        covariance -- that function stays the host reference -- with the weights' ess, evidence, live count and best."""
        mean, cov = np.empty(3), np.empty((3, 3))
        ess, ev, live, best = C.c_double(), C.c_double(), C.c_int(), C.c_int()
        self._check(self._lib.ekf_hypotheses_mixture(self._live(), _p(mean), _p(cov), C.byref(ess), C.byref(ev), C.byref(live), C.byref(best)))
        return HypothesisMixture(mean, cov, ess.value, ev.value, live.value, best.value)

    def log(self, capacity: int):
        """Keeps the mixture of the last ``capacity`` steps of ``run`` on the device (``ekf_hypotheses_log``); restarts the count.
        0 switches the log off.  ``step`` / ``update`` write no rows."""
        self._check(self._lib.ekf_hypotheses_log(self._live(), int(capacity)))
        self._log_cap = int(capacity)

    def logged(self) -> int:
        """Steps logged since ``log`` switched the log on."""
        n = C.c_longlong(0)
        self._check(self._lib.ekf_hypotheses_log_steps(self._live(), C.byref(n)))
        return int(n.value)

    def trace(self, first: Optional[int] = None, count: Optional[int] = None) -> HypothesisTrace:
        """Steps [first, first + count) of the log (default: every step still in the ring): the bank behind each step's update
        and before its resampling.  Blocking, one copy.  ``evaluation.trajectory_ate`` takes it."""
        total = self.logged()
        if first is None:
            first = max(0, total - getattr(self, "_log_cap", 0)) if count is None else max(0, total - int(count))
        if count is None:
            count = total - int(first)
        first, count = int(first), int(count)
        T = max(count, 0)
        mean, cov, ess, ev = np.empty((T, 3)), np.empty((T, 3, 3)), np.empty(T), np.empty(T)
        live, best, res = np.empty(T, dtype=np.int32), np.empty(T, dtype=np.int32), np.empty(T, dtype=np.int32)
        self._check(self._lib.ekf_hypotheses_download_log(self._live(), first, count, _p(mean), _p(cov), _p(ess), _p(ev), _p(live, _ip),
                                                   _p(best, _ip), _p(res, _ip)))
        return HypothesisTrace(mean, cov, ess, ev, live, best, res != 0, first)

    def adopt(self, k: int, f: "EkfSlam", b: int = 0):
        """Hypothesis k's pose, pose block and pose rows into trajectory ``b`` of ``f``, whose landmark means and P[3:, 3:] must
        be the bank's map bit for bit (a fork of the slot the bank was made from): checked on the device first; on a
        difference ``EkfError`` and nothing written."""
        self._check(self._lib.ekf_hyp_adopt(self._live(), int(k), f._h, int(b)))

    def set_nis_gate(self, threshold: Optional[float] = None, confidence: Optional[float] = None):
        """``EkfSlam.set_nis_gate`` for the bank; rejections are counted per hypothesis (``rejected``)."""
        self._check(self._lib.ekf_hyp_set_nis_gate(self._live(), EkfSlam.nis_gate_threshold(threshold, confidence)))

    def sync(self):
        self._check(self._lib.ekf_hyp_sync(self._live()))


class EkfSlam:
    """A bank of ``batch`` independent EKF-SLAM filters resident on one MI355X.

    State per trajectory: ``mu`` (3+2N,) and ``P`` (3+2N, 3+2N) float64 in HBM.  All stepping calls
    are asynchronous on the handle's stream; ``mean()/covariance()/sync()`` block.
    """

    def __init__(self, n_max: int, batch: int = 1, device: int = 0, config: Optional[EkfConfig] = None):
        self._lib = load_library()
        self.config = config or EkfConfig()
        self.n_max = int(n_max)
        self.batch = int(batch)
        self._h = C.c_void_p()
        cc = self.config._c()
        rc = self._lib.ekf_create(int(device), self.n_max, self.batch, C.byref(cc), C.byref(self._h))
        if rc != 0:
            msg = self._lib.ekf_last_error(None).decode()
            self._h = C.c_void_p()
            raise EkfError(f"ekf_create failed ({rc}): {msg}")
        # windows beyond the device front end's limits are associated on the host (step_detections): per trajectory, the
        # complete TAG_INDEX while it holds ids the device table cannot (>= 1024), and the last host-made tags_positions
        self._assoc_gate, self._assoc_ignore = self.config.gate_range, tuple(self.config.ignore_tags)
        self._host_index = {}
        self._host_tags = {}
        self._host_unmatched = {}                            # localize_detections' host route: the last window's unmatched ids
        # per-call staging arrays and their ctypes pointers, made once: `ndarray.ctypes.data_as` costs ~2 us per argument,
        # seven of them were most of what an online step of a small filter cost on the host (the library copies everything
        # it needs out of these arrays before the call returns)
        self._lin, self._ang = np.zeros(self.batch), np.zeros(self.batch)
        self._m = np.zeros(self.batch, dtype=np.int32)
        self._plin, self._pang, self._pm = _p(self._lin), _p(self._ang), _p(self._m, _ip)
        self._stages = {}
        self._out = None
        self._pose_cap = 0                                   # ring size of the pose log (log_poses); 0: off
        self._stream_steps = 0                               # steps of the uploaded stream (stream_upload)
        self._factor_generation = 0                          # counts factor() and release_factor(): a CovFactor is live while it matches

    # -- plumbing ------------------------------------------------------------------------------
    def _check(self, rc: int):
        if rc != 0:
            raise EkfError(f"status {rc}: {self._lib.ekf_last_error(self._h).decode()}")

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.ekf_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _per_traj(self, x, name, out):
        """One value per trajectory (a scalar or a one-element array is repeated) into the staging array `out`."""
        if np.ndim(x) > 1 or (np.ndim(x) == 1 and len(x) not in (1, self.batch)):
            raise ValueError(f"{name}: expected {self.batch} values")
        out[:] = x

    def _obs(self, idx, ranges, bearings):
        """Observations into the padded [batch, stride] staging arrays + m[batch]; returns their pointers and the stride
        (entries beyond m[b] are whatever an earlier call left there: the library reads m[b] of them)."""
        if isinstance(idx, np.ndarray) and idx.ndim == 2:
            # a whole bank at once, the same number of observations for every trajectory: three block copies instead of three
            # per trajectory (256 trajectories: 160 -> 10 us of host time per call)
            if idx.shape[0] != self.batch or np.shape(ranges) != idx.shape or np.shape(bearings) != idx.shape:
                raise ValueError("observations: [batch, m] arrays of equal shape expected")
            m = idx.shape[1]
            st = self._stage(max(1, m))
            st[0][:, :m], st[1][:, :m], st[2][:, :m] = idx, ranges, bearings
            self._m[:] = m
            return st[3], st[4], st[5], self._pm, max(1, m)
        if self.batch == 1 and (len(idx) == 0 or np.ndim(idx[0]) == 0):
            idx, ranges, bearings = (idx,), (ranges,), (bearings,)
        if len(idx) != self.batch:
            raise ValueError("observations: one list per trajectory expected")
        lens = [len(i) for i in idx]
        stride = max(1, max(lens))
        I, R, B, pI, pR, pB = self._stage(stride)
        for b, mb in enumerate(lens):
            if len(ranges[b]) != mb or len(bearings[b]) != mb:
                raise ValueError("idx / ranges / bearings lengths differ")
            I[b, :mb] = idx[b]
            R[b, :mb] = ranges[b]
            B[b, :mb] = bearings[b]
        self._m[:] = lens
        return pI, pR, pB, self._pm, stride

    def _stage(self, stride):
        st = self._stages.get(stride)
        if st is None:
            I = np.zeros((self.batch, stride), dtype=np.int32)
            R, B = np.zeros((self.batch, stride)), np.zeros((self.batch, stride))
            st = self._stages[stride] = (I, R, B, _p(I, _ip), _p(R), _p(B))
        return st

    def _small_out(self):
        """Output staging for small states (what the library packs into one pinned buffer anyway): pointers made once."""
        if self._out is None:
            mu, P = np.empty(_SMALL_OUT_N), np.empty(_SMALL_OUT_N * _SMALL_OUT_N)
            self._out = (mu, P, _p(mu), _p(P))
        return self._out

    # -- state ---------------------------------------------------------------------------------
    def size(self, b: int = 0) -> int:
        n = C.c_int()
        self._check(self._lib.ekf_state_size(self._h, b, C.byref(n)))
        return n.value

    def set_state(self, mean, cov, b: int = 0):
        """Upload mean and covariance of trajectory b (the upper triangle of `cov` is authoritative: the device
        stores a covariance as its upper triangle and returns it mirrored)."""
        mean = _f64(mean)
        n = mean.shape[0]
        cov = _f64(cov, (n, n))
        self._check(self._lib.ekf_upload_state(self._h, b, _p(mean), _p(cov), n))

    def set_state_diag(self, mean, diag, b: int = 0):
        """P = diag(diag): avoids shipping a dense n x n host matrix for block-diagonal starts."""
        mean = _f64(mean)
        n = mean.shape[0]
        diag = _f64(diag, (n,))
        self._check(self._lib.ekf_upload_state_diag(self._h, b, _p(mean), _p(diag), n))

    def mean(self, b: int = 0) -> np.ndarray:
        n = self.size(b)
        out = np.empty(n)
        self._check(self._lib.ekf_download_mean(self._h, b, _p(out), n))
        return out

    def covariance(self, b: int = 0) -> np.ndarray:
        n = self.size(b)
        out = _pinned.empty(self._lib, (n, n)) if n > _SMALL_OUT_N else np.empty((n, n))
        self._check(self._lib.ekf_download_state(self._h, b, None, _p(out), n))
        return out

    def covariance_block(self, r0: int, c0: int, rows: int, cols: int, b: int = 0) -> np.ndarray:
        """P[r0:r0+rows, c0:c0+cols] only (e.g. the 3x3 pose block) -- O(rows*cols) over PCIe."""
        out = np.empty((rows, cols))
        self._check(self._lib.ekf_download_block(self._h, b, r0, c0, rows, cols, _p(out)))
        return out

    def marginals(self, b: Optional[int] = None):
        """Marginal covariances of the pose and of every landmark, without applying the pending update (no covariance
        pass, no mirror: one read-only kernel over P_base and the pending ranks, O(n k) per trajectory).  Equal to the
        blocks ``covariance_block`` returns after ``flush()`` to rounding, bit-identical where nothing is pending.

        ``b`` given: ``(pose (3, 3), landmarks (N_b, 2, 2))`` of trajectory b.
        ``b`` None: the whole bank in one call, ``(pose (B, 3, 3), landmarks (B, N_hi, 2, 2), counts (B,))`` with the
        blocks beyond a trajectory's landmark count NaN."""
        if b is None:
            b0, count = 0, self.batch
        else:
            b0, count = int(b), 1
        cap = max((self.size(t) - 3) // 2 for t in range(b0, b0 + count))
        pose = _pinned.empty(self._lib, (count, 3, 3))
        lms = _pinned.empty(self._lib, (count, cap, 2, 2)) if cap > 0 else np.empty((count, 0, 2, 2))
        counts = np.empty(count, dtype=np.int32)
        self._check(self._lib.ekf_download_marginals(self._h, b0, count, _p(pose), _p(lms) if cap > 0 else None, cap,
                                                     _p(counts, _ip)))
        if b is not None:
            return pose[0], lms[0, :counts[0]]
        return pose, lms, counts

    def joint(self, landmarks, b: Optional[int] = None):
        """Mean and full joint covariance -- cross-covariances included -- of the pose and a chosen subset of landmarks,
        without applying the pending update (``ekf_download_joint``: no covariance pass, no mirror, one read-only gather
        kernel).  The sub-state is [x, y, theta, l_j0 x, l_j0 y, l_j1 x, ...] in the order the indices are given (any order,
        none twice, at most EKF_JMAX).  Equal to ``state(b)[1][np.ix_(s, s)]`` after ``flush()`` to rounding, bit-identical
        where nothing is pending; a permuted or a smaller selection returns the same bits at the corresponding entries.

        ``b`` given: ``(mean (3 + 2k,), cov (3 + 2k, 3 + 2k))`` of trajectory b for a 1-D index list.
        ``b`` None: one list per trajectory, ``(mean (B, ns), cov (B, ns, ns), k (B,))`` with ns = 3 + 2 max(k, 1) and the
        rows and columns beyond a trajectory's own 3 + 2 k NaN."""
        if b is None:
            b0, count = 0, self.batch
            lists = [np.asarray(x, dtype=np.int64).reshape(-1) for x in landmarks]
            if len(lists) != count:
                raise ValueError("joint: one landmark list per trajectory expected")
        else:
            b0, count = int(b), 1
            lists = [np.asarray(landmarks, dtype=np.int64).reshape(-1)]
        kk = np.array([len(x) for x in lists], dtype=np.int32)
        if kk.max() > EKF_JMAX:
            raise ValueError(f"joint: at most EKF_JMAX = {EKF_JMAX} landmarks per trajectory, got {int(kk.max())}")
        stride = max(1, int(kk.max()))
        lm = np.zeros((count, stride), dtype=np.int32)
        for t, x in enumerate(lists):
            if x.size and (x.min() < np.iinfo(np.int32).min or x.max() > np.iinfo(np.int32).max):
                raise ValueError("joint: landmark index outside the state")
            lm[t, :len(x)] = x
        ns = 3 + 2 * stride
        mean = _pinned.empty(self._lib, (count, ns))
        cov = _pinned.empty(self._lib, (count, ns, ns))
        self._check(self._lib.ekf_download_joint(self._h, b0, count, _p(lm, _ip), _p(kk, _ip), stride, _p(mean), _p(cov)))
        if b is not None:
            n = 3 + 2 * int(kk[0])
            return mean[0, :n], cov[0, :n, :n]
        return mean, cov, kk

    def factor(self, b: Optional[int] = None) -> "CovFactor":
        """The Cholesky factor P = U^T U of the current covariance of trajectory b, or of the whole bank (``b`` None), formed
        on the device (``ekf_factor``: the pending update is applied first, the filter itself is only read).  Returns a
        ``CovFactor``; a later ``factor()`` or ``release_factor()`` replaces it."""
        b0, count = (0, self.batch) if b is None else (int(b), 1)
        logdet, info = np.empty(count), np.empty(count, dtype=np.int32)
        self._factor_generation += 1
        self._check(self._lib.ekf_factor(self._h, b0, count, _p(logdet), _p(info, _ip)))
        n = np.array([self.size(t) for t in range(b0, b0 + count)], dtype=np.int32)
        means = [self.mean(t) for t in range(b0, b0 + count)]
        return CovFactor(self, self._factor_generation, b0, count, b is not None, logdet, info, n, means)

    def release_factor(self):
        """Free the factor workspace on the device; a CovFactor made before is no longer usable."""
        self._factor_generation += 1
        self._check(self._lib.ekf_factor_release(self._h))

    # -- direct measurements -------------------------------------------------------------------
    @staticmethod
    def _chi2_gate(confidence, dof):
        from scipy.stats import chi2
        if not 0.0 < confidence < 1.0:
            raise ValueError("confidence must lie in (0, 1)")
        return np.where(np.asarray(dof) > 0, chi2.ppf(confidence, np.maximum(dof, 1)), np.inf)

    def update_direct(self, targets, z, R, m=None, gate=None) -> "DirectUpdate":
        """Direct measurements ``z = x[s] + v, v ~ N(0, R)`` of the whole bank in one call (``ekf_update_direct``): per
        trajectory a list of targets -- ``EKF_DIRECT_POSE`` (x, y, theta), ``EKF_DIRECT_POSITION`` (x, y) or a landmark index
        (its x, y) --, for each its measurement ``z`` (3 or 2 values) and noise covariance ``R`` (3 x 3 or 2 x 2).  All fixes of
        a trajectory are applied jointly.  ``targets`` / ``z`` / ``R`` are one ragged list per trajectory (a flat list for a
        single trajectory), or padded arrays (B, S), (B, S, 3), (B, S, 3, 3) with ``m`` (B,) counts.  ``gate`` (scalar or (B,),
        None: no gate): a trajectory whose joint NIS exceeds it is rejected as a whole.  The pending update is applied first
        (a covariance pass), the fixes cost one kernel and one more pass whatever their number."""
        B = self.batch
        if m is None:
            if B == 1 and (len(targets) == 0 or np.ndim(targets[0]) == 0):
                targets, z, R = (targets,), (z,), (R,)
            if len(targets) != B or len(z) != B or len(R) != B:
                raise ValueError("update_direct: one list of targets, z and R per trajectory expected")
            mm = np.array([len(t) for t in targets], dtype=np.int32)
            stride = max(1, int(mm.max()))
            T = np.zeros((B, stride), dtype=np.int32)
            Z, RR = np.zeros((B, stride, 3)), np.zeros((B, stride, 3, 3))
            for b in range(B):
                if len(z[b]) != mm[b] or len(R[b]) != mm[b]:
                    raise ValueError("update_direct: targets / z / R lengths differ")
                for j in range(mm[b]):
                    d = 3 if int(targets[b][j]) == EKF_DIRECT_POSE else 2
                    T[b, j] = int(targets[b][j])
                    zj, Rj = np.asarray(z[b][j], dtype=np.float64), np.asarray(R[b][j], dtype=np.float64)
                    if zj.ndim != 1 or Rj.ndim != 2 or len(zj) < d or min(Rj.shape) < d:
                        raise ValueError(f"update_direct: a {d}-row fix needs {d} values and a {d} x {d} covariance")
                    Z[b, j, :d] = zj[:d]                     # (a padded 3-vector / 3 x 3 block is taken by its leading part)
                    RR[b, j, :d, :d] = Rj[:d, :d]
        else:
            T = _i32(targets)
            stride = T.shape[1] if T.ndim == 2 else 0
            Z, RR, mm = _f64(z, (B, stride, 3)), _f64(R, (B, stride, 3, 3)), _i32(m)
            if T.shape != (B, stride) or mm.shape != (B,) or stride < 1:
                raise ValueError("update_direct: (B, S) targets, (B, S, 3) z, (B, S, 3, 3) R and (B,) m expected")
        if stride > EKF_MMAX:
            raise ValueError(f"update_direct: at most EKF_MMAX = {EKF_MMAX} fixes per trajectory, got {stride}")
        g = None
        if gate is not None:
            g = np.empty(B)
            self._per_traj(gate, "gate", g)
        nis, dof, applied = np.empty(B), np.empty(B, dtype=np.int32), np.empty(B, dtype=np.int32)
        self._check(self._lib.ekf_update_direct(self._h, 0, B, _p(T, _ip), _p(Z), _p(RR), _p(mm, _ip), stride,
                                                _p(g) if g is not None else None, _p(nis), _p(dof, _ip), _p(applied, _ip)))
        return DirectUpdate(nis, dof, applied.astype(bool))

    def fix_pose(self, pose, cov, b: Optional[int] = None, position_only: bool = False, confidence: Optional[float] = None):
        """An absolute pose fix [x, y, theta] with covariance `cov` (3 x 3) -- or, ``position_only``, [x, y] with a 2 x 2
        one.  ``b`` None: a row of `pose` (and a `cov`, or one for all) per trajectory; else trajectory b alone.
        ``confidence`` gates the fix at the chi-square quantile of its 3 (2) degrees of freedom.  Returns ``DirectUpdate``."""
        d = 2 if position_only else 3
        bs = list(range(self.batch)) if b is None else [int(b)]
        pose = np.broadcast_to(np.asarray(pose, dtype=np.float64), (len(bs), d))
        cov = np.broadcast_to(np.asarray(cov, dtype=np.float64), (len(bs), d, d))
        tg = EKF_DIRECT_POSITION if position_only else EKF_DIRECT_POSE
        targets, z, R = [[] for _ in range(self.batch)], [[] for _ in range(self.batch)], [[] for _ in range(self.batch)]
        for i, t in enumerate(bs):
            targets[t], z[t], R[t] = [tg], [pose[i]], [cov[i]]
        gate = None if confidence is None else self._chi2_gate(confidence, np.array([len(x) * d for x in targets]))
        return self.update_direct(targets, z, R, gate=gate)

    def anchor_landmarks(self, landmarks, xy, cov, b: Optional[int] = None, confidence: Optional[float] = None):
        """Surveyed landmarks: landmark ``landmarks[j]`` is known to lie at ``xy[j]`` with covariance `cov` (2 x 2, one for
        all, or one per landmark; at most EKF_MMAX per call).  ``b`` None: the same survey for every trajectory of the bank;
        else trajectory b alone.  Two anchored landmarks fix the gauge of the whole map.  ``confidence`` gates the joint update
        at the chi-square quantile of its 2 k degrees of freedom.  Returns ``DirectUpdate``."""
        lm = [int(j) for j in np.asarray(landmarks).reshape(-1)]
        xy = _f64(xy, (len(lm), 2))
        cov = np.broadcast_to(np.asarray(cov, dtype=np.float64), (len(lm), 2, 2))
        bs = list(range(self.batch)) if b is None else [int(b)]
        targets, z, R = [[] for _ in range(self.batch)], [[] for _ in range(self.batch)], [[] for _ in range(self.batch)]
        for t in bs:
            targets[t], z[t], R[t] = lm, list(xy), list(cov)
        gate = None if confidence is None else self._chi2_gate(confidence, np.array([2 * len(x) for x in targets]))
        return self.update_direct(targets, z, R, gate=gate)

    # -- linear measurements -------------------------------------------------------------------
    def update_linear(self, landmarks, H, R, z=None, innovation=None, gate=None, b: Optional[int] = None) -> "LinearUpdate":
        """Linear measurements ``z = H x[s] + v, v ~ N(0, R)`` over the sub-state ``[x, y, theta, l_j0 x, l_j0 y, ...]`` of the
        pose and the listed landmarks (``ekf_update_linear``; the sub-state is ``joint(landmarks)``'s): per trajectory a
        landmark list (at most EKF_LINEAR_LMAX, any order, none twice; empty: the pose alone), ``H`` (D, 3 + 2 k), ``R``
        (D, D; the upper triangle is read) and exactly one of ``z`` (D,: the device forms y = z - H mu[s], no row wrapped) and
        ``innovation`` (D,: y itself, for a model linearised at the mean ``joint`` returned).  D <= EKF_LINEAR_ROWS; all rows
        of a trajectory are applied jointly.  ``b`` None: one entry per trajectory of the bank (a trajectory with no rows
        passes ``H`` of shape (0, ...) or ``None``); or padded arrays -- ``landmarks = (lm (B, L), k (B,))``, ``H`` (B, Ds, 3 + 2 L),
        ``R`` (B, Ds, Ds), ``z`` / ``innovation`` ``= (values (B, Ds), d (B,))``.  ``b`` given: that trajectory's arrays alone.
        ``gate`` (scalar or one per trajectory, None: no gate): a trajectory whose joint NIS exceeds it is rejected as a whole.
        The pending update is applied first (a covariance pass), the rows cost one kernel and one more pass whatever their
        number.  The active bound rises over the highest landmark named."""
        if (z is None) == (innovation is None):
            raise ValueError("update_linear: exactly one of z and innovation expected")
        rr, mode = (z, 0) if innovation is None else (innovation, 1)
        B = self.batch
        if isinstance(landmarks, tuple) and isinstance(rr, tuple) and b is None:
            lm, kk = _i32(landmarks[0]), _i32(landmarks[1])
            rv, dd = _f64(rr[0]), _i32(rr[1])
            if lm.ndim != 2 or rv.ndim != 2 or lm.shape[0] != B or rv.shape[0] != B or kk.shape != (B,) or dd.shape != (B,):
                raise ValueError("update_linear: (B, L) landmarks with (B,) k and (B, Ds) values with (B,) d expected")
            ls, ds = lm.shape[1], rv.shape[1]
            HH, RR = _f64(H, (B, ds, 3 + 2 * ls)), _f64(R, (B, ds, ds))
            b0, count = 0, B
        else:
            if b is not None:
                b0, count = int(b), 1
                landmarks, H, R, rr = (landmarks,), (H,), (R,), (rr,)
            else:
                b0, count = 0, B
            if len(landmarks) != count or len(H) != count or len(R) != count or len(rr) != count:
                raise ValueError("update_linear: one landmark list, H, R and z / innovation per trajectory expected")
            lists = [np.asarray(x if x is not None else [], dtype=np.int64).reshape(-1) for x in landmarks]
            vals = [np.asarray(x if x is not None else [], dtype=np.float64).reshape(-1) for x in rr]
            kk = np.array([len(x) for x in lists], dtype=np.int32)
            dd = np.array([len(x) for x in vals], dtype=np.int32)
            ls, ds = max(1, int(kk.max())), max(1, int(dd.max()))
            lm = np.zeros((count, ls), dtype=np.int32)
            HH, RR, rv = np.zeros((count, ds, 3 + 2 * ls)), np.zeros((count, ds, ds)), np.zeros((count, ds))
            for t in range(count):
                D, ns = int(dd[t]), 3 + 2 * int(kk[t])
                if lists[t].size and (lists[t].min() < np.iinfo(np.int32).min or lists[t].max() > np.iinfo(np.int32).max):
                    raise ValueError("update_linear: landmark index outside the state")
                lm[t, :kk[t]] = lists[t]
                if D == 0:
                    continue
                Ht, Rt = np.asarray(H[t], dtype=np.float64), np.asarray(R[t], dtype=np.float64)
                if Ht.shape != (D, ns) or Rt.shape != (D, D):
                    raise ValueError(f"update_linear: {D} rows over {int(kk[t])} landmarks need H ({D}, {ns}) and R ({D}, {D}), "
                                     f"got {Ht.shape} and {Rt.shape}")
                HH[t, :D, :ns], RR[t, :D, :D], rv[t, :D] = Ht, Rt, vals[t]
        if ls > EKF_LINEAR_LMAX or ds > EKF_LINEAR_ROWS:
            raise ValueError(f"update_linear: at most EKF_LINEAR_LMAX = {EKF_LINEAR_LMAX} landmarks and EKF_LINEAR_ROWS = "
                             f"{EKF_LINEAR_ROWS} rows per trajectory, got {ls} and {ds}")
        g = None
        if gate is not None:
            g = np.empty(count)
            if count == B:
                self._per_traj(gate, "gate", g)
            else:
                g[:] = gate
        nis, applied = np.empty(count), np.empty(count, dtype=np.int32)
        self._check(self._lib.ekf_update_linear(self._h, b0, count, _p(lm, _ip), _p(kk, _ip), ls, _p(HH), _p(rv), _p(RR), _p(dd, _ip),
                                                ds, mode, _p(g) if g is not None else None, _p(nis), _p(applied, _ip)))
        if count != B:                                       # (per trajectory of the bank, as update_direct reports)
            full = np.zeros(B), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
            full[0][b0], full[1][b0], full[2][b0] = nis[0], dd[0], applied[0]
            nis, dd, applied = full
        return LinearUpdate(nis, dd.copy(), applied.astype(bool))

    def constrain_landmarks(self, i, j, offset, cov, b: Optional[int] = None, confidence: Optional[float] = None):
        """Relative constraints between landmarks: ``l_j - l_i = offset + v, v ~ N(0, cov)`` -- "tag j lies 0.585 m east of
        tag i" from a surveyed map that knows no world frame, or, with a zero offset and a tiny `cov`, "i and j are the same
        tag" (then ``remove_landmarks([j])`` merges them).  ``i``, ``j``: one index each or K of them, ``offset`` (K, 2),
        `cov` 2 x 2 (one for all) or (K, 2, 2); one row pair per constraint, all K applied jointly in one call (the distinct
        landmarks of a call number at most EKF_LINEAR_LMAX, the constraints EKF_LINEAR_ROWS // 2).  ``b`` None: the same
        constraints for every trajectory of the bank; else trajectory b alone.  ``confidence`` gates the joint update at the
        chi-square quantile of its 2 K rows.  Returns ``LinearUpdate``."""
        ii, jj = np.asarray(i, dtype=np.int64).reshape(-1), np.asarray(j, dtype=np.int64).reshape(-1)
        K = len(ii)
        if len(jj) != K or K == 0:
            raise ValueError("constrain_landmarks: as many i as j, and at least one, expected")
        if (ii == jj).any():
            raise ValueError("constrain_landmarks: a constraint names one landmark twice")
        off = np.broadcast_to(np.asarray(offset, dtype=np.float64), (K, 2))
        cv = np.broadcast_to(np.asarray(cov, dtype=np.float64), (K, 2, 2))
        lms = sorted({int(x) for x in ii} | {int(x) for x in jj})
        place = {l: 3 + 2 * p for p, l in enumerate(lms)}
        H, R = np.zeros((2 * K, 3 + 2 * len(lms))), np.zeros((2 * K, 2 * K))
        for c in range(K):
            for a in range(2):
                H[2 * c + a, place[int(jj[c])] + a] = 1.0
                H[2 * c + a, place[int(ii[c])] + a] = -1.0
            R[2 * c:2 * c + 2, 2 * c:2 * c + 2] = cv[c]
        gate = None if confidence is None else float(self._chi2_gate(confidence, 2 * K))
        if b is not None:
            return self.update_linear(lms, H, R, z=off.reshape(-1), gate=gate, b=b)
        B = self.batch
        return self.update_linear([lms] * B, [H] * B, [R] * B, z=[off.reshape(-1)] * B, gate=gate)

    def update_custom(self, landmarks, h, z, R, jac=None, wrap=None, b: int = 0, confidence: Optional[float] = None,
                      step: float = 1e-5):
        """A measurement model of the caller's: ``z = h(x_s) + v, v ~ N(0, R)`` with ``x_s`` the sub-state of the pose and
        `landmarks` of trajectory b (``joint(landmarks, b)``'s order).  Reads the sub-mean (``joint``: no covariance pass),
        evaluates ``h`` and its Jacobian there -- ``jac(x_s)`` (D, ns), or central differences of ``h`` with the absolute
        `step` per coordinate when ``jac`` is None (error of a Jacobian entry: step^2 / 6 |h'''| + eps (|h| + |x|) / step) --, forms
        the innovation ``z - h(x_s)`` with the rows listed in ``wrap`` (angles) wrapped to [-pi, pi), and applies it with
        ``update_linear`` in innovation mode.  ``confidence`` gates at the chi-square quantile of the D rows."""
        lms = [int(x) for x in np.asarray(landmarks, dtype=np.int64).reshape(-1)]
        xs, _ = self.joint(lms, b)
        xs = np.array(xs, dtype=np.float64)
        z = np.asarray(z, dtype=np.float64).reshape(-1)
        h0 = np.asarray(h(xs), dtype=np.float64).reshape(-1)
        if h0.shape != z.shape:
            raise ValueError(f"update_custom: h returns {h0.shape[0]} values for {z.shape[0]} measurements")
        if jac is not None:
            J = np.asarray(jac(xs), dtype=np.float64).reshape(len(z), len(xs))
        else:
            J = np.empty((len(z), len(xs)))
            for c in range(len(xs)):
                e = np.zeros(len(xs))
                e[c] = step
                J[:, c] = (np.asarray(h(xs + e), dtype=np.float64).reshape(-1) - np.asarray(h(xs - e), dtype=np.float64).reshape(-1)) / (2.0 * step)
        y = z - h0
        if wrap is not None:
            rows = np.asarray(wrap, dtype=np.int64).reshape(-1)
            y[rows] = (y[rows] + np.pi) % (2.0 * np.pi) - np.pi
        gate = None if confidence is None else float(self._chi2_gate(confidence, len(z)))
        return self.update_linear(lms, J, R, innovation=y, gate=gate, b=b)

    # -- motion models of the caller's -----------------------------------------------------------
    def predict_linear(self, pose, F, Q, b: Optional[int] = None, apply=None):
        """A prediction with the caller's motion model (``ekf_predict_linear``): ``pose`` is the NEW pose mean [x, y, theta],
        taken verbatim (wrap theta yourself), ``F = d(new pose)/d(old pose)`` (3, 3) and ``Q`` (3, 3; the upper triangle is
        read; positive semi-definite, all zero allowed) the process noise:  mu[0:3] = pose,  P[r, r] = F P[r, r] F^T + Q,
        P[r, j] = F P[r, j].  ``b`` None: the whole bank -- ``pose`` (B, 3), ``F`` and ``Q`` (B, 3, 3) or one (3, 3) for every
        trajectory; ``apply`` (B,) leaves the trajectories with a zero entry bit for bit.  ``b`` given: that trajectory alone.
        Asynchronous like ``predict``: no covariance pass, no rank, also while ranks are pending; one pose-log row."""
        if b is None:
            b0, count = 0, self.batch
        else:
            b0, count = int(b), 1
        pp = _f64(np.asarray(pose, dtype=np.float64).reshape(-1, 3), (count, 3))
        FF = _f64(np.broadcast_to(np.asarray(F, dtype=np.float64), (count, 3, 3)))
        QQ = _f64(np.broadcast_to(np.asarray(Q, dtype=np.float64), (count, 3, 3)))
        ap = None
        if apply is not None:
            ap = _i32(np.asarray(apply).reshape(-1) != 0)
            if ap.shape != (count,):
                raise ValueError(f"predict_linear: apply needs {count} entries")
        self._check(self._lib.ekf_predict_linear(self._h, b0, count, _p(pp), _p(FF), _p(QQ), _p(ap, _ip) if ap is not None else None))

    def predict_odometry(self, delta, cov, b: Optional[int] = None):
        """Odometry as a pose increment: ``delta = (dx, dy, dtheta)`` in the robot frame with its 3 x 3 covariance ``cov`` --
        ``pose' = pose (+) delta`` (``compose_pose``; theta wrapped to [-pi, pi)), ``F = d(pose (+) delta)/d(pose)``,
        ``Q = J cov J^T`` with ``J = d/d(delta) = diag(R(theta), 1)``.  Reads the poses with ``joint([], ...)`` (no covariance
        pass), then ``predict_linear``.  ``b`` None: ``delta`` (B, 3) or one for all, ``cov`` (B, 3, 3) or one for all."""
        if b is None:
            count = self.batch
            poses = np.array(self.joint([[]] * count)[0][:, :3])
        else:
            count = 1
            poses = np.array(self.joint([], int(b))[0][:3]).reshape(1, 3)
        dd = np.broadcast_to(np.asarray(delta, dtype=np.float64), (count, 3))
        cv = np.broadcast_to(np.asarray(cov, dtype=np.float64), (count, 3, 3))
        new, FF, QQ = np.empty((count, 3)), np.empty((count, 3, 3)), np.empty((count, 3, 3))
        for t in range(count):
            new[t], FF[t], J = compose_pose(poses[t], dd[t])
            Cu = np.triu(cv[t])
            QQ[t] = J @ (Cu + np.triu(Cu, 1).T) @ J.T
        self.predict_linear(new, FF, QQ, b=b)

    def predict_custom(self, f, u=None, Q=None, jac=None, b: int = 0, step: float = 1e-6):
        """A motion model of the caller's for trajectory b: ``f(pose, u)`` returns the new pose [x, y, theta] (wrapped by the
        caller where it matters), ``jac(pose, u)`` its 3 x 3 Jacobian by the pose -- or, when ``jac`` is None, central
        differences of ``f`` with the absolute `step` per coordinate (error of a Jacobian entry: step^2 / 6 times the third
        derivative plus eps |f| / step; a theta that ``f`` wraps must not cross the seam within `step`).  ``Q`` (3, 3; None: zero)
        is the process noise.  Reads the pose with ``joint([], b)`` (no covariance pass), then ``predict_linear``."""
        x = np.array(self.joint([], int(b))[0][:3], dtype=np.float64)
        new = np.asarray(f(x, u), dtype=np.float64).reshape(3)
        if jac is not None:
            J = np.asarray(jac(x, u), dtype=np.float64).reshape(3, 3)
        else:
            J = np.empty((3, 3))
            for c in range(3):
                e = np.zeros(3)
                e[c] = step
                J[:, c] = (np.asarray(f(x + e, u), dtype=np.float64).reshape(3) - np.asarray(f(x - e, u), dtype=np.float64).reshape(3)) / (2.0 * step)
        self.predict_linear(new, J, np.zeros((3, 3)) if Q is None else Q, b=int(b))

    def _unlabelled(self, ranges, bearings, m):
        """Unlabelled observations as padded (B, stride) float64 arrays + m (B,) int32: (B, S) arrays with `m` (default: S
        each), or one list per trajectory (a flat list for a single trajectory)."""
        if m is None and not isinstance(ranges, np.ndarray):
            if self.batch == 1 and (len(ranges) == 0 or np.ndim(ranges[0]) == 0):
                ranges, bearings = (ranges,), (bearings,)
            if len(ranges) != self.batch or len(bearings) != self.batch:
                raise ValueError("observations: one list per trajectory expected")
            lens = [len(r) for r in ranges]
            stride = max(1, max(lens))
            R, Bg = np.zeros((self.batch, stride)), np.zeros((self.batch, stride))
            for b, mb in enumerate(lens):
                if len(bearings[b]) != mb:
                    raise ValueError("ranges / bearings lengths differ")
                R[b, :mb], Bg[b, :mb] = ranges[b], bearings[b]
            return R, Bg, np.array(lens, dtype=np.int32)
        R = _f64(ranges).reshape(self.batch, -1)
        Bg = _f64(bearings).reshape(self.batch, -1)
        if R.shape != Bg.shape:
            raise ValueError("observations: [batch, m] arrays of equal shape expected")
        mm = np.full(self.batch, R.shape[1], dtype=np.int32) if m is None else _i32(np.broadcast_to(m, (self.batch,)))
        if R.shape[1] == 0:
            R, Bg = np.zeros((self.batch, 1)), np.zeros((self.batch, 1))
        return R, Bg, mm

    def associate(self, ranges, bearings, m=None, full: bool = False) -> "Associations":
        """Score every landmark of every trajectory's map against its UNLABELLED range/bearing observations, on the device
        (``ekf_associate``): per observation the two landmarks of smallest d = NIS + ln det S with their NIS and ln det S,
        and the smallest NIS over all landmarks.  The covariance is the current one -- pending ranks included -- read
        without a covariance pass; the noise is the trajectory's (``set_noise``).  Blocking; changes nothing of the filter
        or its scheduling.  Observations: (B, S) arrays with ``m`` (B,) valid per trajectory (default S), or one list per
        trajectory; at most EKF_MMAX each.  ``full=True`` adds the (B, S, N_hi) matrices of NIS and ln det S.
        ``frontend.resolve_associations`` turns one trajectory's rows into an assignment."""
        R, Bg, mm = self._unlabelled(ranges, bearings, m)
        B, S = R.shape
        cand = np.empty((B, S, 2), dtype=np.int32)
        nis, logdet, mn = np.empty((B, S, 2)), np.empty((B, S, 2)), np.empty((B, S))
        all_nis = all_ld = None
        cap = 0
        if full:
            cap = max((self.size(t) - 3) // 2 for t in range(B))
            all_nis = _pinned.empty(self._lib, (B, S, cap)) if cap > 0 else np.empty((B, S, 0))
            all_ld = _pinned.empty(self._lib, (B, S, cap)) if cap > 0 else np.empty((B, S, 0))
        self._check(self._lib.ekf_associate(self._h, 0, B, _p(R), _p(Bg), _p(mm, _ip), S, _p(cand, _ip), _p(nis), _p(logdet),
                                            _p(mn), _p(all_nis) if full else None, _p(all_ld) if full else None, cap))
        return Associations(cand, nis, logdet, mn, all_nis, all_ld)

    def step_unlabelled(self, lin, ang, ranges, bearings, m=None, accept: float = 9.21, create: float = 18.42,
                        joint: bool = False):
        """One step from UNLABELLED observations: ``predict``, ``associate``, ``frontend.resolve_associations`` per
        trajectory, ``add_landmarks`` for the observations that fit nothing (world position from the predicted pose, as
        ``frontend.associate`` places a new tag), then ``update`` with the pairs in observation order.  ``accept`` /
        ``create`` are NIS thresholds (defaults: the chi-square quantiles of 2 degrees of freedom at 0.99 and 0.9999): an
        observation is matched when its candidate's NIS <= accept, a new landmark when even the best-fitting landmark's
        NIS > create, dropped as ambiguous in between.  Returns one int array per trajectory: the landmark each
        observation updated (new ones included), -1 for a dropped one.  Only existing calls are made: a run whose
        associations equal the truth is bit-identical to the labelled predict / add_landmarks / update run.

        ``joint=True`` replaces the greedy individual test by joint compatibility: per trajectory the candidates of an
        observation are its (at most two) ``associate`` candidates with NIS <= accept, one ``joint()`` call fetches the
        covariance of the pose and the union of all candidates for the whole bank, and
        ``frontend.joint_compatibility`` picks the largest jointly consistent set of pairings -- a pose error larger than
        the landmark spacing no longer shifts every observation onto its neighbour.  The observations it leaves unmatched
        become new landmarks or are dropped by the same ``create`` rule."""
        self.predict(lin, ang)
        R, Bg, mm = self._unlabelled(ranges, bearings, m)
        a = self.associate(R, Bg, mm)
        if joint:
            cands, sels = [], []
            for b in range(self.batch):
                mb = int(mm[b])
                # (associate() ranks by d = NIS + ln det S; joint_compatibility takes ascending individual NIS: stable sort)
                cb = [[j for _, j in sorted(((float(a.nis[b, q, c]), int(a.cand[b, q, c])) for c in range(2)
                                             if a.cand[b, q, c] >= 0 and a.nis[b, q, c] <= accept), key=lambda x: x[0])]
                      for q in range(mb)]
                cands.append(cb)
                sels.append(sorted({j for c in cb for j in c}))
            jm, jc, _ = self.joint(sels)
            qs = self.noise()[1]
        out, idx, zr, zb = [], [], [], []
        for b in range(self.batch):
            mb = int(mm[b])
            if joint:
                assign, _nis, _done = joint_compatibility(R[b, :mb], Bg[b, :mb], cands[b], sels[b], jm[b], jc[b],
                                                          (qs[b] ** 2, qs[b] ** 2))
                rest = np.flatnonzero(assign < 0)
                new_obs = [int(q) for q in rest if a.cand[b, q, 0] < 0 or a.min_nis[b, q] > create]
            else:
                assign, new_obs, _dropped = resolve_associations(a.cand[b, :mb], a.nis[b, :mb], a.min_nis[b, :mb], accept, create)
            if len(new_obs):
                n_lm = (self.size(b) - 3) // 2
                if 3 + 2 * (n_lm + len(new_obs)) > self.n_max:
                    raise EkfError(f"step_unlabelled: trajectory {b}'s map would grow to {n_lm + len(new_obs)} landmarks, "
                                   f"beyond this handle's capacity n_max = {self.n_max}")
                x0, y0, th = self.mean(b)[:3]
                xy = [(x0 + R[b, q] * np.cos(Bg[b, q] + th), y0 + R[b, q] * np.sin(Bg[b, q] + th)) for q in new_obs]
                self.add_landmarks(np.array(xy), b)
                assign[np.asarray(new_obs)] = n_lm + np.arange(len(new_obs))
            keep = np.flatnonzero(assign >= 0)
            out.append(assign)
            idx.append(assign[keep].astype(np.int32))
            zr.append(R[b, keep])
            zb.append(Bg[b, keep])
        self.update(idx, zr, zb)
        return out

    def log_innovations(self, capacity: int):
        """Switch the innovation log on with a ring of the last `capacity` steps (restarting the step count at 0), or off
        with 0.  Every landmark update of every logged step -- each ``update`` / ``step`` / ``step_state`` /
        ``step_detections`` call and each stream step ``stream_run`` runs -- leaves its landmark index, innovation y, its
        covariance S and its NIS.  The filter's results and scheduling are the same bits with the log on or off."""
        self._check(self._lib.ekf_log_innovations(self._h, int(capacity)))
        self._innov_cap = int(capacity)

    def innovations(self, first: Optional[int] = None, count: Optional[int] = None) -> "Innovations":
        """Steps [first, first + count) of the innovation log (default: every step still in the ring), as
        ``Innovations(steps (K,), m (K, B), idx (K, B, W), y (K, B, W, 2), S (K, B, W, 2, 2), nis (K, B, W))``.  W is the
        largest m in the range (at most EKF_AMAX); entries beyond a step's m are -1 / NaN.  Blocking; runs no covariance
        pass.  ``evaluation.nis_consistency`` turns it into consistency statistics and a log-likelihood."""
        logged = C.c_longlong(0)
        self._check(self._lib.ekf_innovation_steps(self._h, C.byref(logged)))
        total = logged.value
        if first is None:
            first = max(0, total - getattr(self, "_innov_cap", 0)) if count is None else max(0, total - int(count))
        if count is None:
            count = total - int(first)
        first, count = int(first), int(count)
        B = self.batch
        shape = (max(count, 0), B)
        m = np.empty(shape, dtype=np.int32)
        idx = np.empty(shape + (EKF_AMAX,), dtype=np.int32)
        y = np.empty(shape + (EKF_AMAX, 2))
        S = np.empty(shape + (EKF_AMAX, 2, 2))
        nis = np.empty(shape + (EKF_AMAX,))
        self._check(self._lib.ekf_download_innovations(self._h, first, count, _p(m, _ip), _p(idx, _ip), _p(y), _p(S),
                                                       _p(nis)))
        rej = np.empty(shape + (EKF_AMAX,), dtype=np.int32)
        self._check(self._lib.ekf_download_innovation_rejections(self._h, first, count, _p(rej, _ip)))
        W = min(int(m.max()), EKF_AMAX) if m.size else 0
        return Innovations(np.arange(first, first + count, dtype=np.int64), m, idx[..., :W].copy(), y[..., :W, :].copy(),
                           S[..., :W, :, :].copy(), nis[..., :W].copy(), rej[..., :W].copy())

    def log_poses(self, capacity: int):
        """Switch the pose log on with a ring of the last `capacity` steps (restarting the step count at 0), or off with 0.
        Every ``predict`` / ``update`` / ``step`` / ``step_state`` / ``step_detections`` call and every stream step of
        ``stream_run`` / ``run_stream`` leaves the pose mean and the 3 x 3 pose block as they stand after it -- the whole
        trajectory out of one uploaded stream.  The filter's results and scheduling are the same bits with the log on or
        off.  Its step count is independent of the innovation log's (a lone ``predict`` is a row here)."""
        self._check(self._lib.ekf_log_poses(self._h, int(capacity)))
        self._pose_cap = int(capacity)

    @property
    def pose_steps(self) -> int:
        """Steps logged since ``log_poses`` switched the pose log on."""
        logged = C.c_longlong(0)
        self._check(self._lib.ekf_pose_steps(self._h, C.byref(logged)))
        return int(logged.value)

    def poses(self, first: Optional[int] = None, count: Optional[int] = None) -> "PoseTrace":
        """Steps [first, first + count) of the pose log (default: every step still in the ring), as
        ``PoseTrace(first, mean (T, B, 3), cov (T, B, 3, 3))``.  Blocking, one copy; runs no covariance pass.
        ``evaluation.trajectory_ate`` and ``evaluation.pose_nees_series`` judge it against ground truth."""
        total = self.pose_steps
        if first is None:
            first = max(0, total - self._pose_cap) if count is None else max(0, total - int(count))
        if count is None:
            count = total - int(first)
        first, count = int(first), int(count)
        shape = (max(count, 0), self.batch)
        mean = np.empty(shape + (3,))
        cov = np.empty(shape + (3, 3))
        self._check(self._lib.ekf_download_poses(self._h, first, count, _p(mean), _p(cov)))
        return PoseTrace(first, mean, cov)

    @staticmethod
    def nis_gate_threshold(threshold: Optional[float] = None, confidence: Optional[float] = None) -> float:
        """The threshold ``set_nis_gate`` passes to the library: `threshold` itself, or for a `confidence` p the chi-square
        quantile of 2 degrees of freedom in closed form, -2 ln(1 - p) (what ``scipy.stats.chi2.ppf(p, 2)`` gives, and the
        gate ``evaluation.nis_consistency(confidence=p)`` counts against); +inf (off) when both are None."""
        if threshold is not None and confidence is not None:
            raise ValueError("set_nis_gate: give a threshold or a confidence, not both")
        if confidence is not None:
            p = float(confidence)
            if not 0.0 < p < 1.0:
                raise ValueError(f"set_nis_gate: confidence must lie in (0, 1), got {confidence!r}")
            return -2.0 * math.log1p(-p)
        if threshold is None:
            return math.inf
        g = float(threshold)
        if not g > 0.0:                                  # (NaN too)
            raise ValueError(f"set_nis_gate: the threshold must be > 0, got {threshold!r}")
        return g

    def set_nis_gate(self, threshold: Optional[float] = None, confidence: Optional[float] = None):
        """Switch the NIS validation gate on: a landmark update whose NIS = y^T S^-1 y exceeds the threshold -- `threshold`,
        or the chi2_2 quantile at `confidence` -- is rejected on the device: mean and covariance stay as they were, later
        updates see the state as if it had never been given.  None for both switches it off (the default: same results and
        scheduling as without the gate).  Applies to the work enqueued after the call and clears ``gate_counts()``."""
        g = self.nis_gate_threshold(threshold, confidence)
        self._check(self._lib.ekf_set_nis_gate(self._h, g))

    def gate_counts(self) -> np.ndarray:
        """(B,) int64: landmark updates each trajectory's gate rejected since the last ``set_nis_gate``.  Blocking."""
        out = np.zeros(self.batch, dtype=np.int64)
        self._check(self._lib.ekf_download_gate_counts(self._h, 0, self.batch, out.ctypes.data_as(C.POINTER(C.c_longlong))))
        return out

    @staticmethod
    def noise_arrays(batch: int, motion_sigma=None, meas_sigma=None):
        """The arrays ``set_noise`` passes to the library: each argument a scalar (every trajectory), a (batch,) array or None
        (the handle's config value: a NULL array), as float64 (batch,) arrays.  ValueError for another shape, a non-finite
        value, motion_sigma < 0 or meas_sigma <= 0."""
        out = []
        for x, name, floor_ok in ((motion_sigma, "motion_sigma", True), (meas_sigma, "meas_sigma", False)):
            if x is None:
                out.append(None)
                continue
            a = np.asarray(x, dtype=np.float64)
            if a.ndim == 0:
                a = np.full(batch, float(a))
            elif a.shape != (batch,):
                raise ValueError(f"set_noise: {name} must be a scalar or shaped ({batch},), got {a.shape}")
            if not np.all(np.isfinite(a)):
                raise ValueError(f"set_noise: {name} must be finite")
            if floor_ok and np.any(a < 0.0):
                raise ValueError(f"set_noise: {name} must be >= 0")
            if not floor_ok and np.any(a <= 0.0):
                raise ValueError(f"set_noise: {name} must be > 0")
            out.append(np.ascontiguousarray(a))
        return out[0], out[1]

    def set_noise(self, motion_sigma=None, meas_sigma=None):
        """Per-trajectory noise constants: trajectory b predicts with motion_sigma[b] and updates with meas_sigma[b] (the
        reference's MOTION_MODEL_VARIANCE / MEASUREMENT_MODEL_VARIANCE) instead of the handle's config.  Each argument is a
        scalar, a (B,) array or None (the config's value).  Applies to the work enqueued after the call; ``set_noise()``
        returns to the handle's constants (the same results as a handle that never called it).  The initial covariance,
        ``predict_dense`` and the association gate do not use these."""
        ms, qs = self.noise_arrays(self.batch, motion_sigma, meas_sigma)
        self._check(self._lib.ekf_set_noise(self._h, 0, self.batch, None if ms is None else _p(ms),
                                            None if qs is None else _p(qs)))

    def noise(self):
        """(motion (B,), meas (B,)): the noise sigmas in effect for work enqueued next.  Does not block."""
        ms, qs = np.empty(self.batch), np.empty(self.batch)
        self._check(self._lib.ekf_get_noise(self._h, 0, self.batch, _p(ms), _p(qs)))
        return ms, qs

    def state(self, b: int = 0):
        n = self.size(b)
        if n <= _SMALL_OUT_N:
            mu, P, pmu, pP = self._small_out()
            self._check(self._lib.ekf_download_state(self._h, b, pmu, pP, n))
            return mu[:n].copy(), P[:n * n].reshape(n, n).copy()
        mu, P = np.empty(n), _pinned.empty(self._lib, (n, n))
        self._check(self._lib.ekf_download_state(self._h, b, _p(mu), _p(P), n))
        return mu, P

    def add_landmarks(self, xy, b: int = 0):
        """Append landmarks with world guesses xy (k,2): variance landmark_init_var, zero cross terms."""
        xy = _f64(xy).reshape(-1, 2)
        first = (self.size(b) - 3) // 2
        self._check(self._lib.ekf_add_landmarks(self._h, b, first, _p(xy), xy.shape[0]))

    def remove_landmarks(self, landmarks, b: Optional[int] = 0) -> np.ndarray:
        """Marginalise the landmarks with these indices out of trajectory b (None: out of every trajectory, one launch).  The
        others keep their order and the indices above a removed one move down: mean and covariance become ``np.delete`` of
        ``state(b)`` taken just before, on both axes, bit for bit.  ``tag_index()`` / ``tags_positions()`` follow (a removed
        tag seen again is a new landmark at the end); an uploaded stream must be uploaded again before ``stream_run``.  The
        innovation log keeps the indices it logged.  Returns ``old_to_new`` (int32, one entry per old landmark, -1 for the
        removed ones; with b None for the bank's largest landmark count -- the same map for every trajectory).  Blocking;
        ``EkfError`` for an index outside the state or given twice, with nothing changed."""
        lm = np.ascontiguousarray(np.asarray(landmarks, dtype=np.int64).ravel())
        if lm.size and (lm.min() < np.iinfo(np.int32).min or lm.max() > np.iinfo(np.int32).max):
            raise EkfError("remove_landmarks: landmark index outside the state")
        lm = lm.astype(np.int32)
        traj = range(self.batch) if b is None else (int(b),)
        n_lm = max((self.size(t) - 3) // 2 for t in traj)
        self._check(self._lib.ekf_remove_landmarks(self._h, -1 if b is None else int(b), _p(lm, _ip) if lm.size else None,
                                                   int(lm.size)))
        keep = np.ones(n_lm, dtype=bool)
        keep[lm] = False
        old_to_new = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
        for t in traj:
            if t in self._host_index:                  # (untagged landmarks' placeholder ids are made again on the next window)
                self._host_index[t] = remap_tag_index({k: j for k, j in self._host_index[t].items() if k >= 0}, old_to_new)
            if t in self._host_tags:
                self._host_tags[t] = {int(old_to_new[j]): v for j, v in self._host_tags[t].items() if old_to_new[j] >= 0}
        return old_to_new

    def copy_from(self, other: "EkfSlam", src=0, dst=0):
        """Copy the complete filter state of trajectory ``src`` of `other` (another handle on the same GPU, or ``self``) into
        trajectory ``dst`` of this one, on the device: afterwards ``state(dst)`` equals ``other.state(src)`` bit for bit, and
        so do size, active bound, ``tag_index`` / ``tags_positions`` and the sticky flags -- the same calls on both from
        there on give the same bits.  ``src`` and ``dst`` are ints or equal-length sequences (one launch for all pairs; a
        source may appear several times, a destination once).  The slot's noise row, gate counter, log rows and uploaded
        stream are NOT copied.  What is pending on either handle is applied first.  Blocking; ``EkfError`` with nothing
        changed for an index outside its bank, a destination named twice, a trajectory both read and written inside one
        handle, handles on different devices, or a state larger than this handle's ``n_max``.  A second handle of the same
        shape plus ``copy_from`` is a checkpoint: ``spare.copy_from(f)`` parks a state, ``f.copy_from(spare)`` restores it."""
        s = np.atleast_1d(np.asarray(src, dtype=np.int64)).ravel()
        d = np.atleast_1d(np.asarray(dst, dtype=np.int64)).ravel()
        if s.shape != d.shape:
            raise ValueError(f"copy_from: src and dst must have the same length, got {s.size} and {d.size}")
        lim = np.iinfo(np.int32)
        if s.size and (min(s.min(), d.min()) < lim.min or max(s.max(), d.max()) > lim.max):
            raise EkfError("copy_from: trajectory index out of range")
        s, d = np.ascontiguousarray(s, dtype=np.int32), np.ascontiguousarray(d, dtype=np.int32)
        self._check(self._lib.ekf_copy_trajectories(self._h, _p(d, _ip) if d.size else None, other._h,
                                                    _p(s, _ip) if s.size else None, int(s.size)))
        # (what the host association keeps per trajectory follows the state: step_detections)
        hi = {int(b): dict(other._host_index[int(a)]) if int(a) in other._host_index else None for a, b in zip(s, d)}
        ht = {int(b): dict(other._host_tags[int(a)]) if int(a) in other._host_tags else None for a, b in zip(s, d)}
        for table, new in ((self._host_index, hi), (self._host_tags, ht)):
            for b, v in new.items():
                if v is None:
                    table.pop(b, None)
                else:
                    table[b] = v

    def join(self, other: "EkfSlam", src=0, dst=0, transform=None, cov=None) -> "MapJoin":
        """Append the map of trajectory ``src`` of `other` (another handle on the same GPU, or ``self``) to trajectory ``dst``
        of this one, on the device (``ekf_join_maps``).  ``transform`` None: sequential map joining -- the source's frame is
        this trajectory's current pose, which is replaced by the composition with the source's pose; the source's landmarks
        are appended with the pose's uncertainty and its correlations with this map.  ``transform`` (x, y, phi) with
        covariance ``cov`` (3 x 3, default zero): the source's frame in this map's, independent of both; this trajectory's
        pose and map stay bit for bit, the source's pose is dropped.  ``src`` and ``dst`` are ints or equal-length sequences
        (one launch; a source may appear several times, a destination once; ``transform`` (k, 3) and ``cov`` (k, 3, 3) then).
        The source is only read; restart a local filter with ``set_state_diag``.  Returns ``MapJoin``: where the appended
        landmarks start, how many, and for each the landmark of this map that already carried its tag (``tag_index``) or -1
        -- fuse such a pair with ``constrain_landmarks(i, j, 0, tiny)`` and ``remove_landmarks([j])``.  What is pending on
        either handle is applied first.  Blocking; ``EkfError`` with nothing changed for a bad index, a destination twice,
        a trajectory both read and written, different devices, a joined state above ``n_max``, a non-finite transform or
        a ``cov`` that is no covariance."""
        scalar = np.ndim(src) == 0 and np.ndim(dst) == 0
        s = np.atleast_1d(np.asarray(src, dtype=np.int64)).ravel()
        d = np.atleast_1d(np.asarray(dst, dtype=np.int64)).ravel()
        if s.shape != d.shape:
            raise ValueError(f"join: src and dst must have the same length, got {s.size} and {d.size}")
        lim = np.iinfo(np.int32)
        if s.size and (min(s.min(), d.min()) < lim.min or max(s.max(), d.max()) > lim.max):
            raise EkfError("join: trajectory index out of range")
        s, d = np.ascontiguousarray(s, dtype=np.int32), np.ascontiguousarray(d, dtype=np.int32)
        k = int(s.size)
        T = cT = None
        if transform is None:
            if cov is not None:
                raise ValueError("join: cov without a transform")
        else:
            T = np.ascontiguousarray(np.broadcast_to(_f64(transform).reshape(-1, 3), (k, 3)))
            cT = np.zeros((k, 3, 3)) if cov is None else np.ascontiguousarray(np.broadcast_to(_f64(cov).reshape(-1, 3, 3), (k, 3, 3)))
        count = np.array([(other.size(int(a)) - 3) // 2 if 0 <= a < other.batch else 0 for a in s], dtype=np.int32)
        stride = max(1, int(count.max()) if k else 1)
        first = np.zeros(max(k, 1), dtype=np.int32)
        twins = np.full((max(k, 1), stride), -1, dtype=np.int32)
        self._check(self._lib.ekf_join_maps(self._h, _p(d, _ip) if k else None, other._h, _p(s, _ip) if k else None, k,
                                            None if T is None else _p(T), None if cT is None else _p(cT),
                                            _p(first, _ip), _p(twins, _ip), stride))
        first, twins = first[:k], twins[:k, :int(count.max()) if k else 0]
        if scalar:
            return MapJoin(int(first[0]), int(count[0]), twins[0].copy())
        return MapJoin(first, count, twins)

    def transform(self, T, cov=None, b: Optional[int] = None):
        """Move the filter into another frame, in place, on the device (``ekf_transform``): ``T`` = (x, y, phi) is the OLD
        frame expressed in the NEW one (``join``'s ``transform`` convention; ``frontend.fit_transform`` returns it), ``cov``
        its 3 x 3 covariance or None when the frame is known exactly.  Every landmark becomes ``t + R l``, the pose
        ``(t + R p_xy, theta + phi)`` (theta is not wrapped), the covariance ``J P J^T`` (+ ``A cov A^T``): exact for any
        offset, no rank and no covariance pass.  ``b`` None: the whole bank -- ``T`` (3,) for all or (batch, 3), ``cov``
        (3, 3) or (batch, 3, 3); ``b`` an int: that trajectory alone, the others stay bit for bit.  What is pending is
        applied first.  Sizes, ``tag_index()``, noise rows, gate counters, flags and log rows stay; ``tags_positions()``
        follows; an uploaded stream stays runnable.  Without ``cov`` the active bound stays, with it every item becomes
        correlated with every other.  ``T`` = 0 without ``cov`` changes nothing, bit for bit.  Blocking; ``EkfError`` with
        nothing changed for a trajectory outside the bank, a non-finite ``T`` or a ``cov`` that is no covariance."""
        b0, count = (0, self.batch) if b is None else (int(b), 1)
        if not -2 ** 31 <= b0 < 2 ** 31:
            raise EkfError("transform: trajectory index out of range")
        T = _f64(T)
        if T.shape not in ((3,), (count, 3)):
            raise ValueError(f"transform: T must be (3,) or ({count}, 3), got {T.shape}")
        T = np.ascontiguousarray(np.broadcast_to(T.reshape(-1, 3), (count, 3)))
        cT = None
        if cov is not None:
            cT = _f64(cov)
            if cT.shape not in ((3, 3), (count, 3, 3)):
                raise ValueError(f"transform: cov must be (3, 3) or ({count}, 3, 3), got {cT.shape}")
            cT = np.ascontiguousarray(np.broadcast_to(cT.reshape(-1, 3, 3), (count, 3, 3)))
        self._check(self._lib.ekf_transform(self._h, b0, count, _p(T), None if cT is None else _p(cT)))
        # (what the host association keeps per trajectory follows the state: the last window's world positions)
        for i in range(count):
            tags = self._host_tags.get(b0 + i)
            if tags:
                c, s = math.cos(T[i, 2]), math.sin(T[i, 2])
                self._host_tags[b0 + i] = {j: [T[i, 0] + (c * v[0] - s * v[1]), T[i, 1] + (s * v[0] + c * v[1])] + list(v[2:])
                                           for j, v in tags.items()}

    def align_landmarks(self, landmarks, xy, weights=None, b: int = 0) -> np.ndarray:
        """Align trajectory b with a survey: fit the current means of ``landmarks`` to their surveyed positions ``xy`` (k, 2)
        (``frontend.fit_transform``, ``weights`` as there; at least two distinct landmarks) and move the filter through the
        fitted frame with ``transform(T, b=b)`` -- WITHOUT a covariance.  Returns ``T``.  The survey's information goes into
        the filter once, through ``anchor_landmarks`` afterwards ("align, then anchor"): the alignment only brings the map
        close enough for that linear update to be valid, whatever the offset was.  Passing the fit's covariance to
        ``transform`` as well would count the survey twice."""
        lm = np.asarray(landmarks, dtype=np.int64).reshape(-1)
        xy = _f64(xy, (len(lm), 2))
        nl = (self.size(b) - 3) // 2
        if lm.size and (lm.min() < 0 or lm.max() >= nl):
            raise EkfError("align_landmarks: landmark index outside the state")
        mean = self.mean(b)[3:].reshape(-1, 2)
        T, _cov = fit_transform(mean[lm], xy, weights)
        self.transform(T, b=b)
        return T

    def fork(self, src: int = 0, dst=None):
        """Fork trajectory ``src`` inside the bank, on the device: ``dst`` (an int, a sequence, or None for every other
        trajectory) becomes a bit-exact twin of it -- ``copy_from(self, src, dst)`` with one source: the source's covariance
        is read once however many twins are made.  Each twin keeps its own noise row, gate counter and log rows: set the
        noise bank, fork, and the bank is a tuning grid or a Monte-Carlo bank starting from one mapped state."""
        src = int(src)
        if dst is None:
            dst = [b for b in range(self.batch) if b != src]
        d = np.atleast_1d(np.asarray(dst, dtype=np.int64)).ravel()
        self.copy_from(self, np.full(d.shape, src, dtype=np.int64), d)

    def flags(self, b: int = 0) -> int:
        f = C.c_uint()
        self._check(self._lib.ekf_status_flags(self._h, b, C.byref(f)))
        return f.value

    def flush(self):
        """Apply the pending low-rank covariance update to P now (asynchronous)."""
        self._check(self._lib.ekf_flush(self._h))

    def sync(self):
        self._check(self._lib.ekf_sync(self._h))

    # -- the EKF ---------------------------------------------------------------------------------
    def predict(self, lin, ang):
        """Motion model + P <- G_F P G_F^T + F^T R F  (src/replay_no_ros.py:368-430)."""
        self._per_traj(lin, "lin", self._lin)
        self._per_traj(ang, "ang", self._ang)
        self._check(self._lib.ekf_predict(self._h, self._plin, self._pang))

    def update(self, idx, ranges, bearings):
        """Sequential range/bearing updates in the given order (src/replay_no_ros.py:436-480)."""
        pI, pR, pB, pm, stride = self._obs(idx, ranges, bearings)
        self._check(self._lib.ekf_update(self._h, pI, pR, pB, pm, stride))

    def step(self, lin, ang, idx, ranges, bearings):
        """predict + update in one fused pass over P.  Observations: a list per trajectory (a flat list for a single
        trajectory), or -- a whole bank with the same number of observations each -- [batch, m] arrays."""
        self._per_traj(lin, "lin", self._lin)
        self._per_traj(ang, "ang", self._ang)
        pI, pR, pB, pm, stride = self._obs(idx, ranges, bearings)
        self._check(self._lib.ekf_step(self._h, self._plin, self._pang, pI, pR, pB, pm, stride))

    # -- localisation on a frozen map ------------------------------------------------------------
    def localize(self, lin, ang, idx, ranges, bearings):
        """predict + the frozen-map (Schmidt-Kalman) update (``ekf_localize_step``): the pose and rows 0..2 of P move, landmark
        means and every P[a, b] with a, b >= 3 stay bit for bit; no rank, never a covariance pass (ranks pending at entry are
        applied first, once).  Arguments as ``step``; an index may come twice."""
        self._per_traj(lin, "lin", self._lin)
        self._per_traj(ang, "ang", self._ang)
        pI, pR, pB, pm, stride = self._obs(idx, ranges, bearings)
        self._check(self._lib.ekf_localize_step(self._h, self._plin, self._pang, pI, pR, pB, pm, stride))

    def localize_update(self, idx, ranges, bearings):
        """The frozen-map update alone (``ekf_localize_update``), behind ``predict``, ``predict_linear`` or ``predict_odometry``."""
        pI, pR, pB, pm, stride = self._obs(idx, ranges, bearings)
        self._check(self._lib.ekf_localize_update(self._h, pI, pR, pB, pm, stride))

    def run_localize(self, first: int = 0, count: Optional[int] = None):
        """Steps [first, first + count) of the uploaded stream (``stream_upload``; default: to its end) in localisation mode
        (``ekf_localize_run``): asynchronous, the same bits as the same steps through ``localize``."""
        if count is None:
            count = self._stream_steps - int(first)
        self._check(self._lib.ekf_localize_run(self._h, int(first), int(count)))

    def step_state(self, lin, ang, idx, ranges, bearings, b: int = 0):
        """``step`` followed by ``state(b)`` as one library call (``ekf_step_fetch``): one iteration of the reference's
        loop, which gets mean and covariance back from every call (src/replay_no_ros.py:229-237).  On the small-state
        path that is one kernel launch and one synchronisation."""
        self._per_traj(lin, "lin", self._lin)
        self._per_traj(ang, "ang", self._ang)
        pI, pR, pB, pm, stride = self._obs(idx, ranges, bearings)
        n = self.size(b)
        if n <= _SMALL_OUT_N:
            mu, P, pmu, pP = self._small_out()
            self._check(self._lib.ekf_step_fetch(self._h, self._plin, self._pang, pI, pR, pB, pm, stride, b, pmu, pP, n))
            return mu[:n].copy(), P[:n * n].reshape(n, n).copy()
        mu, P = np.empty(n), _pinned.empty(self._lib, (n, n))
        self._check(self._lib.ekf_step_fetch(self._h, self._plin, self._pang, pI, pR, pB, pm, stride, b, _p(mu), _p(P), n))
        return mu, P

    # -- device-side front end (association, gate, averaging, augmentation on the GPU) -----------------
    def set_association(self, gate_range: float = 1.5, ignore_tags: Sequence[int] = ()):
        ig = _i32(list(ignore_tags)) if len(ignore_tags) else None
        self._check(self._lib.ekf_set_association(self._h, float(gate_range), _p(ig, _ip) if ig is not None else None,
                                                  len(ignore_tags)))
        self._assoc_gate, self._assoc_ignore = float(gate_range), tuple(int(t) for t in ignore_tags)

    def _window_fits_device(self, win, index_len_hint=None) -> bool:
        """Whether one trajectory's window stays inside the device front end's limits: at most EKF_DMAX = 256 detections, at
        most EKF_AMAX = 32 distinct tags behind IGNORE_TAGS and the gate (src/replay_no_ros.py:286-289), tag ids in [0, 1024)."""
        ids, count, gate2 = [], 0, self._assoc_gate ** 2
        for _stamp, tags in win:
            for tag in tags:
                count += 1
                t = np.asarray(tag.pose_t, dtype=np.float64).ravel()
                if tag.tag_id in self._assoc_ignore or t[2] ** 2 + t[0] ** 2 > gate2:
                    continue
                if tag.tag_id not in ids:
                    ids.append(tag.tag_id)
        return count <= EKF_DMAX and len(ids) <= EKF_AMAX and all(0 <= int(t) < EKF_TAGMAX for t in ids)

    def step_detections(self, lin, ang, detections):
        """One window of raw detections per trajectory: the reference's ``[(timestamp, [tag, ...])]`` list
        (src/replay_no_ros.py:280-284), or a list of such lists for a batch.  Association, the 1.5 m gate,
        per-tag averaging, augmentation, prediction and update all run on the GPU.

        The device front end has limits the reference's dictionaries do not (:280-301): tag ids in [0, 1024), at most 256
        detections and 32 distinct tags per window (round 6; until round 5: 64 and 16 -- the reference's normal mode, a 0.7 s
        window of every camera frame, :17, did not fit).  Every window is checked against them on the host first; when a
        trajectory's window does not fit -- or its TAG_INDEX already holds an id the device table cannot -- the CALL takes
        the host association (``frontend.associate``: no limits), augmentation through ``add_landmarks`` and the update
        through ``step`` (which splits lists of more than 16 landmarks), and the device's table follows the host's
        afterwards where its ids allow.  Same results either way (tests/test_gpu_api_regressions.py).  Only the capacity
        stays fixed: a map that would outgrow ``n_max`` raises ``EkfError`` before anything is enqueued."""
        self._per_traj(lin, "lin", self._lin)
        self._per_traj(ang, "ang", self._ang)
        lin, ang = self._lin, self._ang
        if self.batch == 1 and (len(detections) == 0 or isinstance(detections[0], tuple)):
            detections = [detections]
        if len(detections) != self.batch:
            raise ValueError("detections: one window per trajectory expected")
        if self._host_index or not all(self._window_fits_device(win) for win in detections):
            self._lib.ekf_debug_note_assoc_fallback(self._h)       # (counted: ekf_debug_assoc_fallbacks / assoc_fallbacks())
            return self._step_detections_host(lin, ang, detections)
        self._host_tags.clear()
        self._detections_call(self._lib.ekf_step_detections, detections)

    def _detections_call(self, entry, detections):
        """One window per trajectory, frames concatenated in order, into the arrays ``ekf_step_detections`` and
        ``ekf_localize_detections`` take; lin / ang are in the staging arrays."""
        count, ids, pt, pe, stride = _pack_windows(detections)
        self._check(entry(self._h, self._plin, self._pang, _p(count, _ip), _p(ids, _ip), _p(pt), _p(pe), stride))

    # -- localisation from raw detections --------------------------------------------------------
    def localize_detections(self, lin, ang, detections):
        """``localize`` on whatever one window of raw detections per trajectory matches (``ekf_localize_detections``): window
        format and batch handling as ``step_detections``, but the map is frozen -- a tag the trajectory's TAG_INDEX does not
        hold is skipped and reported by ``unmatched_tags``, nothing is added, the table and the sizes stay as they are.
        Association, gate, averaging and the step run on the GPU with no host round trip; ``tags_positions`` returns the matched
        tags.  The call takes the host route -- ``tag_index`` + ``mean`` + ``frontend.associate_known`` + ``localize``, counted
        in ``assoc_fallbacks()`` -- when a window does not fit the device front end (``step_detections`` has the limits) or a
        trajectory's TAG_INDEX lives on the host because it holds ids the device table cannot."""
        self._per_traj(lin, "lin", self._lin)
        self._per_traj(ang, "ang", self._ang)
        if self.batch == 1 and (len(detections) == 0 or isinstance(detections[0], tuple)):
            detections = [detections]
        if len(detections) != self.batch:
            raise ValueError("detections: one window per trajectory expected")
        if self._host_index or not all(self._window_fits_device(win) for win in detections):
            self._lib.ekf_debug_note_assoc_fallback(self._h)
            return self._localize_detections_host(self._lin.copy(), self._ang.copy(), detections)
        self._localize_detections_device(detections)

    def _localize_detections_device(self, detections):
        self._host_tags.clear()
        self._host_unmatched.clear()
        self._detections_call(self._lib.ekf_localize_detections, detections)

    def _localize_detections_host(self, lin, ang, detections):
        tags_all, unmatched_all = [], []
        for b, win in enumerate(detections):
            index = self.tag_index(b)                              # (the host's while it is in charge; no stand-in ids)
            tags, unmatched = associate_known(win, index, self.mean(b)[:3], self._assoc_gate, self._assoc_ignore,
                                              n_landmarks=(self.size(b) - 3) // 2)
            tags_all.append(tags)
            unmatched_all.append(unmatched)
        idx = [list(t.keys()) for t in tags_all]
        self.localize(lin, ang, idx, [[t[k][4] for k in ks] for t, ks in zip(tags_all, idx)],
                      [[t[k][5] for k in ks] for t, ks in zip(tags_all, idx)])
        for b, (tags, unmatched) in enumerate(zip(tags_all, unmatched_all)):
            self._host_tags[b] = tags
            self._host_unmatched[b] = unmatched

    def unmatched_tags(self, b: int = 0) -> list:
        """The distinct tag ids of trajectory b's last ``localize_detections`` window that its map does not hold, in order of
        first appearance (``ekf_download_unmatched``: the first EKF_AMAX of them; the host route keeps all)."""
        if b in self._host_unmatched:
            return [int(t) for t in self._host_unmatched[b]]
        m = C.c_int()
        ids = np.full(EKF_AMAX, -1, dtype=np.int32)
        self._check(self._lib.ekf_download_unmatched(self._h, b, C.byref(m), _p(ids, _ip), EKF_AMAX))
        return [int(t) for t in ids[:min(m.value, EKF_AMAX)]]

    def reset_pose(self, pose, cov, b: Optional[int] = None):
        """The kidnapped-robot entry: the pose mean replaced by ``pose``, the pose block set to ``cov`` (3, 3), every
        pose-landmark cross term dropped; the map stays.  ``predict_linear(pose, F = 0, Q = cov)``: ``b`` None resets the whole
        bank (``pose`` (B, 3) or one for all), ``b`` given that trajectory alone."""
        count = self.batch if b is None else 1
        self.predict_linear(np.broadcast_to(np.asarray(pose, dtype=np.float64), (count, 3)), np.zeros((3, 3)), cov, b=b)

    def hypotheses(self, count: int, b: int = 0) -> "HypothesisBank":
        """A bank of ``count`` pose hypotheses on trajectory b's map as it stands now (``ekf_hyp_create``): the map is copied
        once -- nothing this filter does afterwards reaches the bank --, every hypothesis starts from b's pose, and the bank
        takes this filter's config, b's noise pair and the NIS gate.  Seed them with ``HypothesisBank.reset``
        (``frontend.poses_on_circle``), step them, rank them (``evaluation.resolve_hypotheses``) and write the winner back with
        ``HypothesisBank.adopt``."""
        hy = C.c_void_p()
        self._check(self._lib.ekf_hyp_create(self._h, int(b), int(count), C.byref(hy)))
        return HypothesisBank(self._lib, hy, count, self.size(b))

    def _step_detections_host(self, lin, ang, detections):
        """The same window through the host association (see step_detections): what the reference does at :280-360 with
        its unbounded dictionaries, then the device's augmentation and update."""
        indices, tags_all = [], []
        for b, win in enumerate(detections):                       # everything is checked before anything is enqueued
            index = dict(self._host_index[b]) if b in self._host_index else self.tag_index(b)
            n_old = self.size(b)
            if 3 + 2 * len(index) != n_old:
                # landmarks added without a tag (add_landmarks / set_state): give them ids no detector produces
                for j in range((n_old - 3) // 2):
                    if j not in index.values():
                        index[-1 - j] = j
            tags = associate(win, index, self.mean(b)[:3], self._assoc_gate, self._assoc_ignore)
            if 3 + 2 * len(index) > self.n_max:
                raise EkfError(f"step_detections: trajectory {b}'s map would grow to {len(index)} landmarks, beyond this "
                               f"handle's capacity n_max = {self.n_max}")
            indices.append(index)
            tags_all.append(tags)
        for b, (index, tags) in enumerate(zip(indices, tags_all)):
            n_old, n_new = self.size(b), 3 + 2 * len(index)
            new_xy = [(tags[(i - 3) // 2][0], tags[(i - 3) // 2][1]) for i in range(n_old, n_new, 2)]   # (:355-360)
            if new_xy:
                self.add_landmarks(np.array(new_xy), b)
        idx = [list(t.keys()) for t in tags_all]
        self.step(lin, ang, idx, [[t[k][4] for k in ks] for t, ks in zip(tags_all, idx)],
                  [[t[k][5] for k in ks] for t, ks in zip(tags_all, idx)])
        for b, (index, tags) in enumerate(zip(indices, tags_all)):
            self._host_tags[b] = tags
            real = {t: j for t, j in index.items() if t >= 0}
            if len(real) == len(index) and all(t < EKF_TAGMAX for t in real):
                self.set_tag_index(real, b)                        # the device table can hold it: it follows the host's
                self._host_index.pop(b, None)
            else:
                self._host_index[b] = index                        # ids beyond the device table: the host stays in charge

    def assoc_fallbacks(self) -> int:
        """Windows `step_detections` took through the host association because they did not fit the device front end."""
        return int(self._lib.ekf_debug_assoc_fallbacks(self._h))

    def tags_positions(self, b: int = 0) -> dict:
        """What EKF_pose_estimation returns as its third value for the last window (:331-337), update order."""
        if b in self._host_tags:                                   # the last window was associated on the host
            return dict(self._host_tags[b])
        m = C.c_int()
        idx, tid = np.zeros(EKF_AMAX, dtype=np.int32), np.zeros(EKF_AMAX, dtype=np.int32)
        arrs = [np.zeros(EKF_AMAX) for _ in range(5)]
        self._check(self._lib.ekf_download_tags(self._h, b, C.byref(m), _p(idx, _ip), _p(tid, _ip), *[_p(a) for a in arrs]))
        if self.flags(b) & EKF_FLAG_ASSOC:
            raise EkfError("device-side association dropped a detection (tag id outside [0, 1024), more than "
                           f"{EKF_AMAX} distinct tags in one window, or the state is full): the map no longer matches "
                           "the reference's; use a larger n_max or the host association")
        xw, yw, err, rng, brg = arrs
        return {int(idx[i]): [xw[i], yw[i], err[i], int(tid[i]), rng[i], brg[i]] for i in range(m.value)}

    def tag_index(self, b: int = 0) -> dict:
        """TAG_INDEX of trajectory b: {tag_id: landmark index} (:294-295) -- the device's table, or the host's while it
        holds ids the device table cannot (see step_detections)."""
        if b in self._host_index:
            return {t: j for t, j in self._host_index[b].items() if t >= 0}
        cap = max(1, (self.n_max - 3) // 2)
        tags = np.full(cap, -1, dtype=np.int32)
        cnt = C.c_int()
        self._check(self._lib.ekf_download_tag_index(self._h, b, _p(tags, _ip), cap, C.byref(cnt)))
        return {int(tags[i]): i for i in range(cnt.value) if tags[i] >= 0}    # (a landmark joined in as a twin carries no tag)

    def set_tag_index(self, tag_index: dict, b: int = 0):
        order = [t for t, _ in sorted(tag_index.items(), key=lambda kv: kv[1])]
        if sorted(tag_index.values()) != list(range(len(order))):
            raise ValueError("TAG_INDEX values must be 0..len-1")
        arr = _i32(order) if order else None
        self._check(self._lib.ekf_upload_tag_index(self._h, b, _p(arr, _ip) if arr is not None else None, len(order)))

    def stream_upload(self, lin, ang, idx, ranges, bearings, m=None) -> int:
        """Copy a whole input stream into HBM (blocking).  Returns the number of steps.

        lin, ang: [steps, batch]; idx, ranges, bearings: [steps, batch, stride]; m: [steps, batch]
        (default: every step observes ``stride`` landmarks).
        """
        lin = _f64(lin).reshape(-1, self.batch)
        steps = lin.shape[0]
        ang = _f64(ang).reshape(steps, self.batch)
        idx = _i32(idx).reshape(steps, self.batch, -1)
        stride = idx.shape[2]
        ranges = _f64(ranges).reshape(steps, self.batch, stride)
        bearings = _f64(bearings).reshape(steps, self.batch, stride)
        m = np.full((steps, self.batch), stride, dtype=np.int32) if m is None else _i32(m).reshape(steps, self.batch)
        self._check(self._lib.ekf_stream_upload(self._h, steps, _p(lin), _p(ang), _p(idx, _ip), _p(ranges),
                                                _p(bearings), _p(m, _ip), stride))
        self._stream_steps = steps
        return steps

    def stream_run(self, first: int, count: int):
        """Enqueue steps [first, first+count) of the uploaded stream (asynchronous)."""
        self._check(self._lib.ekf_stream_run(self._h, int(first), int(count)))

    def run_stream(self, lin, ang, idx, ranges, bearings, m=None):
        """stream_upload + stream_run of every step."""
        steps = self.stream_upload(lin, ang, idx, ranges, bearings, m)
        self.stream_run(0, steps)

    def predict_dense(self, F, Q, b: int = 0):
        """P <- F P F^T + Q for a general dense Jacobian (fp64 MFMA GEMMs)."""
        n = self.size(b)
        F, Q = _f64(F, (n, n)), _f64(Q, (n, n))
        self._check(self._lib.ekf_predict_dense(self._h, b, _p(F), _p(Q)))

    # -- measurement hooks ---------------------------------------------------------------------
    def timer_begin(self):
        self._check(self._lib.ekf_timer_begin(self._h))

    def timer_end(self) -> float:
        ms = C.c_double()
        self._check(self._lib.ekf_timer_end(self._h, C.byref(ms)))
        return ms.value

    def profile_enable(self, on: bool = True):
        self._check(self._lib.ekf_profile_enable(self._h, int(on)))

    def profile_read(self):
        """(total ms, number) of the launches of the covariance pass that carried an event pair since the last read."""
        ms, cnt = C.c_double(), C.c_longlong()
        self._check(self._lib.ekf_profile_read(self._h, C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value

    def profile_read_class(self, cls: int):
        """(total ms, number) of the bracketed launches of class `cls` (1 solve, 2 chain / gather, 3 panel, 4 the k_direct launch of
        update_direct, 5 the k_linear launch of update_linear, 6 the k_join launch of join, 7 the k_predict_pose launch of predict_linear,
        9 / 10 the k_loc_solve / k_loc_rows launches of localize; needs the option
        "profile_kernels"); read before `profile_read`, which resets."""
        ms, cnt = C.c_double(), C.c_longlong()
        self._check(self._lib.ekf_profile_read_class(self._h, int(cls), C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value

    def profile_passes(self) -> int:
        """All launches of the covariance pass since profiling was enabled (with "profile_stride" = k every k-th is timed)."""
        return int(self._lib.ekf_profile_passes(self._h))

    def last_pass(self) -> str:
        """Name of the kernel the last covariance pass launched (e.g. ``ekf::k_flush_rs<20, true, false, true>``: k-tiles,
        nontemporal, column-panel layout, W fragments formed from V -- as rocprofv3 prints it), '' if none yet."""
        k, t, st = C.c_int(), C.c_int(), C.c_int()
        self._check(self._lib.ekf_last_pass(self._h, C.byref(k), C.byref(t), C.byref(st)))
        if k.value < 0:
            return ""
        nt = "true" if st.value else "false"
        tiles = next(x for x in (4, 8, 12, 16, 20) if x >= t.value)
        if k.value == 2:
            wv = "true" if self._lib.ekf_debug_last_pass_wv(self._h) == 1 else "false"
            return f"ekf::k_flush_rs<{tiles}, {nt}, {'true' if self.n_max > 4096 else 'false'}, {wv}>"
        regs = {4: (4, 0), 8: (8, 0), 12: (12, 0), 16: (16, 0), 20: (15, 5)}[tiles]
        return f"ekf::k_flush<{regs[0]}, {regs[1]}, {nt}>"

    def cadence_counters(self):
        """(fused cadences launched by stream_run so far, steps of the uploaded stream they covered): which path ran."""
        a, b = C.c_long(), C.c_long()
        self._check(self._lib.ekf_debug_cadences(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_option(self, name: str, value: int):
        self._check(self._lib.ekf_set_option(self._h, name.encode(), int(value)))


# ------------------------------------------------------------------------------------------------
# Drop-in for the reference function
# ------------------------------------------------------------------------------------------------
class _DropInState:
    """Device state kept between EKF_pose_estimation calls so that a SMALL state need not be uploaded again when the
    caller passes back exactly what the previous call returned (the reference loop does, src/replay_no_ros.py:229-237).
    "Exactly" is checked against PRIVATE byte-for-byte records of what was returned, never against the returned arrays
    themselves: the caller owns those and may edit them in place.  Beyond 131 x 131 nothing is remembered and every call
    uploads: proving that a large covariance is unchanged means reading all of it (row and column sums of the 128 MB at
    N = 2000 cost 19 ms per call), uploading it takes 2.3 ms."""
    filt: Optional[EkfSlam] = None
    mean_obj: Optional[np.ndarray] = None      # the objects handed to the caller (identity test only)
    cov_obj: Optional[np.ndarray] = None
    mean_copy: Optional[bytes] = None          # private records of their contents (small states only)
    cov_copy: Optional[bytes] = None


_drop = _DropInState()
DROP_IN_CONFIG = EkfConfig()      # edit like the reference's module constants
DROP_IN_ALWAYS_UPLOAD = False     # True: never trust the records, upload mean and covariance every call
# Opt-in residency for LARGE states.  False (default): beyond 131 x 131 every call uploads the upper
# triangle (1.4 ms of the 3.8 ms per call at N = 2000).  True: a call that receives the very `mean` / `covariance` OBJECTS
# the previous call returned -- what the reference's loop passes back, src/replay_no_ros.py:229-237 -- skips the upload at
# any size, on the identity of the objects alone: an IN-PLACE edit of the returned arrays between two calls is then NOT
# seen (their bytes are not compared: reading 128 MB costs more than uploading them).  Small states keep the byte-for-byte
# check either way.
DROP_IN_TRUST_IDENTITY = False
DROP_IN_MIN_CAPACITY = 79         # n_max of the first handle (38 landmarks: the small-state path, P resident in LDS); grows by doubling


def EKF_pose_estimation(angular_displacement, linear_displacement, motion_model_mean, motion_model_covariance,
                        delta_t, timestamp_detectedTags_pair_list, TAG_INDEX):
    """Drop-in for ``EKF_pose_estimation`` (src/replay_no_ros.py:269-482).

    Same arguments (``delta_t`` accepted and unused, like :274), same return triple
    ``(mean, covariance, tags_positions)``; ``TAG_INDEX`` is mutated in place (:295).
    Raises ``KeyError`` like :359 when a newly indexed tag has no measurement this window.
    """
    cfg = DROP_IN_CONFIG
    mean_in = np.asarray(motion_model_mean, dtype=np.float64)
    cov_in = np.asarray(motion_model_covariance, dtype=np.float64)
    tags_positions = associate(timestamp_detectedTags_pair_list, TAG_INDEX, mean_in,
                               cfg.gate_range, cfg.ignore_tags)
    n_old = mean_in.shape[0]
    n_new = max(n_old, 3 + 2 * len(TAG_INDEX))
    new_xy = []
    for i in range(n_old, n_new, 2):                      # :355-360
        j = (i - 3) // 2
        new_xy.append((tags_positions[j][0], tags_positions[j][1]))   # KeyError like the reference

    d = _drop
    small = n_old <= _SMALL_OUT_N
    same_objects = (not DROP_IN_ALWAYS_UPLOAD and d.filt is not None and d.mean_obj is motion_model_mean
                    and d.cov_obj is motion_model_covariance and d.filt.size() == n_old and cov_in.shape == (n_old, n_old))
    resident = same_objects and ((small and d.mean_copy == mean_in.tobytes() and d.cov_copy == cov_in.tobytes())
                                 or (not small and DROP_IN_TRUST_IDENTITY))
    if d.filt is None or d.filt.n_max < n_new or d.filt.config != cfg:
        cap = max(DROP_IN_MIN_CAPACITY, n_new if d.filt is None else max(n_new, 2 * d.filt.n_max - 3))
        cap |= 1
        if d.filt is not None:
            d.filt.close()
        d.filt = EkfSlam(cap, 1, 0, dataclasses.replace(cfg))
        resident = False
    f = d.filt
    if not resident:
        f.set_state(mean_in, cov_in)
    if new_xy:
        f.add_landmarks(np.array(new_xy))
    idx = list(tags_positions.keys())
    mean, cov = f.step_state(linear_displacement, angular_displacement, idx,
                             [tags_positions[k][4] for k in idx], [tags_positions[k][5] for k in idx])
    # (q == 0 or a singular S leave NaN in the mean, like NumPy's 0/0 at :466-469 -- the sticky device flag says the same,
    #  but asking for it costs a round trip per call)
    if not np.isfinite(mean).all():
        warnings.warn("EKF_pose_estimation: non-finite state (q == 0 or singular S)", RuntimeWarning)
    d.mean_obj, d.cov_obj = mean, cov
    d.mean_copy, d.cov_copy = (mean.tobytes(), cov.tobytes()) if len(mean) <= _SMALL_OUT_N else (None, None)
    return mean, cov, tags_positions


# ------------------------------------------------------------------------------------------------
# 3-state prototype surface (src/EKF-SLAM.py:29-84)
# ------------------------------------------------------------------------------------------------
motion_noise = np.diag([0.1, 0.1, np.radians(5)])      # EKF-SLAM.py:12
observation_noise = np.diag([0.5, 0.5])                # EKF-SLAM.py:13
_proto = {}


def _proto_filter(kind: str) -> EkfSlam:
    if kind not in _proto:
        cfg = EkfConfig(meas_sigma=float(np.sqrt(observation_noise[0, 0])))
        _proto[kind] = EkfSlam(3 if kind == "predict" else 5, 1, 0, cfg)
    return _proto[kind]


def predict(state, covariance, control, dt):
    """3-state EKF prediction, ``src/EKF-SLAM.py:29-56``: arc motion for |omega| > 1e-6, theta wrapped
    with atan2(sin, cos), straight-line Jacobian F, ``covariance <- F P F^T + motion_noise`` on the GPU
    (general dense path)."""
    v, omega = control
    state = np.asarray(state, dtype=np.float64)
    theta = state[2]
    if abs(omega) > 1e-6:
        dx = -v / omega * np.sin(theta) + v / omega * np.sin(theta + omega * dt)
        dy = v / omega * np.cos(theta) - v / omega * np.cos(theta + omega * dt)
        dth = omega * dt
    else:
        dx, dy, dth = v * np.cos(theta) * dt, v * np.sin(theta) * dt, 0.0
    new_state = state + np.array([dx, dy, dth])
    new_state[2] = np.arctan2(np.sin(new_state[2]), np.cos(new_state[2]))
    F = np.array([[1.0, 0.0, -v * dt * np.sin(theta)], [0.0, 1.0, v * dt * np.cos(theta)], [0.0, 0.0, 1.0]])
    f = _proto_filter("predict")
    f.set_state(new_state, covariance)
    f.predict_dense(F, motion_noise)
    return new_state, f.covariance()


def update(state, covariance, observation, landmark_pos):
    """3-state EKF update against a known landmark, ``src/EKF-SLAM.py:59-84``.  Runs the device update
    on [x, y, theta, lx, ly] with a zero-covariance landmark block, which reduces to the 2x3 H of :67-70
    (observation noise diag(0.5, 0.5), :13)."""
    f = _proto_filter("update")
    mu = np.concatenate([np.asarray(state, dtype=np.float64)[:3], np.asarray(landmark_pos, dtype=np.float64)[:2]])
    P = np.zeros((5, 5))
    P[:3, :3] = covariance
    f.set_state(mu, P)
    f.update([0], [float(observation[0])], [float(observation[1])])
    mu2, P2 = f.state()
    return mu2[:3].copy(), P2[:3, :3].copy()
