"""CPU: localisation from raw detections (ekf_localize_detections / ekf_download_unmatched; EkfSlam.localize_detections,
unmatched_tags, reset_pose) without a device -- the C-ABI surface (header, binding, library export), frontend.associate_known
against frontend.associate, the recovery condition of the kidnapped-robot case on the dense model alone, the replay driver and
the node adapter in localisation mode on a CPU stand-in backend, and the host-side plan under the sanitizers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests import host_check
from tests import loc_det_world as ldw
from tests import localize_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIGNATURES = {
    "ekf_localize_detections": ["ekf_handle *h", "const double *lin", "const double *ang", "const int *count", "const int *tag_id",
                                "const double *pose_t", "const double *pose_err", "int stride"],
    "ekf_download_unmatched": ["ekf_handle *h", "int b", "int *m", "int *tag_id", "int capacity"],
}


def test_header_library_and_binding_declare_the_same_calls():
    text = open(os.path.join(ROOT, "include", "ekfslam_hip.h")).read()
    from slam_duckietown_amd import ekf_bindings as eb
    for name, want in SIGNATURES.items():
        decl = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert decl, f"{name} is not declared in include/ekfslam_hip.h"
        assert [" ".join(p.split()) for p in decl.group(1).split(",")] == want, name
        assert eb.ABI[name][0] is C.c_int and len(eb.ABI[name][1]) == len(want), name
    assert eb.ABI["ekf_localize_detections"][1] == eb.ABI["ekf_step_detections"][1]      # the arguments of its mapping twin
    assert eb.ABI["ekf_download_unmatched"][1] == [C.c_void_p, C.c_int, eb._ip, eb._ip, C.c_int]
    for method in ("localize_detections", "unmatched_tags", "reset_pose"):
        assert callable(getattr(eb.EkfSlam, method))
    makefile = open(os.path.join(ROOT, "slam-duckietown_amd", "csrc", "Makefile")).read()
    assert "ekf_loc_assoc.hip" in makefile
    lib = eb.library_path()
    if not os.path.exists(lib):
        pytest.skip("the library is not built")
    exported = host_check.exported_symbols(lib)
    for name in SIGNATURES:
        assert exported.get(name) == "T", name
    assert eb.load_library().ekf_localize_detections(None, None, None, None, None, None, None, 0) != 0   # a NULL handle: refused
    assert eb.load_library().ekf_download_unmatched(None, 0, None, None, 0) != 0


# ---- frontend.associate_known ----------------------------------------------------------------------------------------------------
def test_associate_known_against_associate():
    from slam_duckietown_amd import frontend
    world = ldw.World(9, 3)
    index = {t: j for j, t in enumerate(world.ids)}
    pose = np.array([0.1, -0.05, 0.3])
    for frames, which in ((1, [4, 0, 7]), (3, [2, 8, 1, 5]), (9, [6, 3]), (2, [])):        # (9 frames: np.mean's pairwise sum of the errors)
        world.move()
        win = world.window(which, frames)
        grown = dict(index)
        want = frontend.associate(win, grown, pose)
        got, unmatched = frontend.associate_known(win, index, pose)
        assert grown == index and unmatched == []
        assert list(got) == list(want) == which
        for j in which:
            assert got[j][3] == want[j][3] == world.ids[j]
            assert all(np.array_equal(got[j][q], want[j][q]) for q in (0, 1, 2, 4, 5)), j     # the same numbers, bit for bit
    # unknown tags, an ignored one, one beyond the gate: reported in order of first appearance, the index as it was
    win = world.window([1, 2], 2)
    win[0][1].insert(1, ldw.det(977, 0.1, 0.6))
    win[0][1].append(ldw.det(955, -0.2, 0.7))
    win[1][1].insert(0, ldw.det(977, 0.1, 0.61))
    win[1][1].append(ldw.det(world.ids[5], 0.0, 0.5))                                      # ignored below
    win[1][1].append(ldw.det(world.ids[6], 1.2, 1.2))                                      # 1.7 m: beyond the gate
    win[1][1].append(ldw.det(966, 1.2, 1.2))                                               # unknown AND beyond the gate: dropped first
    before = dict(index)
    got, unmatched = frontend.associate_known(win, index, pose, 1.5, (world.ids[5],))
    assert index == before and unmatched == [977, 955] and list(got) == [1, 2]
    clean = world.window([], 1)
    clean[0] = (0.0, [t for _s, tags in win for t in tags if t.tag_id in (world.ids[1], world.ids[2])])
    want = frontend.associate(clean, dict(index), pose)
    assert all(np.array_equal(got[j][q], want[j][q]) for j in (1, 2) for q in (0, 1, 2, 4, 5))
    # a stale row: an index at or beyond the landmark count is unmatched
    got, unmatched = frontend.associate_known(world.window([7, 3], 1), index, pose, n_landmarks=7)
    assert list(got) == [3] and unmatched == [world.ids[7]]


# ---- the recovery condition of the kidnapped-robot case, on the model alone ---------------------------------------------------------
def test_recovery_condition_holds_on_the_model():
    """From a pose reset 0.3 m and 0.2 rad away from the truth with a covariance covering that offset, the stream's localisation
    windows bring the pose's Mahalanobis distance to the truth under the chi-square(3) 0.999 quantile -- in float64, on
    tests/localize_model.py alone: what tests/test_gpu_localize_detections.py then asks of the device on the same stream."""
    world, wins, reset_truth, loc = ldw.recovery_stream()
    cfg = lm.with_noise(ldw.CFG, **ldw.RECOVERY_NOISE)
    mean, cov, index = ldw.oracle_map(world, wins, cfg, ldw.RECOVERY_P0)      # (mapped with the tuned filter too)
    assert len(index) == ldw.RECOVERY_N
    assert abs(np.linalg.norm(ldw.RECOVERY_OFFSET[:2]) - 0.3) < 1e-15 and ldw.RECOVERY_OFFSET[2] == 0.2
    # reset_pose's definition, predict_linear(pose, F = 0, Q = cov): the pose replaced, the cross terms dropped
    mean[:3] = reset_truth + ldw.RECOVERY_OFFSET
    cov[:3, :] = 0.0
    cov[:, :3] = 0.0
    cov[:3, :3] = ldw.RECOVERY_COV
    d2 = [ldw.mahalanobis(mean, cov, reset_truth)]
    for win, truth in loc:
        (mean, cov), tags, unmatched = ldw.model_window(mean, cov, index, win, cfg=cfg)
        assert len(tags) == 4 and not unmatched
        d2.append(ldw.mahalanobis(mean, cov, truth))
    err = float(np.linalg.norm(mean[:2] - loc[-1][1][:2]))
    print(f"recovery on the model: Mahalanobis^2 at the reset and behind each window {[round(v, 2) for v in d2]}, "
          f"final position error {err:.4f} m")
    assert len(loc) == ldw.RECOVERY_WINDOWS and d2[-1] < ldw.CHI2_3_0999
    assert err < 0.1                                         # and it is a recovery: the 0.3 m offset is gone


# ---- the replay driver and the node adapter in localisation mode ---------------------------------------------------------------------
class LocalizingBackend:
    """A CPU stand-in with the backend protocol of slam_duckietown_amd.replay in localisation mode (set_map): association against
    the frozen map by frontend.associate_known, the step by the model's ROWS form.  It records what the driver hands it."""

    def __init__(self):
        self.mean, self.cov, self.index = np.zeros(3), np.eye(3) * 0.1, {}
        self.calls, self.unmatched = [], []

    def set_state(self, mean, cov):
        self.mean, self.cov = np.array(mean, dtype=float), np.array(cov, dtype=float)

    def set_map(self, mean, cov, tag_index):
        self.set_state(mean, cov)
        self.index = dict(tag_index)

    def pose(self):
        return self.mean[:3]

    def state(self):
        return self.mean, self.cov

    def step(self, ang, lin, detections, tag_index):
        from slam_duckietown_amd import frontend
        self.calls.append((ang, lin, detections))
        tags, self.unmatched = frontend.associate_known(detections, self.index, self.mean[:3], n_landmarks=(len(self.mean) - 3) // 2)
        idx = list(tags)
        self.mean, self.cov = lm.rows_step(self.mean, self.cov, lin, ang, idx, [tags[k][4] for k in idx], [tags[k][5] for k in idx], ldw.CFG)
        return tags

    def close(self):
        pass


def finished_map(seed=17, N=7):
    world = ldw.World(N, seed)
    mean, cov, index = ldw.oracle_map(world, ldw.mapping_windows(world))
    return world, mean, cov, index


def against_the_model(mean, cov, index, calls, poses, final):
    """The recorded calls through the literal form of the model, from the map: every pose and the final state."""
    k = 0
    for ang, lin, win in calls:
        (mean, cov), _, _ = ldw.model_window(mean, cov, index, win, lin, ang)
        assert np.allclose(poses[k], mean[:3], rtol=0, atol=1e-11), k
        k += 1
    assert k == len(poses) and lm.rel(final[0], mean) < 1e-11 and lm.rel(final[1], cov) < 1e-11


def literal(tags):
    return repr([(t.tag_id, [float(v) for v in t.pose_t.ravel()], t.pose_err) for t in tags])


def test_replay_in_localisation_mode():
    import slam_duckietown_amd.replay as rp
    world, mean, cov, index = finished_map()
    lines, lt, rt = [], 1000, 2000
    for k in range(45):                                      # 10 Hz: wheel ticks, a frame every third event, one with a tag the map lacks
        stamp = 50.0 + 0.1 * k
        lt, rt = lt + 1 + k % 3, rt + 2
        lines += [f"{stamp:.3f},left_wheel,{lt}", f"{stamp:.3f},right_wheel,{rt}"]
        if k % 3 == 0:
            tags = world.window([(k + i) % world.N for i in range(3)])[0][1]
            if k == 12:
                tags.insert(1, ldw.det(999, 0.1, 0.8))
            lines.append(f"{stamp + 0.01:.3f},detections,{literal(tags)}")
    be = LocalizingBackend()
    seen = []
    res = rp.replay(lines, backend=be, localize=True, map_state=(mean, cov, index), on_window=lambda d: seen.append(dict(d["tag_index"])))
    assert res.windows == len(be.calls) == len(res.poses) >= 5 and any(len(w) > 1 for _a, _l, w in be.calls)
    assert res.tag_index == index and all(s == index for s in seen) and 999 not in res.tag_index      # the map's, untouched
    assert res.mean.shape == mean.shape and np.array_equal(res.mean[3:], mean[3:]) and np.array_equal(res.covariance[3:, 3:], cov[3:, 3:])
    assert res.path[0] == (mean[0], mean[1]) and all(set(t) <= set(index.values()) for t in res.measured_tags)
    against_the_model(mean, cov, index, be.calls, res.poses, (res.mean, res.covariance))
    assert lm.rel(res.mean[:3], mean[:3]) > 1e-6             # (it moved)
    with pytest.raises(ValueError):
        rp.replay(lines, backend=LocalizingBackend(), localize=True)                       # no map
    with pytest.raises(ValueError):
        rp.replay(lines, backend=LocalizingBackend(), map_state=(mean, cov, index))        # a map without the mode
    with pytest.raises(ValueError):
        rp.replay(lines, backend=LocalizingBackend(), localize=True, map_state=(mean, cov, index), god_key=[1, 2])


def test_node_adapter_in_localisation_mode():
    from slam_duckietown_amd.node_adapter import EkfNodeAdapter
    world, mean, cov, index = finished_map(seed=23)
    be = LocalizingBackend()
    ad = EkfNodeAdapter(backend=be, localize=True)
    ad.set_map(mean, cov, index)
    poses, lt, rt = [], 0, 0
    for k in range(30):
        if k % 5 != 4:                                       # (every fifth tick the encoders stand still: no step)
            lt, rt = lt + 2 + k % 2, rt + 3
            ad.on_left_encoder(lt, 135)
            ad.on_right_encoder(rt, 135)
        if k % 2 == 0:
            tags = world.window([(k + i) % world.N for i in range(2)])[0][1]
            if k == 6:
                tags.append(ldw.det(998, -0.1, 0.7))
            ad.on_image(k, tags)
        poses.append(ad.on_timer())
    assert sum(p is None for p in poses) == 6 and len(be.calls) == 24
    assert ad.tag_index == index and 998 not in ad.tag_index and set(ad.tags) <= set(index.values())
    final = ad.state()
    assert np.array_equal(final[0][3:], mean[3:]) and np.array_equal(final[1][3:, 3:], cov[3:, 3:])
    against_the_model(mean, cov, index, be.calls, [p for p in poses if p is not None], final)
    with pytest.raises(ValueError):
        EkfNodeAdapter(backend=LocalizingBackend()).set_map(mean, cov, index)              # not in localisation mode


# ---- the host plan ---------------------------------------------------------------------------------------------------------------
def test_localize_detections_plan_under_the_sanitizers(tmp_path):
    """plan_localize_detections (csrc/ekf_host_plan.h) and the unmatched record's size (csrc/ekf_device.h), compiled with plain
    g++ under AddressSanitizer + UndefinedBehaviorSanitizer and run through tests/localize_detections_plan_check.cpp.  CPU only."""
    host_check.run_under_sanitizers("localize_detections_plan_check", tmp_path, 300)
    api = open(os.path.join(ROOT, "slam-duckietown_amd", "csrc", "ekf_api.hip")).read()
    assert re.search(r"\bplan_localize_detections\(", api)                                # called from the API ...
    assert not re.search(r"^(static|inline)[^\n;]*\bplan_localize_detections\(", api, flags=re.M)   # ... and defined only in the header
