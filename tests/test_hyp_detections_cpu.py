"""CPU: a hypothesis bank's windows of raw detections where no GPU is needed -- the host plan under the sanitizers
(tests/hyp_detections_check.cpp), the binding's packing and argument checks against a stand-in library, the header's four new
declarations with their ABI types, the kidnapped-robot condition on the model fleet, the judge of the GPU tests against three
planted mistakes, and the kernel's source."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import host_check
from tests import hyp_detections_model as hdm
from tests import loc_det_world as ldw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-duckietown_amd", "csrc")
NAMES = ["ekf_hypotheses_set_association", "ekf_hypotheses_step_detections", "ekf_hypotheses_detections_upload", "ekf_hypotheses_download_tags"]


# ---- the host plan -------------------------------------------------------------------------------------------------------------
def test_host_plan_under_sanitizers_and_the_api_uses_it(tmp_path):
    host_check.run_under_sanitizers("hyp_detections_check", tmp_path, 300)
    api = open(os.path.join(CSRC, "ekf_api.hip")).read()
    for fn in ("plan_hyp_detections", "plan_hyp_detection_stream", "finish_hyp_detection_stream", "fill_hyp_det_records", "plan_hyp_download_tags"):
        assert re.search(r"\b%s\(" % fn, api), fn
        assert not re.search(r"^(static|inline)[^\n;]*\b%s\(" % fn, api, flags=re.M), fn
    # the new entry points stand outside the span tests/test_hyp_run_cpu.py reads, and the run launches on the bank's stream only
    run = api[api.index('extern "C" int ekf_hypotheses_run('):api.index("static void hyp_row_out(")]
    assert "launch_hyp_associate" not in run and "rp.passes" in run and "rec_offset(i, p)" in run
    for name in NAMES:
        assert ('extern "C" int %s(' % name) not in run and ('extern "C" int %s(' % name) in api, name


# ---- the binding ---------------------------------------------------------------------------------------------------------------
class FakeLib:
    """Stands in for the library under HypothesisBank: keeps what the detection entries are handed."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _arr(p, typ, n):
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(typ)), shape=(n,)).copy() if n else np.zeros(0)

    def ekf_hypotheses_step_detections(self, h, lin, ang, count, ids, pt, pe):
        self.calls.append(("step", lin, ang, count, self._arr(ids, C.c_int, count), self._arr(pt, C.c_double, 3 * count).reshape(-1, 3),
                           self._arr(pe, C.c_double, count)))
        return 0

    def ekf_hypotheses_detections_upload(self, h, steps, lin, ang, count, ids, pt, pe, stride):
        self.calls.append(("upload", steps, stride, self._arr(lin, C.c_double, steps), self._arr(ang, C.c_double, steps),
                           self._arr(count, C.c_int, steps), self._arr(ids, C.c_int, steps * stride).reshape(steps, -1) if steps else None,
                           self._arr(pt, C.c_double, 3 * steps * stride).reshape(steps, -1, 3) if steps else None))
        return 0

    def ekf_hypotheses_set_association(self, h, gate, ids, n):
        self.calls.append(("assoc", gate, n, None if ids is None else self._arr(ids, C.c_int, n)))
        return 0

    def ekf_hypotheses_download_tags(self, h, step, m, idx, tid, err, rng, brg, nu, un, fl):
        self.calls.append(("tags", step))
        C.cast(m, C.POINTER(C.c_int))[0] = 2
        for i, (j, t) in enumerate(((4, 77), (1, 33))):
            idx[i], tid[i], err[i], rng[i], brg[i] = j, t, 0.001 * (i + 1), 1.0 + i, 0.1 * (i + 1)
        C.cast(nu, C.POINTER(C.c_int))[0] = 40                 # more than EKF_AMAX distinct unmatched ids: the first 32 come back
        for i in range(32):
            un[i] = 900 + i
        C.cast(fl, C.POINTER(C.c_uint))[0] = 2
        return 0

    def ekf_hypotheses_run(self, h, first, count, fraction, split, u, z):
        self.calls.append(("run", first, count))
        return 0

    def ekf_hyp_destroy(self, h):
        return 0


def fake_bank(K=3, n=15):
    from slam_duckietown_amd.ekf_bindings import HypothesisBank
    lib = FakeLib()
    return HypothesisBank(lib, C.c_void_p(1), K, n), lib


def test_binding_packs_windows_and_refuses_what_the_device_cannot_take():
    bank, lib = fake_bank()
    win = [(0.0, [ldw.det(11, 0.1, 0.7), ldw.det(12, -0.2, 0.9, err=2e-3)]), (1.0, [ldw.det(11, 0.12, 0.71)])]
    bank.step_detections(0.004, 0.02, win)
    kind, lin, ang, count, ids, pt, pe = lib.calls[-1]
    assert (kind, lin, ang, count) == ("step", 0.004, 0.02, 3) and list(ids) == [11, 12, 11]
    assert np.array_equal(pt, [[0.1, 0.0, 0.7], [-0.2, 0.0, 0.9], [0.12, 0.0, 0.71]]) and np.array_equal(pe, [1e-3, 2e-3, 1e-3])
    bank.step_detections(0.0, 0.0, [])
    assert lib.calls[-1][3] == 0
    bank.upload_detections([0.1, 0.2, 0.3], [1.0, 2.0, 3.0], [win, [], [(0.0, [ldw.det(5, 0.0, 0.5)])]])
    kind, steps, stride, lin, ang, count, ids, pt = lib.calls[-1]
    assert (kind, steps, stride) == ("upload", 3, 3) and list(lin) == [0.1, 0.2, 0.3] and list(ang) == [1.0, 2.0, 3.0] and list(count) == [3, 0, 1]
    assert np.array_equal(ids, [[11, 12, 11], [0, 0, 0], [5, 0, 0]]) and np.array_equal(pt[2, 0], [0.0, 0.0, 0.5])
    bank.run(fraction=0.0)
    assert lib.calls[-1] == ("run", 0, 3)                      # run() defaults to the uploaded windows
    bank.upload_detections([], [], [])
    assert lib.calls[-1][:3] == ("upload", 0, 1)
    n = len(lib.calls)
    with pytest.raises(ValueError, match="one entry per step"):
        bank.upload_detections([0.1], [1.0, 2.0], [win, win])
    with pytest.raises(ValueError, match="EKF_DMAX"):
        bank.step_detections(0.0, 0.0, [(0.0, [ldw.det(11, 0.1, 0.7)] * 257)])
    with pytest.raises(ValueError, match=r"tag id 1024 outside \[0, 1024\)"):
        bank.upload_detections([0.1, 0.2], [0.0, 0.0], [win, [(0.0, [ldw.det(1024, 0.1, 0.7)])]])
    with pytest.raises(ValueError, match="tag id -1 outside"):
        bank.step_detections(0.0, 0.0, [(0.0, [ldw.det(-1, 0.1, 0.7)])])
    assert len(lib.calls) == n, "a refused window reached the library"
    bank.step_detections(0.0, 0.0, [(0.0, [ldw.det(11, 0.1, 0.7)] * 256)])     # the largest window is taken
    assert lib.calls[-1][3] == 256
    assert "no silent host" in type(bank).step_detections.__doc__ and "NO host fallback" in type(bank)._pack_detections.__doc__
    # what comes back
    assert bank.tags() == {4: (77, 0.001, 1.0, 0.1), 1: (33, 0.002, 2.0, 0.2)} and list(bank.tags(step=5)) == [4, 1]
    assert [c for c in lib.calls[-2:]] == [("tags", -1), ("tags", 5)]
    assert bank.unmatched_tags() == [900 + i for i in range(32)] and bank.window_flags(2) == 2
    bank.set_association(1.2, [7, 9])
    assert lib.calls[-1][:3] == ("assoc", 1.2, 2) and list(lib.calls[-1][3]) == [7, 9]
    bank.set_association()
    assert lib.calls[-1] == ("assoc", 1.5, 0, None)


def test_header_declares_and_binding_types_the_four_entry_points():
    from slam_duckietown_amd import ekf_bindings as eb
    from slam_duckietown_amd import replay as rp
    raw = open(os.path.join(ROOT, "include", "ekfslam_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*ekf_hypotheses\s*\*\s*hy\b" % name, text), name
        assert name in eb.ABI and eb.ABI[name][0] is C.c_int and eb.ABI[name][1][0] is C.c_void_p, name
    assert eb.ABI["ekf_hypotheses_step_detections"][1] == [C.c_void_p, C.c_double, C.c_double, C.c_int, eb._ip, eb._dp, eb._dp]
    assert eb.ABI["ekf_hypotheses_detections_upload"][1] == [C.c_void_p, C.c_int, eb._dp, eb._dp, eb._ip, eb._ip, eb._dp, eb._dp, C.c_int]
    assert eb.ABI["ekf_hypotheses_set_association"][1] == [C.c_void_p, C.c_double, eb._ip, C.c_int]
    assert eb.ABI["ekf_hypotheses_download_tags"][1] == [C.c_void_p, C.c_int] + [eb._ip] * 3 + [eb._dp] * 3 + [eb._ip] * 2 + [C.POINTER(C.c_uint)]
    for method in ("step_detections", "upload_detections", "tags", "unmatched_tags", "set_association"):
        assert callable(getattr(eb.HypothesisBank, method)), method
    assert callable(rp.relocalize)
    bank_text = raw[raw.index("A bank of pose hypotheses on ONE frozen map"):raw.index("typedef struct ekf_hypotheses ekf_hypotheses;")]
    not_part = bank_text[bank_text.index("Not part of a bank:"):]
    assert "raw detections" not in not_part[:not_part.index(".")], "the header still lists raw detections as not part of a bank"


# ---- the kidnapped robot: the model fleet meets what the GPU test asks -----------------------------------------------------------------
def test_model_fleet_meets_the_relocalisation_thresholds():
    """hdm.RELOC_K = 32 seeds on the circle of one sighting, the dense model per seed (tests/hypotheses_model.py's reset and
    log-likelihood, ldw.model_window per window), no resampling: the seed with the largest log-likelihood ends within
    chi2_3(0.999) of the truth and within 0.1 m -- what tests/test_gpu_hyp_detections.py asks of replay.relocalize."""
    case = hdm.reloc_case()
    assert len(case.seeds) == hdm.RELOC_K and len(case.steps) == ldw.RECOVERY_WINDOWS
    start = np.linalg.norm(case.seeds[:, :2] - ldw.recovery_stream()[2][:2], axis=1)
    assert start.max() > 0.5, "the seeds do not span the circle"
    fleet = hdm.reloc_fleet(case)
    ll = np.array([f[2] for f in fleet])
    best = int(np.argmax(ll))
    mean, cov, _ = fleet[best]
    d2, err = ldw.mahalanobis(mean, cov, case.truth), float(np.linalg.norm(mean[:2] - case.truth[:2]))
    print(f"model fleet: best seed {best}, Mahalanobis^2 {d2:.3f}, position error {err:.4f} m, log-likelihood {ll[best]:.2f} (median {np.median(ll):.2f})")
    assert d2 < ldw.CHI2_3_0999 and err < 0.1
    assert np.median(ll) < ll[best] - 10.0, "the log-likelihood does not tell the seeds apart"


# ---- the judge ---------------------------------------------------------------------------------------------------------------------
def test_judge_catches_three_planted_mistakes():
    world = ldw.World(40, 21)
    index = {t: j for j, t in enumerate(world.ids)}
    world.move()
    win = world.window([3, 17, 3, 8], 3)
    win[1][1].insert(1, ldw.det(1001, 0.3, 0.8))
    want = hdm.walk(win, index, 40)
    assert list(want[0]) == [3, 17, 8] and want[1] == [1001] and want[2] == 0 and hdm.judge(want, want) is None
    assert "unmatched" in hdm.judge(hdm.walk(win, index, 40, mutant=hdm.MUTANTS[0]), want) or \
        "matched landmarks" in hdm.judge(hdm.walk(win, index, 40, mutant=hdm.MUTANTS[0]), want)
    assert "gap" in hdm.judge(hdm.walk(win, index, 40, mutant=hdm.MUTANTS[1]), want)
    many = world.window([(7 * i + 2) % 40 for i in range(33)], 1)
    want = hdm.walk(many, index, 40)
    assert len(want[0]) == 32 and want[2] == hdm.EKF_FLAG_ASSOC and hdm.judge(want, want) is None
    assert "matched landmarks" in hdm.judge(hdm.walk(many, index, 40, mutant=hdm.MUTANTS[2]), want)
    # ... and a wrong flag, a wrong tag id, a last-bit difference beyond the bar
    assert "flag" in hdm.judge((want[0], want[1], 0), want)
    k = next(iter(want[0]))
    swapped = dict(want[0])
    swapped[k] = (swapped[k][0] + 1,) + swapped[k][1:]
    assert "tag id" in hdm.judge((swapped, want[1], want[2]), want)
    off = dict(want[0])
    off[k] = off[k][:2] + (off[k][2] + 1e-11, off[k][3])
    assert "gap" in hdm.judge((off, want[1], want[2]), want)
    # the model is frontend.associate_known where both are defined
    from slam_duckietown_amd import frontend
    ref, unmatched = frontend.associate_known(win, index, np.zeros(3), n_landmarks=40)
    got = hdm.walk(win, index, 40)
    assert unmatched == got[1] and {k: (v[3], v[2], v[4], v[5]) for k, v in ref.items()} == got[0]


# ---- the kernel's source -----------------------------------------------------------------------------------------------------------
def test_kernel_runs_the_shared_walk_and_has_no_arithmetic_of_its_own():
    src = open(os.path.join(CSRC, "ekf_loc_assoc.hip")).read()
    start = src.index("void k_hyp_associate(")
    body = src[start:src.index("\n}\n", start)]
    assert "det_walk(" in body and "det_tag_out(" in body and "det_heads(" in body
    assert not re.search(r"\b(sqrt|atan2|hypot|cos|sin)\s*\(", body), "k_hyp_associate has range / bearing arithmetic of its own"
    assert "0.0, 0.0, 0.0" in body                             # the world guess is formed with the pose (0, 0, 0)
    assert "k_hyp_associate" not in open(os.path.join(CSRC, "ekf_hypotheses.hip")).read()
    walk = open(os.path.join(CSRC, "ekf_det_walk.h")).read()
    assert walk.count("sqrt(") == 1 and walk.count("atan2(") == 1, "the averaging is no longer one statement"
    assert "launch_hyp_associate" in open(os.path.join(CSRC, "ekf_launch.h")).read()
