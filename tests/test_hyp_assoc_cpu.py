"""CPU: a hypothesis bank's unlabelled observations where no GPU is needed -- the table of worlds the GPU test judges (no entry
near the wrap, no unclear candidate order: the caps of tests/test_gpu_hyp_associate.py are ZERO, and this file holds the
condition), the judge against three planted mistakes, the binding's packing and argument checks against a stand-in library,
the header's declarations with their ABI types, the host plans under the sanitizers (tests/hyp_unlabelled_check.cpp) and the
kernels' source: one statement of the scoring arithmetic."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests import assoc_world as aw
from tests import host_check
from tests import hyp_assoc_model as ham

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-duckietown_amd", "csrc")
NAMES = ["ekf_hypotheses_associate", "ekf_hypotheses_step_unlabelled", "ekf_hypotheses_update_unlabelled",
         "ekf_hypotheses_download_assignment"]
QD = np.array([orc.EkfConfig().meas_sigma ** 2] * 2)


# ---- the world table -----------------------------------------------------------------------------------------------------------
def test_world_table_is_clear_of_the_wrap_and_of_unclear_orders():
    """In the reference alone, over the four cases: no bearing residual within 1e-9 of an odd multiple of pi, and the first three
    scores of every observation further apart than the judge's tolerances -- so the GPU test excuses nothing and leaves nothing
    out.  (When this was written: 0 of 1 839 observations, 0 of 91 820 entries, smallest gap 3.0e-6 against ~1e-8.)"""
    totals = ham.new_totals()
    gap = np.inf
    for N, K, m in ham.CASES:
        states = ham.model_states(N, K)
        _, zr, zb = ham.observations(ham.model_map(N)[0], N, m)
        ref = ham.model_query(states, zr, zb, QD)
        ham.judge(ref, states, zr, zb, orc.EkfConfig().meas_sigma, totals, what=f"N = {N}, K = {K}, m = {m}: ")
        d = np.sort(ref.all_nis + ref.all_logdet, axis=2)
        gap = min(gap, float(np.diff(d[:, :, :3], axis=2).min()))
    print(f"the table: {totals}, smallest gap between the first three scores {gap:.2e}")
    assert totals["obs"] == sum(K * m for _, K, m in ham.CASES) == 1839
    assert totals["entries"] == sum(K * m * N for N, K, m in ham.CASES) == 91820
    assert totals["excused"] == 0 and totals["left_out"] == 0, totals
    assert gap > 1e-6


# ---- the judge -----------------------------------------------------------------------------------------------------------------
def stepped_state(N):
    """The slot's own dense state one SLAM step further: a hypothesis whose pose rows are non-zero."""
    mu, P = ham.model_map(N)
    cfg = orc.EkfConfig()
    lms, zr, zb = ham.observations(mu, N, 4)
    return orc.ekf_step_dense(mu, P, 0.004, 0.02, lms, zr, zb, cfg)


def test_judge_catches_three_planted_mistakes():
    N, m = 20, 5
    state = stepped_state(N)
    assert np.abs(state[1][:3, 3:]).max() > 1e-6, "the planted case has no cross terms to leave out"
    _, zr, zb = ham.observations(state[0], N, m)
    sigma = orc.EkfConfig().meas_sigma
    good = ham.model_query([state], zr, zb, QD)
    ham.judge(good, [state], zr, zb, sigma, ham.new_totals())
    # 1: scores formed without the cross terms X
    with pytest.raises(AssertionError):
        ham.judge(ham.model_query([state], zr, zb, QD, cross=False), [state], zr, zb, sigma, ham.new_totals())
    # 2: ranking by NIS alone -- on observations between two landmarks whose ln det S differ
    far = ham.model_states(N, 3)
    ranked = ham.model_query(far, zr, zb, QD, by_nis=True)
    assert not np.array_equal(ranked.cand, ham.model_query(far, zr, zb, QD).cand), "ranking by NIS alone changes nothing in this case"
    with pytest.raises(AssertionError):
        ham.judge(ranked, far, zr, zb, sigma, ham.new_totals())
    # 3: a resolve that lets two observations take one landmark -- a table in which observations 0 and 1 both rank landmark 4
    # first: 1 has the smaller NIS and keeps it, 0 falls to its second candidate; with a second candidate beyond `accept` it drops
    from types import SimpleNamespace as NS
    for second, want in ((1.0, [7, 4, 2]), (20.0, [-1, 4, 2])):
        table = NS(cand=np.array([[[4, 7], [4, 9], [2, 4]]], dtype=np.int32), nis=np.array([[[0.5, second], [0.2, 20.0], [0.1, 0.3]]]),
                   min_nis=np.array([[0.5, 0.2, 0.1]]))
        assert list(ham.host_lists(table, [1.0, 2.0, 3.0], [0.1, 0.2, 0.3], aw.ACCEPT)[3][0]) == want
        assert ham.judge_assignment(np.array([want]), table, aw.ACCEPT) is None
        bad = ham.resolve_twice(table.cand[0], table.nis[0], table.min_nis[0], aw.ACCEPT)[None]
        assert list(bad[0]) == [4, 4, 2] and "where the resolve gives" in ham.judge_assignment(bad, table, aw.ACCEPT)


# ---- the binding ---------------------------------------------------------------------------------------------------------------
class FakeLib:
    """Stands in for the library under HypothesisBank: keeps what the unlabelled entries are handed."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _arr(p, n):
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double)), shape=(n,)).copy() if n else np.zeros(0)

    def ekf_hypotheses_associate(self, h, k0, count, zr, zb, m, cand, nis, logdet, mn, all_nis, all_ld, cap):
        self.calls.append(("associate", k0, count, m, self._arr(zr, m), self._arr(zb, m), all_nis is not None, all_ld is not None, cap))
        for i in range(count * m * 2):
            cand[i] = i
        return 0

    def ekf_hypotheses_step_unlabelled(self, h, lin, ang, ms, zr, zb, m, accept, miss):
        self.calls.append(("step", self._arr(lin, 3 if ms else 1), self._arr(ang, 3 if ms else 1), ms, m, self._arr(zr, m), self._arr(zb, m), accept, miss))
        return 0

    def ekf_hypotheses_update_unlabelled(self, h, zr, zb, m, accept, miss):
        self.calls.append(("update", m, self._arr(zr, m), self._arr(zb, m), accept, miss))
        return 0

    def ekf_hypotheses_download_assignment(self, h, k0, count, out):
        self.calls.append(("assignment", k0, count))
        for i in range(count * 16):
            out[i] = i % 16 if i % 16 < 3 else -1
        return 0

    def ekf_host_alloc(self, nbytes):                          # (no pinned memory here: the pool hands out ordinary arrays)
        return 0

    def ekf_hyp_destroy(self, h):
        return 0


def fake_bank(K=3, n=15):
    from slam_duckietown_amd.ekf_bindings import HypothesisBank
    lib = FakeLib()
    return HypothesisBank(lib, C.c_void_p(1), K, n), lib


def test_binding_packs_one_shared_list_and_refuses_what_the_library_cannot_take():
    from slam_duckietown_amd import evaluation as ev
    bank, lib = fake_bank()
    a = bank.associate([1.0, 2.0], [0.1, -0.2])
    kind, k0, count, m, zr, zb, f1, f2, cap = lib.calls[-1]
    assert (kind, k0, count, m, f1, f2, cap) == ("associate", 0, 3, 2, False, False, 0) and list(zr) == [1.0, 2.0] and list(zb) == [0.1, -0.2]
    assert a.cand.shape == (3, 2, 2) and a.cand.dtype == np.int32 and a.nis.shape == (3, 2, 2) and a.min_nis.shape == (3, 2) and a.all_nis is None
    assert list(a.cand.ravel()) == list(range(12))
    a = bank.associate(np.array([1.0]), np.array([0.5]), full=True, k=2)
    assert lib.calls[-1][1:4] == (2, 1, 1) and lib.calls[-1][6:] == (True, True, 6) and a.all_nis.shape == a.all_logdet.shape == (1, 1, 6)
    a = bank.associate([], [], k=(1, 2))
    assert lib.calls[-1][1:4] == (1, 2, 0) and a.cand.shape == (2, 0, 2)
    bank.step_unlabelled(0.004, 0.02, [1.0, 2.0, 3.0], [0.1, 0.2, 0.3])
    kind, lin, ang, ms, m, zr, zb, accept, miss = lib.calls[-1]
    assert (kind, ms, m, accept, miss) == ("step", 0, 3, 9.21, 0.0) and list(lin) == [0.004] and list(ang) == [0.02] and list(zr) == [1.0, 2.0, 3.0]
    got = bank.assignments()
    assert lib.calls[-1] == ("assignment", 0, 3) and got.shape == (3, 3) and got.dtype == np.int32 and (got == [0, 1, 2]).all()
    bank.step_unlabelled([0.1, 0.2, 0.3], 0.02, [1.0], [0.1], accept=5.0, miss=-7.5)
    kind, lin, ang, ms, m, zr, zb, accept, miss = lib.calls[-1]
    assert (ms, m, accept, miss) == (1, 1, 5.0, -7.5) and list(lin) == [0.1, 0.2, 0.3] and list(ang) == [0.02] * 3
    bank.update_unlabelled([], [], miss=-1.0)
    assert lib.calls[-1][:2] == ("update", 0) and lib.calls[-1][4:] == (9.21, -1.0) and bank.assignments().shape == (3, 0)
    bank.update_unlabelled(np.arange(16.0), np.zeros(16))
    assert lib.calls[-1][1] == 16 and bank.assignments().shape == (3, 16)
    n = len(lib.calls)
    with pytest.raises(ValueError, match="at most 16"):
        bank.step_unlabelled(0.0, 0.0, np.arange(17.0), np.zeros(17))
    with pytest.raises(ValueError, match="equal length"):
        bank.associate([1.0, 2.0], [0.1])
    with pytest.raises(ValueError, match="ONE flat list"):
        bank.update_unlabelled([[1.0], [2.0], [3.0]], [[0.1], [0.2], [0.3]])
    assert len(lib.calls) == n, "a refused list reached the library"
    # the documented default for `miss`
    want = -0.5 * (9.21 + math.log(0.03 ** 4) + 2.0 * math.log(2.0 * math.pi))
    assert abs(ev.clutter_loglik(9.21, 0.03) - want) < 1e-12 and ev.clutter_loglik(9.21, 1.0) < 0.0
    for bad in ((-1.0, 0.1), (float("nan"), 0.1), (9.21, 0.0), (9.21, float("inf"))):
        with pytest.raises(ValueError):
            ev.clutter_loglik(*bad)


def test_header_declares_and_binding_types_the_four_entry_points():
    from slam_duckietown_amd import ekf_bindings as eb
    raw = open(os.path.join(ROOT, "include", "ekfslam_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*ekf_hypotheses\s*\*\s*hy\b" % name, text), name
        assert name in eb.ABI and eb.ABI[name][0] is C.c_int and eb.ABI[name][1][0] is C.c_void_p, name
    assert eb.ABI["ekf_hypotheses_associate"][1] == [C.c_void_p, C.c_int, C.c_int, eb._dp, eb._dp, C.c_int, eb._ip] + [eb._dp] * 5 + [C.c_int]
    assert eb.ABI["ekf_hypotheses_step_unlabelled"][1] == [C.c_void_p, eb._dp, eb._dp, C.c_int, eb._dp, eb._dp, C.c_int, C.c_double, C.c_double]
    assert eb.ABI["ekf_hypotheses_update_unlabelled"][1] == [C.c_void_p, eb._dp, eb._dp, C.c_int, C.c_double, C.c_double]
    assert eb.ABI["ekf_hypotheses_download_assignment"][1] == [C.c_void_p, C.c_int, C.c_int, eb._ip]
    for method in ("associate", "step_unlabelled", "update_unlabelled", "assignments"):
        assert callable(getattr(eb.HypothesisBank, method)), method
    bank_text = raw[raw.index("A bank of pose hypotheses on ONE frozen map"):raw.index("typedef struct ekf_hypotheses ekf_hypotheses;")]
    not_part = bank_text[bank_text.index("Not part of a bank:"):]
    not_part = not_part[:not_part.index("noise.")]
    assert "likelihood association" not in not_part and "joint compatibility" in not_part and "ekf_hypotheses_run" in not_part
    assert "BIT FOR BIT" in bank_text and "ekf_hypotheses_download_assignment" in bank_text


# ---- the host plans and the source ---------------------------------------------------------------------------------------------
def test_host_plans_under_sanitizers_and_the_api_uses_them(tmp_path):
    host_check.run_under_sanitizers("hyp_unlabelled_check", tmp_path, 300)
    api = open(os.path.join(CSRC, "ekf_api.hip")).read()
    for fn in ("plan_hyp_associate", "plan_hyp_unlabelled", "plan_hyp_assignment"):
        assert re.search(r"\b%s\(" % fn, api), fn
        assert not re.search(r"^(static|inline)[^\n;]*\b%s\(" % fn, api, flags=re.M), fn
    # the existing launches are reused: the unlabelled step launches the bank's own solve and rows on the records it wrote
    body = api[api.index("static int hyp_unlabelled("):api.index('extern "C" int ekf_hypotheses_step_unlabelled(')]
    assert "launch_hyp_score(" in body and "launch_hyp_solve(hy->stream, v, hy->durec.p, 1," in body and "launch_hyp_rows(" in body
    assert body.index("launch_hyp_score(") < body.index("launch_hyp_solve(") < body.index("launch_hyp_rows(")
    assert "hipStreamSynchronize" not in body and "hipMemcpy" not in body, "the unlabelled step makes a host round trip"


def test_scoring_arithmetic_is_stated_once():
    shared = open(os.path.join(CSRC, "ekf_assoc_score.h")).read()
    assert shared.count("void assoc_score(") == 1 and shared.count("atan2(") == 1 and shared.count("log(det)") == 1
    assert "struct AssocBest" in shared and "double nan_min(" in shared
    for name, kernel in (("ekf_associate.hip", "k_assoc_query"), ("ekf_hyp_assoc.hip", "k_hyp_score")):
        src = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())
        assert '#include "ekf_assoc_score.h"' in src and "assoc_score(p5, m5," in src and kernel in src, name
        assert not re.search(r"\b(atan2|sqrt|log|wrap_pi|innov_nis)\s*\(", src), f"{name} has scoring arithmetic of its own"
        assert "struct AssocBest" not in src and "nan_min(double" not in src, name
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "ekf_hyp_assoc.hip" in make and "ekf_assoc_score.h" in make
    assert "launch_hyp_score" in open(os.path.join(CSRC, "ekf_launch.h")).read()
    plan = open(os.path.join(CSRC, "ekf_host_plan.h")).read()
    assert "hyp_score_chunks" in plan and "HS_CHUNK" in plan
