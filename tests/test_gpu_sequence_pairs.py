"""GPU: every ordered pair of state-changing calls against ONE dense model (tests/sequence_cases.py has the table and the
reasons, tests/sequence_model.py the model, tests/test_sequence_cpu.py shows that the 225 cases are admissible and the judge
not blind).

Per case: the block-diagonal start, 28 stream steps and three single steps (on the general kernels ranks are pending),
operation A, operation B, then a continuation (a step and a 4-step stream) -- judged after A, after B and after the
continuation with parity_blocks.assert_state_close: the informed part piece by piece at 1e-9, the loose landmarks on their
own scale, exact zeros, exact symmetry, size, tag index, flags.  A stale bound, floor or size word left by A shows in B or in
the continuation's pass; the failure carries the pair's name.

The handles are made once per path and every case resets them (set_option, set_state_diag, set_tag_index: part of the
surface under test); a case that fails drops them, so that the next one starts from new handles."""
import ctypes as C

import numpy as np
import pytest

from tests import parity_blocks as pb
from tests import sequence_cases as sc
from tests.conftest import path_ran

pytestmark = pytest.mark.gpu

HANDLES = {}            # path -> Device
RECORD = {"cases": set(), "pending": {}, "first": set(), "second": set(), "bound_rose": [], "worst": {}}


@pytest.fixture(scope="module")
def sd():
    import slam_duckietown_amd as sd
    sd.load_library()
    yield sd
    for dev in HANDLES.values():
        dev.close()
    HANDLES.clear()


class Device:
    """The filter beside the model: tests/sequence_model.py's method names on an EkfSlam handle (trajectory 0), the handles
    of sequence_cases.sources() beside it."""

    def __init__(self, sd):
        self.sd, self.f = sd, sd.EkfSlam(sc.N_MAX)
        self.src = {}
        for key, (mean, cov, tags) in sc.sources().items():
            h = sd.EkfSlam(len(mean))
            h.set_state(mean, cov)
            h.set_tag_index(tags)
            got = h.state()
            assert np.array_equal(got[0], mean) and np.array_equal(np.triu(got[1]), np.triu(cov))
            self.src[key] = h

    def close(self):
        for h in [self.f] + list(self.src.values()):
            h.close()

    def raw00(self):
        """P_base[0, 0] as stored (no flush)."""
        out = np.empty(1)
        self.sd.load_library().ekf_debug_snapshot(self.f._h, 0, 0, out.ctypes.data_as(C.POINTER(C.c_double)), 1)
        return float(out[0])

    def got(self):
        f = self.f
        mean, cov = f.state()
        assert f.size() == len(mean)
        return mean, cov, f.tag_index(), f.flags()

    def set_option(self, name, value):
        self.f.set_option(name, value)

    def set_state_diag(self, mean, diag):
        self.f.set_state_diag(mean, diag)

    def set_tag_index(self, tags):
        self.f.set_tag_index(tags)

    def step1(self, lin, ang, idx, zr, zb):
        self.f.step(lin, ang, [int(i) for i in idx], [float(x) for x in zr], [float(x) for x in zb])

    def run_stream(self, lin, ang, idx, zr, zb):
        self.f.run_stream(lin, ang, idx, zr, zb)

    def step_detections(self, lin, ang, win):
        self.f.step_detections(lin, ang, win)
        assert self.f.assoc_fallbacks() == 0               # a device-side window

    def predict_linear(self, pose, F, Q):
        self.f.predict_linear(pose, F, Q, b=0)

    def predict_dense1(self, F, Q):
        self.f.predict_dense(F, Q)

    def update_direct(self, targets, z, R):
        assert self.f.update_direct(targets, z, R).applied.all()

    def update_linear(self, landmarks, H, R, z):
        assert self.f.update_linear(landmarks, H, R, z=z, b=0).applied.all()

    def transform(self, T, cov=None):
        self.f.transform(T, cov, b=0)

    def join(self, key, transform=None, cov=None):
        first = (self.f.size() - 3) // 2
        r = self.f.join(self.src[key], transform=transform, cov=cov)
        assert (r.first, r.count) == (first, (self.src[key].size() - 3) // 2)

    def remove_landmarks(self, lms):
        self.f.remove_landmarks(lms)

    def add_landmarks(self, xy):
        self.f.add_landmarks(xy)

    def copy_in(self, key):
        self.f.copy_from(self.src[key])


def model_bound(tr):
    """The active bound the model's history implies: past the highest landmark correlated with anything."""
    seen = np.flatnonzero(tr.seen)
    return 3 + 2 * (int(seen[-1]) + 1) if len(seen) else 3


@pytest.mark.parametrize("a,b", sc.PAIRS, ids=[sc.pair_name(a, b).replace(" ", "_").replace("/", "-") for a, b in sc.PAIRS])
def test_pair(sd, both_paths, a, b):
    general = both_paths == "general_kernels"
    dev = HANDLES.get(both_paths) or HANDLES.setdefault(both_paths, Device(sd))
    model = sc.new_model()
    name = f"{sc.pair_name(a, b)}, {both_paths}"
    bounds = {}

    def judge(stage):
        tr = model.tr
        bounds[stage] = (model_bound(tr), len(tr.mean))
        if stage == "start":
            # ranks pending: the stored P_base[0, 0] is not the covariance's.  The model and the filter agree to 1e-9 (asserted
            # after A), one pending single step alone adds 0.01 of pose noise: a difference above 1e-6 is what is pending
            raw, want = dev.raw00(), float(tr.cov[0, 0])
            RECORD["pending"][a, b, both_paths] = abs(raw - want) > 1e-6 * want
            if general:
                assert RECORD["pending"][a, b, both_paths], f"{name}: no ranks pending at A (P_base[0, 0] = {raw}, P[0, 0] = {want})"
            return
        got = dev.got()
        err = pb.assert_state_close(got, model.state(), sc.INIT_VAR, sc.TOL, sc.ENTRY_TOL, what=f"{name}, after {stage}: ")
        bounds["P00"] = float(got[1][0, 0])
        assert path_ran(dev.f, both_paths), f"{name}, after {stage}: not the path {both_paths}"
        for pos, op in (("first", a), ("second", b)):
            w = RECORD["worst"].setdefault((both_paths, pos, op), {})
            for p, v in err.items():
                w[p] = max(w.get(p, 0.0), v)

    try:
        sc.run_case(sc.Driver(model, dev), a, b, judge)
        if general:
            # the continuation ended in a covariance pass: a pass kernel has run, and nothing is pending behind the download
            assert "k_flush" in dev.f.last_pass(), f"{name}: the continuation ended in no covariance pass"
            assert dev.raw00() == bounds["P00"], f"{name}: ranks pending behind the last download"
    except AssertionError:
        HANDLES.pop(both_paths).close()
        raise
    except Exception as e:                                 # a call refused or failed: nothing more is started on this device
        HANDLES.pop(both_paths, None)
        pytest.exit(f"{name}: {type(e).__name__}: {e}", returncode=3)
    RECORD["cases"].add((a, b, both_paths))
    RECORD["first"].add((a, both_paths))
    RECORD["second"].add((b, both_paths))
    if bounds["A"][0] < bounds["A"][1] and bounds["B"][0] == bounds["B"][1]:
        RECORD["bound_rose"].append(name)


def test_the_module_kept_its_promises():
    """Every pair ran on both paths; ranks were pending at A in every general-kernels case; every operation ran in both
    positions on both paths; some case left the bound below n before B raised it.  Prints the worst of every piece per
    operation and position (profiles/sequence_pairs.txt)."""
    for (path, pos, op), w in sorted(RECORD["worst"].items()):
        print(f"DEVICE {path:15s} {sc.OPS[op][0]:20s} {pos:6s} {pb.fmt_state(w)}")
    paths = ("default_path", "general_kernels")
    assert RECORD["cases"] == {(a, b, p) for a, b in sc.PAIRS for p in paths}, "not every pair ran (a selection, or failures)"
    assert all(RECORD["pending"][a, b, "general_kernels"] for a, b in sc.PAIRS)
    want = {(i, p) for i in range(len(sc.OPS)) for p in paths}
    assert RECORD["first"] == want and RECORD["second"] == want
    print("bound below n before B, at n after it:", len(RECORD["bound_rose"]), "cases, e.g.", RECORD["bound_rose"][:3])
    assert RECORD["bound_rose"]
