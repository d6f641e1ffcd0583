"""GPU: every ordered pair of state-changing calls against ONE dense model (tests/sequence_cases.py has the table and the
reasons, tests/sequence_model.py the model, tests/test_sequence_cpu.py shows that the 441 cases are admissible and the judge
not blind).

Per case: the block-diagonal start, 28 stream steps and three single steps (on the general kernels ranks are pending),
operation A, operation B, then a continuation (a step and a 4-step stream) -- judged after A, after B and after the
continuation with parity_blocks.assert_state_close: the informed part piece by piece at 1e-9, the loose landmarks on their
own scale, exact zeros, exact symmetry, size, tag index, flags.  A stale bound, floor or size word left by A shows in B or in
the continuation's pass; the failure carries the pair's name.

Localisation (the last six operations: localize, localize_update, run_localize, localize_detections and the two that make a
hypothesis bank on the map as it stands and adopt one hypothesis back, hyp_adopt and hyp_resample_adopt) applies what is pending
at entry and appends no rank: on the general kernels the stored P_base[0, 0] read BEFORE the download behind such an A or B is
the downloaded P[0, 0], bit for bit.  The filter's side of those three asserts more than the state (tests/sequence_device.py):
the unmatched ids, the tag table and the size around localize_detections; around adopt the slot's frozen part and the adopted
pose part, raw and bit for bit.

The handles are made once per path and every case resets them (set_option, set_state_diag, set_tag_index: part of the
surface under test); a case that fails drops them, so that the next one starts from new handles."""
import numpy as np
import pytest

from tests import parity_blocks as pb
from tests import sequence_cases as sc
from tests.conftest import path_ran
from tests.sequence_device import Device

pytestmark = pytest.mark.gpu

HANDLES = {}            # path -> Device
RECORD = {"cases": set(), "pending": {}, "first": set(), "second": set(), "bound_rose": [], "worst": {}, "nothing_pending": set()}


@pytest.fixture(scope="module")
def sd():
    import slam_duckietown_amd as sd
    sd.load_library()
    yield sd
    for dev in HANDLES.values():
        dev.close()
    HANDLES.clear()


@pytest.mark.parametrize("a,b", sc.PAIRS, ids=[sc.pair_name(a, b).replace(" ", "_").replace("/", "-") for a, b in sc.PAIRS])
def test_pair(sd, both_paths, a, b):
    general = both_paths == "general_kernels"
    dev = HANDLES.get(both_paths) or HANDLES.setdefault(both_paths, Device(sd))
    model = sc.new_model()
    name = f"{sc.pair_name(a, b)}, {both_paths}"
    bounds = {}

    def judge(stage):
        tr = model.tr
        bounds[stage] = (sc.model_bound(tr), len(tr.mean))
        if stage == "start":
            # ranks pending: the stored P_base[0, 0] is not the covariance's.  The model and the filter agree to 1e-9 (asserted
            # after A), one pending single step alone adds 0.01 of pose noise: a difference above 1e-6 is what is pending
            raw, want = dev.raw00(), float(tr.cov[0, 0])
            RECORD["pending"][a, b, both_paths] = abs(raw - want) > 1e-6 * want
            if general:
                assert RECORD["pending"][a, b, both_paths], f"{name}: no ranks pending at A (P_base[0, 0] = {raw}, P[0, 0] = {want})"
            return
        op = sc.OPS[a if stage == "A" else b][0] if stage in ("A", "B") else None
        raw = dev.raw00()
        got = dev.got()
        if general and op in sc.LOCALIZE_OPS:
            assert raw == got[1][0, 0], f"{name}, after {stage}: {op} left something pending (P_base[0, 0] = {raw}, P[0, 0] = {got[1][0, 0]})"
            RECORD["nothing_pending"].add((op, stage))
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
    """Every one of the 441 pairs ran on both paths; ranks were pending at A in every general-kernels case; each of the 21
    operations ran in both positions on both paths; some case left the bound below n before B raised it; nothing was pending
    behind any of the six localisation-like operations, first or second.  Prints the worst of every piece per operation and position (profiles/sequence_pairs.txt)."""
    for (path, pos, op), w in sorted(RECORD["worst"].items()):
        print(f"DEVICE {path:15s} {sc.OPS[op][0]:20s} {pos:6s} {pb.fmt_state(w)}")
    paths = ("default_path", "general_kernels")
    assert RECORD["cases"] == {(a, b, p) for a, b in sc.PAIRS for p in paths}, "not every pair ran (a selection, or failures)"
    assert all(RECORD["pending"][a, b, "general_kernels"] for a, b in sc.PAIRS)
    want = {(i, p) for i in range(len(sc.OPS)) for p in paths}
    assert RECORD["first"] == want and RECORD["second"] == want
    print("bound below n before B, at n after it:", len(RECORD["bound_rose"]), "cases, e.g.", RECORD["bound_rose"][:3])
    assert RECORD["bound_rose"]
    assert RECORD["nothing_pending"] == {(op, st) for op in sc.LOCALIZE_OPS for st in ("A", "B")}
