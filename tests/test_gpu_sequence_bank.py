"""GPU: the ordered pairs of state-changing calls in an UNEVEN BANK, call A on one slot and call B on another, against ONE dense
model of the bank (tests/sequence_bank_cases.py has the table and the reasons, tests/sequence_model.py the model,
tests/test_sequence_bank_cpu.py shows that the 529 cases are admissible and the judge not blind).

Per case: three slots of 63, 47 and 71 states in ONE handle, the prelude for the whole bank (on the general kernels ranks are
pending in every slot), operation A on slot 0 or 2, operation B on the other, then a continuation over the whole bank.

After A and after B there is NO download: every slot's whole state is read through joint() over a permutation of all its
landmarks and judged by parity_blocks.assert_state_close against its model slot -- TOL, ENTRY_TOL, exact symmetry, exact zeros,
size, tag index, flags -- so B starts on whatever A left pending in every slot.  After the continuation state(b) of every slot,
under the same judge; on the general kernels a pass kernel has run and the stored P_base[0, 0] of every slot is the downloaded
one.  Behind a localisation operation -- localize_detections and the two hypothesis-bank operations among the six -- nothing is
pending in any slot.

Around every TARGETED call -- hyp_adopt and hyp_resample_adopt are two: the bank is made on the target slot and adopted into
it --, every slot the call does not name is held to the bystander rule (sequence_bank_cases.
assert_bystander): mean bit for bit, covariance within PATH_TOL of the read before the call, and the stored P_base untouched
where nothing was pending.  Behind fork the target's stored triangle and mean are slot 1's over slot 1's size, bit for bit.

Two more cases (run_edge_case) raise slot 2's bound over the 64-column tile edge behind a linear / direct update, where every
slot's bound lay below it: the one thing the pairs cannot show of front_run's per-slot mirror (profiles/sequence_bank.txt).

Time on one MI355X: 21 s for the 1063 tests, 0.064 s for the slowest case (14 s for 805 before the last three operations).

The handles are made once per path and every case resets them; a failed assertion drops them, any other exception ends the
session: nothing more is started on a device after a refused or failed call."""
import time

import numpy as np
import pytest

from tests import parity_blocks as pb
from tests import sequence_bank_cases as bc
from tests import sequence_cases as sc
from tests.conftest import path_ran
from tests.sequence_device import BankDevice

pytestmark = pytest.mark.gpu

PATHS = ("default_path", "general_kernels")
HANDLES = {}            # path -> BankDevice
RECORD = {"cases": set(), "positions": set(), "hands": [], "pending_at_B": [], "idle_calls": {p: 0 for p in PATHS},
          "pending_calls": {p: 0 for p in PATHS}, "loc_idle": set(), "worst": {}, "seconds": {}}


@pytest.fixture(scope="module")
def sd():
    import slam_duckietown_amd as sd
    sd.load_library()
    yield sd
    for dev in HANDLES.values():
        dev.close()
    HANDLES.clear()


def check(sd, both_paths, name, ops, slots_of, runner, seed):
    """One case on the filter and the model: `runner(driver, judge)` drives it; ops: stage -> index into bc.OPS (the stages
    whose worst pieces are recorded under an operation), slots_of: stage -> the slot its operation names.  -> {stage: sizes}."""
    general = both_paths == "general_kernels"
    dev = HANDLES.get(both_paths) or HANDLES.setdefault(both_paths, BankDevice(sd, bc.B))
    model = bc.new_model()
    perms = np.random.default_rng(seed)
    armed, around, sizes, p00 = [False], {}, {}, {}
    t0 = time.perf_counter()

    def read(s):
        """Slot s without a download: (mean, covariance, tag index, flags) through joint(), the stored P_base[0, 0]."""
        perm = [int(j) for j in perms.permutation(model.t[s].n_lm)]
        return dev.joint_state(s, perm), dev.raw00(s)

    def observer(when, call, slot):
        if not armed[0] or slot is None:
            return
        others = [s for s in range(bc.B) if s != slot]
        if when == "before":
            for s in others:
                (mean, cov, _, _), raw = read(s)
                around[s] = (mean, cov, raw, dev.pbase(s))
            return
        for s in others:
            (mean, cov, _, _), raw = read(s)
            idle = bc.assert_bystander(around[s], (mean, cov, raw, dev.pbase(s)), what=f"{name}: slot {s} behind {call} on slot {slot}: ")
            RECORD["idle_calls" if idle else "pending_calls"][both_paths] += 1
        if call == "fork":
            n = dev.f.size(bc.BYSTANDER)
            assert dev.f.size(slot) == n, f"{name}: fork: the twin has {dev.f.size(slot)} states, slot 1 has {n}"
            assert np.array_equal(dev.stored_upper(slot, n), dev.stored_upper(bc.BYSTANDER, n)), f"{name}: fork: the twin's stored P_base is not slot 1's"
            assert np.array_equal(dev.stored_mean(slot)[:n], dev.stored_mean(bc.BYSTANDER)[:n]), f"{name}: fork: the twin's stored mean is not slot 1's"

    def record(stage, s, err):
        for pos, op in ops.items():
            w = RECORD["worst"].setdefault((both_paths, op, pos, s), {})
            for p, v in err.items():
                w[p] = max(w.get(p, 0.0), v)

    def judge(stage):
        if stage == "start":
            # ranks pending: the stored P_base[0, 0] is not the covariance's (the pairs module's criterion), in every slot
            for s in range(bc.B):
                raw, want = dev.raw00(s), float(model.t[s].cov[0, 0])
                if general:
                    assert abs(raw - want) > 1e-6 * want, f"{name}: no ranks pending at A in slot {s} (P_base[0, 0] = {raw}, P[0, 0] = {want})"
            armed[0] = True
            return
        armed[0] = stage != "end"
        op = bc.OPS[ops[stage]][0] if stage in ops else None
        sizes[stage] = []
        for s in range(bc.B):
            what = f"{name}, after {stage}, slot {s}: "
            got, raw = (dev.got(s), None) if stage == "end" else read(s)
            n = dev.f.size(s)
            assert n == len(model.t[s].mean), f"{what}size: {n} where the model has {len(model.t[s].mean)}"
            sizes[stage].append(n)
            record(stage, s, pb.assert_state_close(got, model.state(s), sc.INIT_VAR, sc.TOL, sc.ENTRY_TOL, what=what))
            if stage == "end":
                p00[s] = float(got[1][0, 0])
                continue
            pending = raw != got[1][0, 0]
            if general and op in sc.LOCALIZE_OPS:
                assert not pending, f"{what}{op} left something pending (P_base[0, 0] = {raw}, P[0, 0] = {got[1][0, 0]})"
                RECORD["loc_idle"].add((op, stage, s))
            if general and stage == "A" and "B" in slots_of and s != slots_of["B"] and pending:
                RECORD["pending_at_B"].append((name, s))
        assert path_ran(dev.f, both_paths), f"{name}, after {stage}: not the path {both_paths}"

    try:
        runner(bc.BankDriver(model, dev, observer=observer), judge)
        if general:
            # the continuation ended in a covariance pass: a pass kernel has run, and nothing is pending behind the downloads
            assert "k_flush" in dev.f.last_pass(), f"{name}: the continuation ended in no covariance pass"
            for s in range(bc.B):
                assert dev.raw00(s) == p00[s], f"{name}: ranks pending in slot {s} behind the last download"
    except AssertionError:
        HANDLES.pop(both_paths).close()
        raise
    except Exception as e:                                 # a call refused or failed: nothing more is started on this device
        HANDLES.pop(both_paths, None)
        pytest.exit(f"{name}: {type(e).__name__}: {e}", returncode=3)
    return sizes, time.perf_counter() - t0


@pytest.mark.parametrize("a,b", bc.PAIRS, ids=[bc.pair_id(a, b) for a, b in bc.PAIRS])
def test_pair(sd, both_paths, a, b):
    name = f"{bc.pair_name(a, b)}, {both_paths}"
    slots_of = dict(zip(("A", "B"), bc.targets(a, b)))
    sizes, seconds = check(sd, both_paths, name, {"A": a, "B": b}, slots_of, lambda drv, judge: bc.run_case(drv, a, b, judge), [14, a, b])
    RECORD["cases"].add((a, b, both_paths))
    for pos, op in (("A", a), ("B", b)):
        RECORD["positions"].add((op, pos, slots_of[pos], both_paths))
    if int(np.argmax(sizes["B"])) != int(np.argmax([len(s[0]) for s in bc.starts()])):
        RECORD["hands"].append((name, sizes["B"]))
    RECORD["seconds"][a, b, both_paths] = seconds


@pytest.mark.parametrize("i", range(len(bc.EDGE_OPS)), ids=[n.replace(", ", "+") for n, _ in bc.EDGE_OPS])
def test_a_front_raises_one_slots_bound_over_the_tile_edge(sd, both_paths, i):
    """sequence_bank_cases.run_edge_case: every slot's bound lies below column 64, then a front on slot 2 names landmark 31 --
    the pass behind it needs one 64-column tile more than any slot had (front_run's neff_enq, for the slot the call names)."""
    name = f"{bc.EDGE_OPS[i][0]} of landmark {bc.EDGE_LANDMARK} on slot {bc.EDGE_SLOT}, {both_paths}"
    check(sd, both_paths, name, {}, {"A": bc.EDGE_SLOT}, lambda drv, judge: bc.run_edge_case(drv, i, judge), [15, i])


def test_the_module_kept_its_promises():
    """All 529 pairs ran on both paths; each of the 23 operations ran in both positions on both acting slots; the largest state changed
    slots in some case; on the general kernels some case had ranks pending in the slots B does not name when B ran; the
    bystander's P_base comparison was exercised (nothing pending at a targeted call) on both paths, and so was the bound for
    pending ranks on the general kernels; nothing was pending, in any slot, behind any of the six localisation-like
    operations.  Prints the worst
    of every piece per operation, position and slot, and the time (profiles/sequence_bank.txt)."""
    for (path, op, pos, s), w in sorted(RECORD["worst"].items()):
        print(f"DEVICE {path:15s} {bc.OPS[op][0]:20s} {pos} slot {s} {pb.fmt_state(w)}")
    sec = RECORD["seconds"]
    if sec:
        slow = max(sec, key=sec.get)
        print(f"TIME {len(sec)} cases in {sum(sec.values()):.2f} s; the slowest, {bc.pair_name(*slow[:2])} on {slow[2]}: {sec[slow]:.3f} s")
    print("bystander reads around targeted calls, nothing pending / ranks pending:", RECORD["idle_calls"], RECORD["pending_calls"])
    print("the largest state changed slots:", len(RECORD["hands"]), "cases, e.g.", RECORD["hands"][:2])
    print("ranks pending beside B's slot when B ran:", len(RECORD["pending_at_B"]), "slot reads, e.g.", RECORD["pending_at_B"][:2])
    assert RECORD["cases"] == {(a, b, p) for a, b in bc.PAIRS for p in PATHS}, "not every pair ran (a selection, or failures)"
    assert RECORD["positions"] == {(op, pos, s, p) for op in range(len(bc.OPS)) for pos in ("A", "B") for s in bc.ACTING for p in PATHS}
    assert RECORD["hands"]
    assert RECORD["pending_at_B"]
    assert all(RECORD["idle_calls"][p] > 0 for p in PATHS) and RECORD["pending_calls"]["general_kernels"] > 0
    assert RECORD["pending_calls"]["default_path"] == 0       # (the small-state path never has ranks pending)
    assert RECORD["loc_idle"] == {(op, st, s) for op in sc.LOCALIZE_OPS for st in ("A", "B") for s in range(bc.B)}
