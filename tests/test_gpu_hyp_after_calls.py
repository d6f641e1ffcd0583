"""GPU: the hypothesis bank behind and beside the handle's state-changing calls -- what the call tables cannot hold, because
adopt demands the slot's map unchanged (tests/sequence_cases.py puts ekf_hyp_create and ekf_hyp_adopt INTO the tables; there the
map stands still between the two).

A  The snapshot.  Behind each of the 18 older operations of the table, on both paths: a bank of 2 on the map as A left it, then
   the handle runs the table's continuation (a SLAM step and a stream: the map moves).  The bank's poses and rows are bit for bit
   what they were -- nothing the filter does afterwards reaches the bank --, adopt is refused with "not the bank's map", and the
   refusal leaves the slot untouched, by the bits of P_base and of the mean.  The handle's end state is judged against the dense
   model as in the pairs module: a bank alive beside it changes nothing.

B  The bank beside other slots.  In the uneven bank of tests/sequence_bank_cases.py, behind its prelude (on the general kernels
   ranks are pending in every slot), a bank is made on slot 2: ekf_hyp_create flushes the whole handle, and slots 0 and 1, which
   it does not name, obey the bystander rule.  Slot 1 then becomes a fork of slot 2, and one step of the bank -- it names a loose
   landmark: the bound rises -- gives every hypothesis the bits of localize on that fork; the fork is judged against the model.

Every bar is the project's: bit equality, sequence_cases.TOL / ENTRY_TOL, the bystander rule's PATH_TOL."""
import numpy as np
import pytest

from tests import hyp_support as hs
from tests import parity_blocks as pb
from tests import sequence_bank_cases as bc
from tests import sequence_cases as sc
from tests.conftest import path_ran
from tests.gpu_support import pbase
from tests.sequence_device import BankDevice, Device

pytestmark = pytest.mark.gpu

OLDER = 18              # the operations that came before localize_detections and the two hypothesis operations
HANDLES = {}            # (class, path) -> Device / BankDevice


@pytest.fixture(scope="module")
def sd():
    import slam_duckietown_amd as sd
    sd.load_library()
    yield sd
    for dev in HANDLES.values():
        dev.close()
    HANDLES.clear()


def device(sd, cls, path):
    if (cls, path) not in HANDLES:
        HANDLES[cls, path] = cls(sd)
    return HANDLES[cls, path]


def bank_bits(bank):
    pose, cov = bank.poses()
    return pose, cov, np.stack([bank.rows(k) for k in range(bank.count)])


@pytest.mark.parametrize("a", range(OLDER), ids=[sc.query_name(a).replace(" ", "_").replace("/", "-") for a in range(OLDER)])
def test_the_snapshot_outlives_the_map(sd, both_paths, a):
    dev = device(sd, Device, both_paths)
    f, model = dev.f, sc.new_model()
    name = f"{sc.query_name(a)}, {both_paths}"
    try:
        drv = sc.Driver(model, dev)
        rng = np.random.default_rng([sc.SEED, a, 98])
        sc.setup(drv)
        sc.prelude(drv)
        sc.OPS[a][1](drv, rng)
        with f.hypotheses(2) as bank:
            assert bank.n == len(model.tr.mean), f"{name}: the bank has {bank.n} columns, the model {len(model.tr.mean)}"
            for k in range(2):
                hs.assert_same_bits(bank, k, f, 0, f"{name}: seed, hypothesis {k}")
            was = bank_bits(bank)
            sc.continuation(drv, rng)
            pb.assert_state_close(dev.got(), model.state(), sc.INIT_VAR, sc.TOL, sc.ENTRY_TOL, what=f"{name}, after the continuation: ")
            now = bank_bits(bank)
            assert all(np.array_equal(x, y) for x, y in zip(was, now)), f"{name}: the handle's continuation reached the bank"
            f.sync()
            before = pbase(sd, f, 0), f.mean(0)
            with pytest.raises(sd.EkfError, match="not the bank's map"):
                bank.adopt(0, f, 0)
            assert np.array_equal(pbase(sd, f, 0), before[0]) and np.array_equal(f.mean(0), before[1]), f"{name}: the refused adopt wrote the slot"
        assert path_ran(f, both_paths), f"{name}: not the path {both_paths}"
    except AssertionError:
        HANDLES.pop((Device, both_paths)).close()
        raise
    except Exception as e:                                 # a call refused or failed: nothing more is started on this device
        HANDLES.pop((Device, both_paths), None)
        pytest.exit(f"{name}: {type(e).__name__}: {e}", returncode=3)


def test_a_bank_made_beside_slots_with_ranks_pending(sd, both_paths):
    general = both_paths == "general_kernels"
    dev = device(sd, BankDevice, both_paths)
    f, model = dev.f, bc.new_model()
    name = f"a bank on slot 2, {both_paths}"
    others, made, twin = (0, 1), 2, 1
    try:
        drv = bc.BankDriver(model, dev)
        bc.setup(drv)
        bc.prelude(drv)
        perms = np.random.default_rng(16)

        def read(s):
            mean, cov, _, _ = dev.joint_state(s, [int(j) for j in perms.permutation(model.t[s].n_lm)])
            return mean, cov, dev.raw00(s), dev.pbase(s)

        before = {s: read(s) for s in others}
        for s in others:
            pb.assert_state_close(before[s][:2] + (f.tag_index(s), f.flags(s)), model.state(s), sc.INIT_VAR, sc.TOL, sc.ENTRY_TOL,
                                  what=f"{name}: slot {s} before the bank: ")
            if general:
                assert before[s][2] != before[s][1][0, 0], f"{name}: no ranks pending in slot {s}"
        with f.hypotheses(2, b=made) as bank:
            for s in others:
                idle = bc.assert_bystander(before[s], read(s), what=f"{name}: slot {s} behind hyp_create: ")
                assert idle == (not general), f"{name}: slot {s}: nothing pending is {idle}"
            drv.retarget(twin)
            drv.fork(made, twin)
            tr = model.t[made]
            idx = [0, sc.tail_mid(tr), sc.pick(tr)[1]]
            assert idx[2] in pb.loose_landmarks(tr.cov, sc.INIT_VAR)[0]
            o = hs.observe(tr.mean, idx)
            for k in range(2):
                hs.assert_same_bits(bank, k, f, twin, f"{name}: seed, hypothesis {k} against the fork")
            none = [[], [], []]
            drv.bank_localize([0.004] * bc.B, [0.02] * bc.B, [o if s == twin else none for s in range(bc.B)], True)
            bank.step(0.004, 0.02, *o)
            for k in range(2):
                hs.assert_same_bits(bank, k, f, twin, f"{name}: one step, hypothesis {k} against localize on the fork")
            assert bank.rows(0)[:, 3 + 2 * idx[2]:5 + 2 * idx[2]].any(), f"{name}: the step did not reach the loose landmark's columns"
        pb.assert_state_close(dev.got(twin), model.state(twin), sc.INIT_VAR, sc.TOL, sc.ENTRY_TOL, what=f"{name}: the fork after localize: ")
        assert path_ran(f, both_paths), f"{name}: not the path {both_paths}"
    except AssertionError:
        HANDLES.pop((BankDevice, both_paths)).close()
        raise
    except Exception as e:                                 # a call refused or failed: nothing more is started on this device
        HANDLES.pop((BankDevice, both_paths), None)
        pytest.exit(f"{name}: {type(e).__name__}: {e}", returncode=3)
