"""The filter beside the model of tests/sequence_cases.py: what the GPU modules that run its table share."""
import ctypes as C

import numpy as np

from tests import gpu_support as gs
from tests import hyp_support as hs
from tests import sequence_cases as sc


def source_handles(sd):
    """The handles of sequence_cases.sources(): key -> EkfSlam holding that state and tag index, verbatim."""
    src = {}
    for key, (mean, cov, tags) in sc.sources().items():
        h = sd.EkfSlam(len(mean))
        h.set_state(mean, cov)
        h.set_tag_index(tags)
        got = h.state()
        assert np.array_equal(got[0], mean) and np.array_equal(np.triu(got[1]), np.triu(cov))
        src[key] = h
    return src


def localize_window(f, lin, ang, wins, unmatched):
    """EkfSlam.localize_detections on a device-side window per slot: afterwards every slot's unmatched ids are exactly
    `unmatched[b]`, and its tag table and size what they were (nothing is added on a frozen map)."""
    before = [(f.tag_index(b), f.size(b)) for b in range(f.batch)]
    f.localize_detections(lin, ang, wins)
    assert f.assoc_fallbacks() == 0                        # a device-side window
    for b in range(f.batch):
        got = f.unmatched_tags(b)
        assert got == [int(t) for t in unmatched[b]], f"slot {b}: unmatched tags {got}, the window's unknown ids are {unmatched[b]}"
        assert (f.tag_index(b), f.size(b)) == before[b], f"slot {b}: localize_detections changed the tag table or the size"


def hyp_bank_adopt(sd, f, b, k, drive):
    """A bank of sequence_cases.HYP_COUNT hypotheses on slot b's map as it stands, driven by `drive(bank)`, hypothesis k adopted
    into the slot and the bank closed.  Raw and bit for bit: the adoption left the slot's frozen part alone, and the slot's pose
    mean, block and rows are the hypothesis's."""
    with f.hypotheses(sc.HYP_COUNT, b=b) as bank:
        drive(bank)
        f.covariance_block(0, 0, 3, f.size(b), b)          # (a download mirrors the stored triangle: before the snapshot)
        frozen = hs.frozen_part(sd, f, b)
        bank.adopt(k, f, b)
        assert hs.frozen_same(hs.frozen_part(sd, f, b), frozen), f"slot {b}: adopt moved the slot's map"
        hs.assert_same_bits(bank, k, f, b, f"slot {b} behind adopt({k})")


def hyp_two_steps(motion, one, lists):
    def drive(bank):
        bank.step(*motion[0], *_obs(one))
        bank.step(*motion[1], *(list(x) for x in zip(*(_obs(o) for o in lists))))
    return drive


def hyp_resampled(motion, one, two, pose0, cov0, u, s, z):
    def drive(bank):
        bank.reset(pose0, cov0, k=0)
        bank.step(*motion[0], *_obs(one))
        r = bank.resample(u=u, split=s, z=z)
        assert r.ancestors[0] != 0 and r.offspring[0] == 0 and r.offspring[r.ancestors[0]] >= 2, (r.ancestors, r.offspring)
        bank.step(*motion[1], *_obs(two))
    return drive


def _obs(o):
    return [int(i) for i in o[0]], [float(x) for x in o[1]], [float(x) for x in o[2]]


class Device:
    """The filter beside the model: tests/sequence_model.py's method names on an EkfSlam handle (trajectory 0), the handles
    of sequence_cases.sources() beside it."""

    def __init__(self, sd):
        self.sd, self.f = sd, sd.EkfSlam(sc.N_MAX)
        self.src = source_handles(sd)

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

    def localize1(self, lin, ang, idx, zr, zb):
        self.f.localize(lin, ang, [int(i) for i in idx], [float(x) for x in zr], [float(x) for x in zb])

    def localize_update1(self, idx, zr, zb):
        self.f.localize_update([int(i) for i in idx], [float(x) for x in zr], [float(x) for x in zb])

    def run_localize_stream(self, lin, ang, idx, zr, zb):
        self.f.stream_upload(lin, ang, idx, zr, zb)
        self.f.run_localize(0, len(lin))

    def localize_detections(self, lin, ang, win, unmatched):
        localize_window(self.f, lin, ang, [win], [unmatched])

    def hyp_adopt(self, motion, one, lists, k):
        hyp_bank_adopt(self.sd, self.f, 0, k, hyp_two_steps(motion, one, lists))

    def hyp_resample_adopt(self, motion, one, two, *rest):
        hyp_bank_adopt(self.sd, self.f, 0, 0, hyp_resampled(motion, one, two, *rest))


class BankDevice:
    """The filter beside the BANK model of tests/sequence_bank_cases.py: ONE EkfSlam(N_MAX, batch) and the source handles; the
    model's method names, the targeted ones on slot `target` (BankDriver.retarget sets it), the bank_* ones with one entry per
    slot.  Raw reads per slot, none of which flushes: raw00, pbase, stored_mean, joint_state."""

    def __init__(self, sd, batch=3):
        self.sd, self.f, self.target = sd, sd.EkfSlam(sc.N_MAX, batch=batch), 0
        self.src = source_handles(sd)

    def close(self):
        for h in [self.f] + list(self.src.values()):
            h.close()

    # -- reads ------------------------------------------------------------------------------------------------------------------
    def raw00(self, b):
        return float(gs.raw00(self.sd, self.f, b))

    def pbase(self, b):
        return gs.pbase(self.sd, self.f, b)

    def stored_mean(self, b):
        """The mean buffer the next step reads, raw (all `ld` doubles of slot b)."""
        lib = self.sd.load_library()
        out = np.empty(lib.ekf_debug_snapshot(self.f._h, b, 3, None, 0))
        assert lib.ekf_debug_snapshot(self.f._h, b, 3, out.ctypes.data_as(C.POINTER(C.c_double)), out.size) == out.size
        return out

    def stored_upper(self, b, n):
        """The stored upper triangle of slot b's leading n x n block (P_base is rows x ld here: n_max <= 4096)."""
        ld = len(self.stored_mean(b))
        return np.triu(self.pbase(b).reshape(-1, ld)[:n, :n])

    def joint_state(self, b, perm):
        """Slot b's whole state WITHOUT a download: joint() over the permutation `perm` of all its landmarks, permuted back;
        -> (mean, covariance, tag index, flags)."""
        f = self.f
        mean, cov = sc.unpermute(perm, *f.joint(perm, b))
        return mean, cov, f.tag_index(b), f.flags(b)

    def got(self, b):
        f = self.f
        mean, cov = f.state(b)
        assert f.size(b) == len(mean)
        return mean, cov, f.tag_index(b), f.flags(b)

    # -- handle-wide and targeted calls ---------------------------------------------------------------------------------------
    def set_option(self, name, value):
        self.f.set_option(name, value)

    def set_state_diag(self, mean, diag):
        self.f.set_state_diag(mean, diag, self.target)

    def set_tag_index(self, tags):
        self.f.set_tag_index(tags, self.target)

    def predict_linear(self, pose, F, Q):
        self.f.predict_linear(pose, F, Q, b=self.target)

    def predict_dense1(self, F, Q):
        self.f.predict_dense(F, Q, self.target)

    def update_direct(self, targets, z, R):
        """(the call takes the whole bank: ragged lists, empty for every slot but the target)"""
        ragged = lambda x: [list(x) if b == self.target else [] for b in range(self.f.batch)]
        r = self.f.update_direct(ragged(targets), ragged(z), ragged(R))
        assert r.applied[self.target]

    def update_linear(self, landmarks, H, R, z):
        assert self.f.update_linear(landmarks, H, R, z=z, b=self.target).applied[self.target]

    def transform(self, T, cov=None):
        self.f.transform(T, cov, b=self.target)

    def join(self, key, transform=None, cov=None):
        first = (self.f.size(self.target) - 3) // 2
        r = self.f.join(self.src[key], src=0, dst=self.target, transform=transform, cov=cov)
        assert (r.first, r.count) == (first, (self.src[key].size() - 3) // 2)

    def join_slot(self, src, transform=None, cov=None):
        first = (self.f.size(self.target) - 3) // 2
        r = self.f.join(self.f, src=src, dst=self.target, transform=transform, cov=cov)
        assert (r.first, r.count) == (first, (self.f.size(src) - 3) // 2)

    def fork(self, src, dst):
        self.f.fork(src, dst)

    def remove_landmarks(self, lms):
        self.f.remove_landmarks(lms, self.target)

    def add_landmarks(self, xy):
        self.f.add_landmarks(xy, self.target)

    def copy_in(self, key):
        self.f.copy_from(self.src[key], 0, self.target)

    def hyp_adopt(self, motion, one, lists, k):
        hyp_bank_adopt(self.sd, self.f, self.target, k, hyp_two_steps(motion, one, lists))

    def hyp_resample_adopt(self, motion, one, two, *rest):
        hyp_bank_adopt(self.sd, self.f, self.target, 0, hyp_resampled(motion, one, two, *rest))

    # -- the calls that take the whole bank --------------------------------------------------------------------------------------
    def bank_step(self, lin, ang, obs):
        self.f.step(lin, ang, *self._lists(obs))

    def bank_stream(self, lin, ang, idx, zr, zb, m):
        self.f.run_stream(lin, ang, idx, zr, zb, m)

    def bank_detections(self, lin, ang, wins):
        self.f.step_detections(lin, ang, wins)
        assert self.f.assoc_fallbacks() == 0               # a device-side window

    def bank_localize(self, lin, ang, obs, predict=True):
        if predict:
            self.f.localize(lin, ang, *self._lists(obs))
        else:
            self.f.localize_update(*self._lists(obs))

    def bank_localize_stream(self, lin, ang, idx, zr, zb, m):
        self.f.stream_upload(lin, ang, idx, zr, zb, m)
        self.f.run_localize(0, len(lin))

    def bank_localize_detections(self, lin, ang, wins, unmatched):
        localize_window(self.f, lin, ang, wins, unmatched)

    @staticmethod
    def _lists(obs):
        return ([[int(i) for i in o[0]] for o in obs], [[float(x) for x in o[1]] for o in obs],
                [[float(x) for x in o[2]] for o in obs])
