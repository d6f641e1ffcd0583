"""The filter beside the model of tests/sequence_cases.py: what the GPU modules that run its table share."""
import ctypes as C

import numpy as np

from tests import sequence_cases as sc


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

    def localize1(self, lin, ang, idx, zr, zb):
        self.f.localize(lin, ang, [int(i) for i in idx], [float(x) for x in zr], [float(x) for x in zb])

    def localize_update1(self, idx, zr, zb):
        self.f.localize_update([int(i) for i in idx], [float(x) for x in zr], [float(x) for x in zb])

    def run_localize_stream(self, lin, ang, idx, zr, zb):
        self.f.stream_upload(lin, ang, idx, zr, zb)
        self.f.run_localize(0, len(lin))
