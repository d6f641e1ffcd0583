"""A stand-in for EkfSlam on the CPU, for the host-side code that drives a bank (evaluation.tune_noise, the fork model's
tests): it records the calls made to it and returns an innovation log that is a known function of its noise rows."""
import numpy as np


class FakeInnov:
    def __init__(self, nis, S):
        self.nis, self.S = nis, S


class FakeBank:
    """Stands in for EkfSlam: records the calls tune_noise makes and returns an innovation log whose NIS of trajectory b
    is a known function of its noise pair."""
    made = []

    def __init__(self, n_max, batch, device, config):
        self.n_max, self.batch = n_max, batch
        self.calls, self.diag = [], {}
        FakeBank.made.append(self)

    def set_noise(self, ms, qs):
        self.ms, self.qs = np.asarray(ms), np.asarray(qs)
        self.calls.append("set_noise")

    def set_state_diag(self, mean, diag, b):
        self.diag[b] = np.asarray(diag).copy()
        self.calls.append("set_state_diag")

    def log_innovations(self, cap):
        self.cap = cap
        self.calls.append("log_innovations")

    def stream_upload(self, lin, ang, idx, zr, zb, m):
        assert lin.shape[1] == self.batch and idx.shape[1] == self.batch
        self.steps = lin.shape[0]
        self.calls.append("stream_upload")

    def stream_run(self, first, count):
        assert (first, count) == (0, self.steps)
        self.calls.append("stream_run")

    def innovations(self, first, count):
        K, B = count, self.batch
        # a log whose loglik peaks at (0.2, 0.5): nis grows away from it, S fixed
        v = 2.0 + 50.0 * ((self.ms - 0.2) ** 2 + (self.qs - 0.5) ** 2)
        nis = np.broadcast_to(v[None, :, None], (K, B, 2)).copy()
        S = np.broadcast_to(np.eye(2), (K, B, 2, 2, 2)).copy()
        return FakeInnov(nis, S)

    def close(self):
        self.calls.append("close")
