"""CPU: the host side of device forks (EkfSlam.fork / copy_from, ekf_copy_trajectories) -- evaluation.tune_noise(start=...)
against a NumPy double, the fork model (tests/fork_model.py) under a seeded interleaving, the binding's argument staging
and the C ABI's argument errors (which need no device)."""
import ctypes as C

import numpy as np
import pytest

from tests import fork_model as fm
from tests.fake_bank import FakeBank


class ForkingBank(FakeBank):
    """FakeBank that can be seeded from a running filter, as EkfSlam can."""

    def copy_from(self, other, src=0, dst=0):
        self.seed = (other, src, dst)
        self.calls.append("copy_from")

    def fork(self, src=0, dst=None):
        self.forked = (src, dst)
        self.calls.append("fork")


class Start:
    n_max = 9


def make(n_max, batch, dev, cfg):
    return ForkingBank(n_max, batch, dev, cfg)


def a_stream(steps):
    return (np.zeros(steps), np.zeros(steps), np.zeros((steps, 2), dtype=np.int32), np.ones((steps, 2)), np.zeros((steps, 2)))


def test_tune_noise_start_seeds_by_copy_from_and_fork():
    import slam_duckietown_amd.evaluation as ev
    FakeBank.made = []
    mg, qg = np.array([0.1, 0.2, 0.4]), np.array([0.3, 0.5])
    start = Start()
    res = ev.tune_noise(a_stream(7), mg, qg, None, None, bank_size=4, filter_factory=make, start=(start, 2))
    assert res.bank_sizes == (3, 3) and res.best == (0.2, 0.5)
    for bank in FakeBank.made:
        assert bank.n_max == 9                                     # the start filter's
        assert bank.seed == (start, 2, 0) and bank.forked == (0, None)
        assert "set_state_diag" not in bank.calls
        assert bank.calls == ["set_noise", "copy_from", "fork", "log_innovations", "stream_upload", "stream_run", "close"]
    FakeBank.made = []
    ev.tune_noise(a_stream(7), mg, qg, None, None, n_max=21, filter_factory=make, start=start)     # a bare filter: b = 0
    (bank,) = FakeBank.made
    assert bank.n_max == 21 and bank.seed == (start, 0, 0) and bank.batch == 6


def test_tune_noise_without_start_is_unchanged():
    import slam_duckietown_amd.evaluation as ev
    FakeBank.made = []
    n = 9
    mg, qg = np.array([0.1, 0.2]), np.array([0.3, 0.5])
    res = ev.tune_noise(a_stream(5), mg, qg, np.zeros(n), np.ones(n), filter_factory=make)
    (bank,) = FakeBank.made
    assert bank.calls == ["set_noise"] + ["set_state_diag"] * 4 + ["log_innovations", "stream_upload", "stream_run", "close"]
    assert res.bank_sizes == (4,)
    with pytest.raises((TypeError, ValueError)):
        ev.tune_noise(a_stream(5), mg, qg, None, None, filter_factory=make)     # no start: mean0 is required as before


def test_fork_model_copies_the_state_and_leaves_the_slot():
    m = fm.ForkBank(fm.start_states(6, 3, 40))
    m.set_noise([0.1, 0.2, 0.3], [0.5, 0.6, 0.7])
    m.log_innovations(8)
    m.step(np.full(3, 0.004), np.full(3, 0.02), fm.observations(m, np.random.default_rng(1), 3))
    m.t[0].tags = {7: 2}
    props = fm.slot_properties(m)
    m.fork(0)
    assert fm.slot_properties(m) == props
    for d in (1, 2):
        assert fm.same_state((m.t[d].mean, m.t[d].cov), (m.t[0].mean, m.t[0].cov)) and m.t[d].tags == {7: 2}
        assert m.t[d].mean is not m.t[0].mean
    other = fm.ForkBank(fm.start_states(4, 2, 50))
    other.copy_from(m, [0, 0], [1, 0])
    assert other.t[1].n_lm == 6 and fm.same_state((other.t[0].mean, other.t[0].cov), (m.t[0].mean, m.t[0].cov))
    for bad in (([0], [0]), ([0, 1], [1, 2]), ([0, 0], [1, 1])):
        with pytest.raises(ValueError):
            m.copy_from(m, *bad)
    # twins with different noise rows diverge at the next step
    m.step(np.full(3, 0.004), np.full(3, 0.02), fm.observations(m, np.random.default_rng(2), 3))
    assert not np.array_equal(m.t[0].cov, m.t[1].cov)


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_seeded_interleaving_keeps_the_invariants(seed):
    """step / grow / remove / fork interleaved on the model alone: drive() asserts after every fork that the destinations
    hold the source's bits and that noise rows, rejection counts and the log's step count did not move."""
    m = fm.ForkBank(fm.start_states(8, 4, 100 * seed))
    m.set_noise([0.1, 0.1, 0.2, 0.05], [0.7, 0.7, 0.4, 1.0])
    m.log_innovations(16)
    ran = fm.drive(m, seed, 40, n_cap=14)
    assert ran["fork"] > 0 and ran["step"] > 0
    for tr in m.t:
        assert np.all(np.isfinite(tr.mean)) and np.allclose(tr.cov, tr.cov.T)
    # two slots with equal noise rows that were forked and then only stepped are still twins
    m.fork(0, [1])
    for k in range(5):
        m.step(np.full(4, 0.004), np.full(4, 0.02), fm.observations(m, np.random.default_rng(k), 3))
    assert fm.same_state((m.t[0].mean, m.t[0].cov), (m.t[1].mean, m.t[1].cov))


def test_binding_stages_pairs_without_a_device():
    """copy_from / fork hand (dst, src, k) to the library in the C ABI's order; lengths are checked before the call."""
    from slam_duckietown_amd import ekf_bindings as eb
    assert eb.ABI["ekf_copy_trajectories"][1] == [C.c_void_p, eb._ip, C.c_void_p, eb._ip, C.c_int]
    seen = []

    class Lib:
        def ekf_copy_trajectories(self, dh, d, sh, s, k):
            seen.append((dh, [d[i] for i in range(k)], sh, [s[i] for i in range(k)], k))
            return 0

    def handle(batch, h):
        f = eb.EkfSlam.__new__(eb.EkfSlam)
        f._lib, f._h, f.batch, f._host_index, f._host_tags = Lib(), h, batch, {}, {}
        return f

    f, g = handle(4, "F"), handle(2, "G")
    f.fork(2)
    assert seen.pop() == ("F", [0, 1, 3], "F", [2, 2, 2], 3)
    f.fork(0, 3)
    assert seen.pop() == ("F", [3], "F", [0], 1)
    g._host_index[1] = {5000: 0}
    g._host_tags[1] = {0: [1.0]}
    f._host_tags[2] = {3: [2.0]}
    f.copy_from(g, [1, 0], [0, 2])
    assert seen.pop() == ("F", [0, 2], "G", [1, 0], 2)
    assert f._host_index == {0: {5000: 0}} and f._host_tags == {0: {0: [1.0]}}      # the host association's tables follow
    with pytest.raises(ValueError):
        f.copy_from(g, [0, 1], [0])
    for b in (f, g):
        b._h = None                                               # (nothing to destroy)


def test_argument_errors_need_no_device():
    """The C ABI refuses NULL handles before it touches a device."""
    import __graft_entry__ as ge
    import slam_duckietown_amd as sd
    import os
    if not os.path.exists(sd.library_path()):
        ge.build()
    lib = sd.load_library()
    assert lib.ekf_copy_trajectories(None, None, None, None, 0) == -1
