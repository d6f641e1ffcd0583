"""Per-trajectory noise constants without a device: the C ABI's declarations, the binding's argument checks, and the tuning
sweep's grid assembly on a fake bank."""
import ctypes as C
import re

import numpy as np
import pytest
from tests.fake_bank import FakeBank


def test_noise_symbols_exported_with_declared_signatures():
    import os
    import slam_duckietown_amd as sd
    from slam_duckietown_amd import ekf_bindings as eb
    lib = sd.load_library()
    for name in ("ekf_set_noise", "ekf_get_noise"):
        assert hasattr(lib, name)
        assert eb.ABI[name] == (C.c_int, [C.c_void_p, C.c_int, C.c_int, eb._dp, eb._dp])
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ekfslam_hip.h")).read()
    assert re.search(r"int ekf_set_noise\(ekf_handle \*h, int b0, int count, const double \*motion_sigma, "
                     r"const double \*meas_sigma\);", hdr)
    assert re.search(r"int ekf_get_noise\(ekf_handle \*h, int b0, int count, double \*motion_sigma, double \*meas_sigma\);",
                     hdr)


def test_set_noise_checks_arguments_before_the_library():
    from slam_duckietown_amd import ekf_bindings as eb

    class NoLib:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called ({name})")

    f = eb.EkfSlam.__new__(eb.EkfSlam)
    f.batch = 3
    f._lib, f._h = NoLib(), C.c_void_p()
    for kw in (dict(motion_sigma=[0.1, 0.2]), dict(motion_sigma=np.zeros((3, 1))), dict(meas_sigma=np.ones(4)),
               dict(motion_sigma=[0.1, np.nan, 0.1]), dict(meas_sigma=np.inf), dict(motion_sigma=-0.01),
               dict(meas_sigma=[0.5, 0.0, 0.5]), dict(meas_sigma=-1.0)):
        with pytest.raises(ValueError):
            f.set_noise(**kw)
    ms, qs = eb.EkfSlam.noise_arrays(3, 0.25, [0.5, 0.6, 0.7])
    assert ms.tolist() == [0.25] * 3 and qs.tolist() == [0.5, 0.6, 0.7] and ms.dtype == np.float64
    assert eb.EkfSlam.noise_arrays(3) == (None, None)
    assert eb.EkfSlam.noise_arrays(2, 0.0, 1e-3)[0].tolist() == [0.0, 0.0]     # a zero motion sigma is allowed


def test_tune_noise_grid_assembly_and_argmax():
    import slam_duckietown_amd.evaluation as ev
    FakeBank.made = []
    steps, n = 7, 9
    stream = (np.zeros(steps), np.zeros(steps), np.zeros((steps, 2), dtype=np.int32), np.ones((steps, 2)),
              np.zeros((steps, 2)))
    mg, qg = np.array([0.1, 0.2, 0.4]), np.array([0.3, 0.5])
    diag0 = np.arange(6 * n, dtype=float).reshape(6, n) + 1.0
    res = ev.tune_noise(stream, mg, qg, np.zeros(n), diag0, bank_size=4,
                        filter_factory=lambda n_max, batch, dev, cfg: FakeBank(n_max, batch, dev, cfg))
    assert res.bank_sizes == (3, 3) and [b.batch for b in FakeBank.made] == [3, 3]
    assert res.best == (0.2, 0.5)
    assert res.loglik.shape == (3, 2) and res.traj_anis.shape == (3, 2) and res.traj_bounds.shape == (3, 2, 2)
    for i, s in enumerate(mg):
        for j, q in enumerate(qg):
            v = 2.0 + 50.0 * ((s - 0.2) ** 2 + (q - 0.5) ** 2)
            want = -0.5 * steps * 2 * (v + np.log(np.linalg.det(2 * np.pi * np.eye(2))))
            assert res.loglik[i, j] == pytest.approx(want, rel=1e-12)
            assert res.traj_anis[i, j] == pytest.approx(2 * v, rel=1e-12)
    # grid order: row-major over (motion, measurement); each bank got its own rows of the grid and of diag0
    first, second = FakeBank.made
    assert first.ms.tolist() == [0.1, 0.1, 0.2] and first.qs.tolist() == [0.3, 0.5, 0.3]
    assert second.ms.tolist() == [0.2, 0.4, 0.4] and second.qs.tolist() == [0.5, 0.3, 0.5]
    assert np.array_equal(second.diag[0], diag0[3]) and first.cap == steps
    assert first.calls[0] == "set_noise" and first.calls[-1] == "close"
    one = ev.tune_noise(stream, mg, qg, np.zeros(n), np.ones(n),
                        filter_factory=lambda n_max, batch, dev, cfg: FakeBank(n_max, batch, dev, cfg))
    assert one.bank_sizes == (6,)
    with pytest.raises(ValueError):
        ev.tune_noise(stream, mg, qg, np.zeros(n), np.ones((5, n)), filter_factory=FakeBank)
