"""CPU: map joining (EkfSlam.join, ekf_join_maps) without a device -- the model's two forms against each other
(tests/join_model.py), plan_join and the tile enumeration of k_join under the sanitizers (tests/join_plan_check.cpp), the
binding's argument staging with a fake library, and the C ABI's argument errors that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import host_check
from tests import join_model as jm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cases():
    rng = np.random.default_rng(2024)
    for it in range(400):
        NA, NB = int(rng.integers(0, 6)), int(rng.integers(0, 6))
        never = int(rng.integers(0, NB)) if NB and it % 3 == 0 else None
        xA, PA = jm.random_state(rng, NA)
        xB, PB = jm.random_state(rng, NB, never_observed=never)
        T, cT = jm.random_frame(rng)
        if it % 5 == 0:
            cT = np.zeros((3, 3))
        yield (xA, PA, xB, PB) + ((None, None) if it % 2 else (T, cT))


def test_the_two_forms_agree_within_the_bound():
    """Dense J P_in J^T against the closed form, entrywise within 1e-14 x |J| |P_in| |J|^T; the joined covariance is
    positive definite (Cholesky), also with a never-observed landmark of variance 1e4 in the source."""
    worst, seen = 0.0, set()
    for xA, PA, xB, PB, T, cT in cases():
        md, Pd, bound, mbound = jm.join_dense(xA, PA, xB, PB, T, cT)
        mc, Pc = jm.join_closed(xA, PA, xB, PB, T, cT)
        assert np.array_equal(md, mc)
        assert (np.abs(Pd - Pc) <= 1e-14 * bound).all()
        assert (np.abs(mbound) >= np.abs(md) * (mbound > 0)).all()
        worst = max(worst, float(np.max(np.abs(Pd - Pc) / np.where(bound > 0, bound, 1.0))))
        np.linalg.cholesky((Pc + Pc.T) / 2)                       # raises unless positive definite
        assert Pc.shape == (len(xA) + len(xB) - 3,) * 2 and np.allclose(Pc, Pc.T, rtol=0, atol=1e-12 * np.abs(Pc).max())
        seen.add((len(xA), len(xB), T is None))
    print("worst |dense - closed| / bound:", worst)
    assert {(3, 3, True), (3, 3, False)} <= seen and len(seen) > 50


def test_what_stays_stays():
    rng = np.random.default_rng(7)
    xA, PA = jm.random_state(rng, 4)
    xB, PB = jm.random_state(rng, 3)
    m, P = jm.join_closed(xA, PA, xB, PB)                         # sequential
    assert np.array_equal(P[3:11, 3:11], PA[3:, 3:]) and np.array_equal(m[3:11], xA[3:])
    assert not np.array_equal(m[:3], xA[:3])
    T, cT = jm.random_frame(rng)
    m, P = jm.join_closed(xA, PA, xB, PB, T, cT)                  # explicit
    assert np.array_equal(P[:11, :11], PA) and np.array_equal(m[:11], xA) and not P[:11, 11:].any()
    m, P = jm.join_closed(xA, PA, xB, PB, np.zeros(3), np.zeros((3, 3)))
    assert np.array_equal(P[11:, 11:], PB[3:, 3:]) and np.array_equal(m[11:], xB[3:])
    m, P = jm.join_closed(xA, PA, xB[:3], PB[:3, :3])             # N_B = 0: the pose alone
    assert P.shape == (11, 11) and np.array_equal(P[3:, 3:], PA[3:, 3:])
    # composing with a source at the origin with no uncertainty changes nothing but rounding
    m, P = jm.join_closed(xA, PA, np.zeros(3), np.zeros((3, 3)))
    assert np.allclose(m, xA, rtol=0, atol=1e-15) and np.allclose(P, PA, rtol=1e-14, atol=1e-15)


def test_plan_join_under_the_sanitizers(tmp_path):
    host_check.run_under_sanitizers("join_plan_check", tmp_path, 600)
    api = open(os.path.join(ROOT, "slam-duckietown_amd", "csrc", "ekf_api.hip")).read()
    assert re.search(r"\bplan_join\(", api) and not re.search(r"^(static|inline)[^\n;]*\bplan_join\(", api, flags=re.M)
    # the snapshot buffer and the table are owned through the types of ekf_resources.h
    assert re.search(r"DeviceBuf<double> djn_snap;", api) and re.search(r"DeviceBuf<int> djn_tab;", api)
    mk = open(os.path.join(ROOT, "slam-duckietown_amd", "csrc", "Makefile")).read()
    assert "ekf_join.hip" in mk


def test_binding_stages_pairs_without_a_device():
    """join hands (dst, src, k, T, covT, first, twin, stride) to the library in the C ABI's order; scalars for one pair given
    as ints, arrays for several; lengths are checked before the call."""
    from slam_duckietown_amd import ekf_bindings as eb
    import slam_duckietown_amd as sd
    assert eb.ABI["ekf_join_maps"][1] == [C.c_void_p, eb._ip, C.c_void_p, eb._ip, C.c_int, eb._dp, eb._dp, eb._ip, eb._ip, C.c_int]
    assert eb.MapJoin._fields == ("first", "count", "twins") and sd.MapJoin is eb.MapJoin
    seen = []

    class Lib:
        sizes = {"F": [3 + 2 * 5, 3, 3 + 2 * 2, 3 + 2 * 7], "G": [3 + 2 * 3, 3 + 2 * 4]}

        def ekf_state_size(self, h, b, out):
            out._obj.value = self.sizes[h][b]
            return 0

        def ekf_join_maps(self, dh, d, sh, s, k, T, cT, first, twin, stride):
            seen.append((dh, [d[i] for i in range(k)], sh, [s[i] for i in range(k)], k,
                         None if T is None else [T[i] for i in range(3 * k)], None if cT is None else [cT[i] for i in range(9 * k)],
                         stride))
            for i in range(k):
                first[i] = (self.sizes[dh][d[i]] - 3) // 2
                twin[i * stride] = 1
            return 0

    def handle(batch, h):
        f = eb.EkfSlam.__new__(eb.EkfSlam)
        f._lib, f._h, f.batch, f._host_index, f._host_tags = Lib(), h, batch, {}, {}
        return f

    f, g = handle(4, "F"), handle(2, "G")
    r = f.join(g, 1, 0)
    assert seen.pop() == ("F", [0], "G", [1], 1, None, None, 4)
    assert (r.first, r.count) == (5, 4) and r.twins.tolist() == [1, -1, -1, -1] and isinstance(r.first, int)
    r = f.join(g, [0, 0], [2, 3], transform=[1.0, 2.0, 0.5])
    assert seen.pop() == ("F", [2, 3], "G", [0, 0], 2, [1.0, 2.0, 0.5] * 2, [0.0] * 18, 3)
    assert r.first.tolist() == [2, 7] and r.count.tolist() == [3, 3] and r.twins.shape == (2, 3)
    cov = np.diag([0.1, 0.2, 0.3])
    f.join(f, [1], [0], transform=np.zeros((1, 3)), cov=cov)
    assert seen.pop() == ("F", [0], "F", [1], 1, [0.0] * 3, cov.ravel().tolist(), 1)
    with pytest.raises(ValueError):
        f.join(g, [0, 1], [0])
    with pytest.raises(ValueError):
        f.join(g, 0, 0, cov=cov)
    assert not seen
    for b in (f, g):
        b._h = None                                               # (nothing to destroy)


def test_argument_errors_need_no_device():
    """The C ABI refuses NULL handles before it touches a device, and the symbol is exported."""
    import __graft_entry__ as ge
    import slam_duckietown_amd as sd
    if not os.path.exists(sd.library_path()):
        ge.build()
    lib = sd.load_library()
    assert lib.ekf_join_maps(None, None, None, None, 0, None, None, None, None, 0) == -1
    header = open(os.path.join(ROOT, "include", "ekfslam_hip.h")).read()
    assert "int ekf_join_maps(ekf_handle *dst, const int *dst_b, ekf_handle *src, const int *src_b, int k," in header
