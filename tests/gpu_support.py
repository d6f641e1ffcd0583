"""What a GPU test needs from a handle: the `sd` fixture, raw reads of P_base, the debug counters under their names, and the
comparisons the test files share.  A test module takes the fixture with `from tests.gpu_support import sd  # noqa: F401`
(pytest finds a fixture by its name in the module's namespace)."""
import ctypes as C
from types import SimpleNamespace as NS
from typing import NamedTuple

import numpy as np
import pytest

from oracle import ekf_oracle as orc

REL_TOL = 1e-6          # the north-star bar (BASELINE.json): never relaxed, whatever `tol` says
TIGHT = 1e-9


@pytest.fixture(scope="module")
def sd():
    import slam_duckietown_amd as sd
    sd.load_library()
    return sd


def tag(i, x, z):
    """A detection of tag i at (x, z) in the camera frame, as step_detections takes them."""
    return NS(tag_id=i, pose_R=np.eye(3), pose_t=np.array([[x], [0.0], [z]]), pose_err=0.0)


def raw00(sd, f, b=0):
    """P_base[0, 0] of trajectory b as stored (no flush)."""
    out = np.empty(1)
    sd.load_library().ekf_debug_snapshot(f._h, b, 0, out.ctypes.data_as(C.POINTER(C.c_double)), 1)
    return out[0]


def pbase(sd, f, b, count=None):
    """P_base of trajectory b (its leading `count` doubles, if given), raw, no flush"""
    lib = sd.load_library()
    have = lib.ekf_debug_snapshot(f._h, b, 0, None, 0)
    out = np.empty(have if count is None else min(have, count))
    assert lib.ekf_debug_snapshot(f._h, b, 0, out.ctypes.data_as(C.POINTER(C.c_double)), out.size) == have
    return out


def same(a, b):
    """Two (mean, covariance) pairs, bit for bit."""
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def col(x):
    return x[:, None]


def close(a, b, tol=TIGHT):
    r = orc.rel_fro(a, b)
    assert r < REL_TOL, f"rel Frobenius {r:.3e} exceeds the 1e-6 bar"
    assert r < tol, f"rel Frobenius {r:.3e} exceeds the expected {tol:g}"


def within_bounds(got, xm, Pm, bound, mbound, tol, label=""):
    """The state `got` against a dense model's (xm, Pm), entrywise within tol x the model's own bounds, and exactly
    symmetric; prints the worst ratio to the bound before it asserts."""
    assert got[0].shape == xm.shape and got[1].shape == Pm.shape
    eP, em = np.abs(got[1] - Pm), np.abs(got[0] - xm)
    rP = float(np.max(eP / np.where(bound > 0, bound, 1.0))) if eP.size else 0.0
    rm = float(np.max(em / np.where(mbound > 0, mbound, 1.0))) if em.size else 0.0
    print(f"{label}: worst covariance error / bound {rP:.3g}, mean {rm:.3g}")
    assert (eP <= tol * bound).all() and (em <= tol * mbound).all()
    assert np.array_equal(got[1], got[1].T)


class Counters(NamedTuple):
    """The handle's debug counters: which path ran, and how often."""
    cadences: int               # ekf_debug_cadences: fused cadences launched ...
    covered: int                # ... and the steps of the uploaded stream they covered
    chained: int                # ekf_debug_chained
    lookaheads: int             # ekf_debug_lookaheads
    passes: int                 # profile_passes(): covariance passes since profiling was enabled
    small_launches: int         # ekf_debug_small_launches
    fused_fetches: int          # ekf_debug_fused_fetches
    w_from_v: int               # ekf_debug_w_from_v
    last_pass: str              # last_pass(): the kernel of the last covariance pass, '' if none yet


def counters(sd, f):
    lib = sd.load_library()
    a, b = C.c_long(), C.c_long()
    assert lib.ekf_debug_cadences(f._h, C.byref(a), C.byref(b)) == 0
    return Counters(a.value, b.value, lib.ekf_debug_chained(f._h), lib.ekf_debug_lookaheads(f._h), f.profile_passes(),
                    lib.ekf_debug_small_launches(f._h), lib.ekf_debug_fused_fetches(f._h), lib.ekf_debug_w_from_v(f._h),
                    f.last_pass())


def scheduling(sd, f):
    """The counters without what names the last pass's kernel: what the innovation log and the NIS gate are compared on."""
    return counters(sd, f)._replace(w_from_v=None, last_pass=None)


def final(sd, f, read=scheduling):
    """Everything a log must not change: every trajectory's state and flags, and the scheduling counters (`read`: which)."""
    return [f.state(b) for b in range(f.batch)], [f.flags(b) for b in range(f.batch)], read(sd, f)


def same_bits(a, b):
    (sa, fa, ca), (sb, fb, cb) = a, b
    for (ma, Pa), (mb, Pb) in zip(sa, sb):
        assert np.array_equal(ma, mb) and np.array_equal(Pa, Pb)
    assert fa == fb and ca == cb


def bank(sd, streams, steps=None, config=None, run=True, options=()):
    """A bank over `streams` (one synthetic stream per trajectory, equal shapes), the whole stream uploaded and its first
    `steps` steps run."""
    B, n = len(streams), len(streams[0][0])
    f = sd.EkfSlam(n, batch=B, config=config)
    for name, value in options:
        f.set_option(name, value)
    for b, s in enumerate(streams):
        f.set_state_diag(s[0], s[1], b)
    f.stream_upload(np.stack([s[2] for s in streams], 1), np.stack([s[3] for s in streams], 1),
                    np.stack([s[4] for s in streams], 1), np.stack([s[5] for s in streams], 1),
                    np.stack([s[6] for s in streams], 1))
    if run:
        f.stream_run(0, steps if steps is not None else len(streams[0][2]))
    return f
