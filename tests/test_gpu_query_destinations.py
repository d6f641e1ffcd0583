"""GPU: where the read-only queries write (ekf_download_marginals, ekf_associate, ekf_download_joint through ctypes).

A pinned destination (ekf_host_alloc) is written by the kernels in place, an ordinary one through the handle's staging buffer
and one copy.  One bank of three trajectories with 5, 40 and 17 landmarks (n_max = 83: the general kernels), three steps
enqueued and not flushed: every combination of pinned and ordinary destinations returns the same bits -- the NaN padding
beyond a trajectory's own landmarks included -- and the bits the binding returns; the three queries share one staging buffer
that grows and is reused; none of it touches the filter, which then flushes to the oracle's state."""
import ctypes as C
import itertools

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests.gpu_support import pbase, sd  # noqa: F401

pytestmark = pytest.mark.gpu

TIGHT = 1e-9                # tests/test_gpu_marginals.py: a flushed state against the dense oracle
SIZES = (5, 40, 17)         # landmarks per trajectory
N_MAX = 3 + 2 * 40
STEPS = 3
B = len(SIZES)
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def world():
    """The three trajectories' streams, the oracle's state behind them (computed once, never written) and the queries' inputs."""
    streams = [orc.synthetic_stream(N, STEPS, min(8, N - 1), 70 + b) for b, N in enumerate(SIZES)]
    cfg = orc.EkfConfig()
    oracle = []
    for s in streams:
        om, oP = s[0].copy(), np.diag(s[1])
        for k in range(STEPS):
            om, oP = orc.ekf_step_dense(om, oP, s[2][k], s[3][k], s[4][k], s[5][k], s[6][k], cfg)
        oracle.append((om, oP))
    rng = np.random.default_rng(3)
    S = 4
    zr, zb = np.zeros((B, S)), np.zeros((B, S))
    for b, (om, _) in enumerate(oracle):                # observations of random landmarks from the oracle's pose, perturbed
        for q in range(S):
            d = om[3 + 2 * int(rng.integers(SIZES[b])):][:2] - om[:2] + rng.normal(0, 0.05, 2)
            zr[b, q], zb[b, q] = np.hypot(*d), orc.wrap_pi(np.arctan2(d[1], d[0]) - om[2])
    return dict(streams=streams, oracle=oracle, zr=zr, zb=zb, m=np.array([4, 3, 0], dtype=np.int32),
                sels=[[0, 3], [5, 39, 12, 1], [16, 2, 7]])


def make_filter(sd, world):
    """A handle with the three steps enqueued on the per-step kernels, ranks pending."""
    f = sd.EkfSlam(N_MAX, batch=B)
    f.set_option("fused_cadence", 0)
    f.profile_enable(True)
    for b, s in enumerate(world["streams"]):
        f.set_state_diag(s[0], s[1], b)
    for k in range(STEPS):
        col = lambda i: [s[i][k] for s in world["streams"]]
        f.step(np.array(col(2)), np.array(col(3)), col(4), col(5), col(6))
    return f


class Arrays:
    """Destinations of a call: pinned ones from ekf_host_alloc (freed on exit), ordinary ones from numpy; filled with a
    pattern no kernel writes."""

    def __init__(self, lib):
        self.lib, self.ptrs = lib, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.lib.ekf_host_free(p)

    def new(self, shape, pinned, dtype=np.float64):
        if pinned:
            count = int(np.prod(shape))
            p = self.lib.ekf_host_alloc(count * np.dtype(dtype).itemsize)
            assert p
            self.ptrs.append(p)
            ct = C.c_double if dtype == np.float64 else C.c_int
            a = np.ctypeslib.as_array((ct * count).from_address(p)).reshape(shape)
        else:
            a = np.empty(shape, dtype=dtype)
        a[...] = 12345
        return a


def ptr(a, t=DP):
    return a.ctypes.data_as(t)


def same_bits(a, b):
    """NaNs at the same positions, everything else bit for bit."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float64:
        return np.array_equal(a, b)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def all_same(got, want):
    return len(got) == len(want) and all(same_bits(g, w) for g, w in zip(got, want))


def raw_marginals(lib, f, pin_pose, pin_lm):
    cap = max(SIZES)
    with Arrays(lib) as A:
        pose, lms = A.new((B, 3, 3), pin_pose), A.new((B, cap, 2, 2), pin_lm)
        counts = np.empty(B, dtype=np.int32)
        assert lib.ekf_download_marginals(f._h, 0, B, ptr(pose), ptr(lms), cap, ptr(counts, IP)) == 0
        return pose.copy(), lms.copy(), counts


def raw_joint(lib, f, sels, pin_mean, pin_cov):
    stride = max(len(s) for s in sels)
    ns = 3 + 2 * stride
    lm = np.zeros((len(sels), stride), dtype=np.int32)
    for t, s in enumerate(sels):
        lm[t, :len(s)] = s
    kk = np.array([len(s) for s in sels], dtype=np.int32)
    with Arrays(lib) as A:
        mean, cov = A.new((len(sels), ns), pin_mean), A.new((len(sels), ns, ns), pin_cov)
        assert lib.ekf_download_joint(f._h, 0, len(sels), ptr(lm, IP), ptr(kk, IP), stride, ptr(mean), ptr(cov)) == 0
        return mean.copy(), cov.copy()


def raw_associate(lib, f, w, pin_cand, pin_full):
    """(the candidate outputs as one group, the full matrices as the other)"""
    S, cap = w["zr"].shape[1], max(SIZES)
    with Arrays(lib) as A:
        cand = A.new((B, S, 2), pin_cand, np.int32)
        nis, ld, mn = A.new((B, S, 2), pin_cand), A.new((B, S, 2), pin_cand), A.new((B, S), pin_cand)
        an, al = A.new((B, S, cap), pin_full), A.new((B, S, cap), pin_full)
        assert lib.ekf_associate(f._h, 0, B, ptr(w["zr"]), ptr(w["zb"]), ptr(w["m"], IP), S, ptr(cand, IP), ptr(nis), ptr(ld),
                                 ptr(mn), ptr(an), ptr(al), cap) == 0
        return cand.copy(), nis.copy(), ld.copy(), mn.copy(), an.copy(), al.copy()


def test_pinned_and_ordinary_destinations_agree_and_the_buffer_is_shared(sd, world):
    lib = sd.load_library()
    combos = list(itertools.product((True, False), repeat=2))
    f, fresh = make_filter(sd, world), make_filter(sd, world)
    try:
        before = [pbase(sd, f, b) for b in range(B)]
        passes = f.profile_passes()
        # ---- one staging buffer for the three, empty so far: a small need, the largest, a middle one, the small one again, all
        # staged; each against the same query on a fresh handle in the same state
        small = [[s[0]] for s in world["sels"]]
        for name, query in [("joint of 1", lambda h: raw_joint(lib, h, small, False, False)),
                            ("associate, full", lambda h: raw_associate(lib, h, world, False, False)),
                            ("marginals", lambda h: raw_marginals(lib, h, False, False)),
                            ("joint of 1 again", lambda h: raw_joint(lib, h, small, False, False))]:
            with make_filter(sd, world) as other:
                assert all_same(query(f), query(other)), name
        # ---- the binding's results, then every combination of pinned and ordinary destinations against them
        pose, lms, counts = f.marginals()
        assert list(counts) == list(SIZES)
        for b, N in enumerate(SIZES):                  # (the padding is part of every comparison below)
            assert np.isnan(lms[b, N:]).all() and not np.isnan(lms[b, :N]).any() and not np.isnan(pose[b]).any()
        jmean, jcov, _ = f.joint(world["sels"])
        for b, s in enumerate(world["sels"]):
            assert np.isnan(jcov[b, 3 + 2 * len(s):]).all() and not np.isnan(jcov[b, :3 + 2 * len(s), :3 + 2 * len(s)]).any()
        a = f.associate(world["zr"], world["zb"], world["m"], full=True)
        want_assoc = (a.cand, a.nis, a.logdet, a.min_nis, a.all_nis, a.all_logdet)
        assert np.isnan(a.all_nis[0, :, SIZES[0]:]).all() and not np.isnan(a.all_nis[0, :world["m"][0], :SIZES[0]]).any()
        assert (a.cand[2] == -1).all() and (a.cand[1, :3] >= 0).all()       # (m = 0: no candidates; m = 3: three rows of them)
        for pins in combos:
            assert all_same(raw_marginals(lib, f, *pins), (pose, lms, counts)), ("marginals", pins)
            assert all_same(raw_joint(lib, f, world["sels"], *pins), (jmean, jcov)), ("joint", pins)
            assert all_same(raw_associate(lib, f, world, *pins), want_assoc), ("associate", pins)
        # ---- nothing of the filter has moved ...
        assert f.profile_passes() == passes
        for b in range(B):
            assert np.array_equal(pbase(sd, f, b), before[b])
        # ---- ... and it goes on: the pending ranks flush to the oracle's state (and to what a handle never queried gives)
        f.flush()
        fresh.flush()
        assert f.profile_passes() == passes + 1        # (ranks were pending all along)
        for b, (om, oP) in enumerate(world["oracle"]):
            mu, P = f.state(b)
            assert orc.rel_fro(mu, om) < TIGHT and orc.rel_fro(P, oP) < TIGHT, (b, orc.rel_fro(mu, om), orc.rel_fro(P, oP))
            mu2, P2 = fresh.state(b)
            assert np.array_equal(mu, mu2) and np.array_equal(P, P2)
    finally:
        f.close()
        fresh.close()
