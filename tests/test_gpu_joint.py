"""GPU: the joint covariance of a landmark subset without the covariance pass (ekf_download_joint, EkfSlam.joint), joint
compatibility on top of it (step_unlabelled(joint=True)) and evaluation.landmark_separation.

Tolerances are those of test_gpu_marginals.py: PATH_TOL = 1e-11 relative Frobenius against state(b)[1][np.ix_(s, s)] taken
AFTER a flush (the pending ranks are summed in another order), 1e-9 against the dense oracle, bit-identical where nothing is
pending.  Where ranks are pending every query also checks that it ran no pass (profile_passes), left P_base as it was
(ekf_debug_snapshot) and returned an exactly symmetric matrix."""
import ctypes as C

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests import assoc_world as aw
from tests import joint_world as jw
from tests.conftest import path_ran
from tests.gpu_support import pbase, sd  # noqa: F401

pytestmark = pytest.mark.gpu

PATH_TOL = 1e-11
TIGHT = 1e-9
EKF_ERR_ARG = -1
EKF_JMAX = 64


def sub_idx(sel):
    return [0, 1, 2] + [3 + 2 * int(j) + d for j in sel for d in range(2)]


def query_untouched(sd, f, sels, bs):
    """joint() of the whole bank, asserting that it ran no pass, wrote nothing of P_base and is exactly symmetric."""
    before = [pbase(sd, f, b) for b in bs]
    passes = f.profile_passes()
    mean, cov, k = f.joint(sels)
    assert f.profile_passes() == passes
    for b, p in zip(bs, before):
        assert np.array_equal(pbase(sd, f, b), p)
    for b in range(len(sels)):
        n = 3 + 2 * len(sels[b])
        assert k[b] == len(sels[b])
        assert np.array_equal(cov[b, :n, :n], cov[b, :n, :n].T) and not np.isnan(cov[b, :n, :n]).any()
        assert np.isnan(cov[b, n:, :]).all() and np.isnan(cov[b, :, n:]).all() and np.isnan(mean[b, n:]).all()
    return mean, cov, k


def three_steps(sd, N=150, B=3, steps=3):
    streams = [orc.synthetic_stream(N, steps, 8, 40 + t) for t in range(B)]
    f = sd.EkfSlam(3 + 2 * N, batch=B)
    f.set_option("fused_cadence", 0)
    f.profile_enable(True)
    for b, s in enumerate(streams):
        f.set_state(s[0], np.diag(s[1]), b)
    for k in range(steps):
        f.step(np.array([s[2][k] for s in streams]), np.array([s[3][k] for s in streams]),
               np.stack([s[4][k] for s in streams]), np.stack([s[5][k] for s in streams]),
               np.stack([s[6][k] for s in streams]))
    return f, streams


@pytest.fixture(scope="module")
def oracle_three_steps():
    """The dense oracle's covariances of `three_steps`, computed once."""
    N, B, steps = 150, 3, 3
    cfg = orc.EkfConfig()
    out = []
    for t in range(B):
        s = orc.synthetic_stream(N, steps, 8, 40 + t)
        om, oP = s[0].copy(), np.diag(s[1])
        for k in range(steps):
            om, oP = orc.ekf_step_dense(om, oP, s[2][k], s[3][k], s[4][k], s[5][k], s[6][k], cfg)
        out.append((om, oP))
    return out


def test_per_step_kernels_with_ranks_pending(sd, oracle_three_steps):
    """N = 150 x 3, three step()s of m = 8, unsorted selections of k = 0, 20 and 64 landmarks (stride padding, more than one
    tile, the maximum; observed landmarks among them): against the oracle and the flushed state."""
    N = 150
    f, streams = three_steps(sd)
    with f:
        rng = np.random.default_rng(2)
        seen = [np.unique(np.asarray(s[4]).ravel()) for s in streams]
        sels = [[],
                [int(j) for j in rng.permutation(np.concatenate([seen[1][:8], np.setdiff1d(np.arange(N), seen[1])[:12]]))],
                [int(j) for j in rng.permutation(np.concatenate([seen[2][:12], np.setdiff1d(np.arange(N), seen[2])[:52]]))]]
        assert [len(s) for s in sels] == [0, 20, 64] and sels[1] != sorted(sels[1]) and sels[2] != sorted(sels[2])
        mean, cov, k = query_untouched(sd, f, sels, range(3))
        assert cov.shape == (3, 131, 131) and mean.shape == (3, 131)
        for b in range(3):
            s = sub_idx(sels[b])
            assert orc.rel_fro(cov[b, :len(s), :len(s)], oracle_three_steps[b][1][np.ix_(s, s)]) < TIGHT
            assert np.array_equal(mean[b, :len(s)], f.mean(b)[s])
        one = f.joint(sels[1], 1)
        assert one[0].shape == (43,) and np.array_equal(one[1], cov[1, :43, :43]) and np.array_equal(one[0], mean[1, :43])
        passes = f.profile_passes()
        f.flush()
        for b in range(3):
            s = sub_idx(sels[b])
            err = orc.rel_fro(cov[b, :len(s), :len(s)], f.state(b)[1][np.ix_(s, s)])
            assert err < PATH_TOL, (b, err)
        assert f.profile_passes() == passes + 1            # ranks were pending: the flush ran the pass
        with pytest.raises(ValueError):
            f.joint(list(range(EKF_JMAX + 1)), 0)


def test_permutation_and_subset_are_bit_identical(sd):
    """Same state, nothing flushed in between: a permuted selection gives the permuted result, a 5-landmark subset of a
    40-landmark query the same entries, bit for bit; the diagonal blocks agree with marginals()."""
    N = 150
    f, streams = three_steps(sd)
    with f:
        rng = np.random.default_rng(7)
        seen = np.unique(np.asarray(streams[1][4]).ravel())
        sel = [int(j) for j in rng.permutation(np.concatenate([seen[:15], np.setdiff1d(np.arange(N), seen)[:25]]))]
        perm = rng.permutation(40)
        m0, c0 = f.joint(sel, 1)
        m1, c1 = f.joint([sel[p] for p in perm], 1)
        at = np.array([0, 1, 2] + [3 + 2 * int(p) + d for p in perm for d in range(2)])
        assert np.array_equal(c1, c0[np.ix_(at, at)]) and np.array_equal(m1, m0[at])
        pick = [3, 31, 0, 17, 39]
        m2, c2 = f.joint([sel[p] for p in pick], 1)
        at = np.array([0, 1, 2] + [3 + 2 * p + d for p in pick for d in range(2)])
        assert np.array_equal(c2, c0[np.ix_(at, at)]) and np.array_equal(m2, m0[at])
        # a bank query with other trajectories beside it returns the same bits too
        _, cb, _ = f.joint([[1, 2, 3], sel, []])
        assert np.array_equal(cb[1, :83, :83], c0)
        pose, lms = f.marginals(1)
        got = np.concatenate([c0[:3, :3].ravel()] + [c0[3 + 2 * p:5 + 2 * p, 3 + 2 * p:5 + 2 * p].ravel() for p in range(40)])
        want = np.concatenate([pose.ravel()] + [lms[j].ravel() for j in sel])
        assert orc.rel_fro(got, want) < PATH_TOL


@pytest.mark.parametrize("N,chain", [(1250, 0), (2000, 1)])
def test_stream_pieces_ending_mid_cadence(sd, N, chain):
    """stream_run in pieces that end mid-cadence (look-ahead at N = 1250 x 1, chained at N = 2000 x 1), joint() of 32
    scattered landmarks between the pieces: equal to the flushed run, and the run's final state bit-identical to the same
    pieces without queries, with the same cadence, chained and look-ahead counts."""
    lib = sd.load_library()
    n, steps, m = 3 + 2 * N, 22, 8
    s = orc.synthetic_stream(N, steps, m, 77)
    rng = np.random.default_rng(5)
    A = rng.normal(size=(n, 6)) * 0.3
    P0 = A @ A.T
    P0[np.arange(n), np.arange(n)] += rng.uniform(0.5, 2.0, n)
    args = tuple(np.asarray(a)[:, None] for a in (s[2], s[3], s[4], s[5], s[6]))
    pieces = [(0, 7), (7, 6), (13, 9)]                      # 56, 104 updates: both boundaries inside a cadence of 40
    seen = np.unique(np.asarray(s[4]).ravel())
    sel = [int(j) for j in np.random.default_rng(8).permutation(
        np.concatenate([seen[::max(1, len(seen) // 16)][:16], np.setdiff1d(np.arange(N), seen)[::N // 20][:16]]))]
    assert len(sel) == 32
    ix = sub_idx(sel)

    def run(mode):
        with sd.EkfSlam(n, batch=1) as f:
            f.set_option("chain", chain)
            f.profile_enable(True)
            f.set_state(s[0], P0)
            f.stream_upload(*args)
            got = []
            for first, count in pieces:
                f.stream_run(first, count)
                if mode == "query":
                    got.append(query_untouched(sd, f, [sel], [0])[1][0])
                elif mode == "flush":
                    f.flush()
                    got.append(f.state(0)[1][np.ix_(ix, ix)])
            return got, f.state(0), f.cadence_counters(), lib.ekf_debug_chained(f._h), lib.ekf_debug_lookaheads(f._h)

    q, ref, plain = run("query"), run("flush"), run("none")
    for got, want in zip(q[0], ref[0]):
        assert orc.rel_fro(got, want) < PATH_TOL
    assert np.array_equal(q[1][0], plain[1][0]) and np.array_equal(q[1][1], plain[1][1])
    assert q[2:] == plain[2:]
    assert q[4] > 0                                        # the look-ahead ran ...
    assert (q[3] > 0) == bool(chain)                       # ... chained exactly where asked


def test_active_bound_block_diagonal_start(sd):
    """N = 600 x 1 from a block-diagonal start, a stream that observes only the first 100 landmarks: a selection on both
    sides of the active bound; beyond it the result is the uploaded diagonal bit for bit."""
    N, steps, m = 600, 4, 8
    n = 3 + 2 * N
    s = orc.synthetic_stream(N, steps, m, 13)
    diag = np.random.default_rng(3).uniform(0.5, 2.0, n)
    idx = np.asarray(s[4]) % 100
    for k in range(steps):                                 # (a step names a landmark once)
        idx[k] = (idx[k, 0] + 11 * np.arange(m)) % 100
    sel = [int(j) for j in np.concatenate([np.unique(idx)[:10], [99, 98, 100, 101, 599, 350, 123]])]
    sel = [j for t, j in enumerate(sel) if j not in sel[:t]]
    sel = sel[::2] + sel[1::2]
    above = [t for t, j in enumerate(sel) if j >= 100]
    assert len(above) >= 5 and len(sel) - len(above) >= 8
    with sd.EkfSlam(n, batch=1) as f:
        f.set_option("fused_cadence", 0)
        f.profile_enable(True)
        f.set_state_diag(s[0], diag)
        for k in range(steps - 1):
            f.step(s[2][k], s[3][k], idx[k], s[5][k], s[6][k])
        cov = query_untouched(sd, f, [sel], [0])[1][0]
        at = np.array([3 + 2 * t + d for t in above for d in range(2)])
        st = np.array([3 + 2 * sel[t] + d for t in above for d in range(2)])
        assert np.array_equal(cov[np.ix_(at, at)], np.diag(diag[st]))
        passes = f.profile_passes()
        f.flush()
        ix = sub_idx(sel)
        assert orc.rel_fro(cov, f.state(0)[1][np.ix_(ix, ix)]) < PATH_TOL
        assert f.profile_passes() == passes + 1            # ranks were pending


def test_column_panels(sd):
    """N = 2100 (n = 4203 > 4096: P_base in column panels), landmarks on both sides of state index 4096 -- landmark 2046
    straddles it --, two steps pending."""
    N, steps = 2100, 2
    n = 3 + 2 * N
    s = orc.synthetic_stream(N, steps, 8, 91)
    idx = np.asarray(s[4]).copy()
    idx[:, :4] = (2040 + np.arange(4))[None, :] + 4 * np.arange(steps)[:, None]   # 2040 .. 2047: around the boundary
    idx[:, 4:] = (idx[:, :4] + 30) % N
    sel = [2047, 5, 2046, 2099, 2040, 1000, 2071, 2045, 2050, 17, 2044]
    rng = np.random.default_rng(4)
    A = rng.normal(size=(n, 4)) * 0.3
    P0 = A @ A.T
    P0[np.arange(n), np.arange(n)] += rng.uniform(0.5, 2.0, n)
    with sd.EkfSlam(n, batch=1) as f:
        f.set_option("fused_cadence", 0)
        f.profile_enable(True)
        f.set_state(s[0], P0)
        for k in range(steps):
            f.step(s[2][k], s[3][k], idx[k], s[5][k], s[6][k])
        cov = query_untouched(sd, f, [sel], [0])[1][0]
        passes = f.profile_passes()
        f.flush()
        ix = sub_idx(sel)
        assert orc.rel_fro(cov, f.state(0)[1][np.ix_(ix, ix)]) < PATH_TOL
        assert f.profile_passes() == passes + 1            # ranks were pending


@pytest.mark.parametrize("N", [12, 20])
def test_small_state_path_and_general_kernels(sd, both_paths, N):
    """After a short stream, joint() of all landmarks in reversed order is state()'s matrix permuted: bit for bit on the
    small-state path, where nothing is ever pending, within PATH_TOL on the general kernels."""
    steps = 6
    st = orc.synthetic_stream(N, steps, 8, 700 + N)
    with sd.EkfSlam(3 + 2 * N, batch=1) as f:
        f.set_state_diag(st[0], st[1])
        f.run_stream(*(np.asarray(a)[:, None] for a in (st[2], st[3], st[4], st[5], st[6])))
        sel = list(range(N))[::-1]
        mean, cov = f.joint(sel, 0)
        assert path_ran(f, both_paths)
        ix = sub_idx(sel)
        assert np.array_equal(cov, cov.T)
        mu, P = f.state(0)
        assert np.array_equal(mean, mu[ix])
        if both_paths == "default_path":
            assert np.array_equal(cov, P[np.ix_(ix, ix)])
        else:
            assert orc.rel_fro(cov, P[np.ix_(ix, ix)]) < PATH_TOL


def test_nothing_pending_is_the_upload(sd):
    """Right after set_state nothing is pending: the query returns the uploaded upper triangle, mirrored, bit for bit."""
    N = 100
    n = 3 + 2 * N
    rng = np.random.default_rng(1)
    A = rng.normal(size=(n, n))
    P = A @ A.T + n * np.eye(n)                            # (not symmetric to the last bit: the upper triangle counts)
    mu = rng.normal(size=n)
    with sd.EkfSlam(n, batch=1) as f:
        f.set_state(mu, P)
        sel = [int(j) for j in rng.permutation(N)[:64]]
        mean, cov = f.joint(sel, 0)
        ix = sub_idx(sel)
        up = np.triu(P) + np.triu(P, 1).T
        assert np.array_equal(cov, up[np.ix_(ix, ix)]) and np.array_equal(mean, mu[ix])


def test_bad_arguments_leave_the_handle_usable(sd):
    lib = sd.load_library()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    f, _ = three_steps(sd, N=100, B=2)
    with f:
        stride = 4
        ns = 3 + 2 * stride
        good = np.array([[5, 1, 99, 3], [7, 0, 0, 0]], dtype=np.int32)
        kk = np.array([4, 1], dtype=np.int32)
        mean, cov = np.empty((2, ns)), np.empty((2, ns, ns))
        call = lib.ekf_download_joint

        def go(b0, count, lm, k, st, m=mean, c=cov):
            return call(f._h, b0, count, None if lm is None else lm.ctypes.data_as(ip), None if k is None else k.ctypes.data_as(ip),
                        st, None if m is None else m.ctypes.data_as(dp), None if c is None else c.ctypes.data_as(dp))

        before = [pbase(sd, f, b) for b in range(2)]
        passes = f.profile_passes()
        assert go(0, 2, good, kk, stride) == 0
        ref_mean, ref_cov = mean.copy(), cov.copy()
        mean[:], cov[:] = 7.0, 7.0
        assert go(-1, 1, good, kk, stride) == EKF_ERR_ARG
        assert go(0, 0, good, kk, stride) == EKF_ERR_ARG
        assert go(1, 2, good, kk, stride) == EKF_ERR_ARG
        assert go(0, 2, good, kk, 0) == EKF_ERR_ARG
        big = np.zeros((2, EKF_JMAX + 1), dtype=np.int32)
        assert go(0, 2, big, np.zeros(2, dtype=np.int32), EKF_JMAX + 1) == EKF_ERR_ARG
        assert go(0, 2, good, np.array([5, 1], dtype=np.int32), stride) == EKF_ERR_ARG
        assert go(0, 2, good, np.array([4, -1], dtype=np.int32), stride) == EKF_ERR_ARG
        assert go(0, 2, np.array([[5, 1, 100, 3], [7, 0, 0, 0]], dtype=np.int32), kk, stride) == EKF_ERR_ARG
        assert go(0, 2, np.array([[5, 1, -1, 3], [7, 0, 0, 0]], dtype=np.int32), kk, stride) == EKF_ERR_ARG
        assert go(0, 2, np.array([[5, 1, 5, 3], [7, 0, 0, 0]], dtype=np.int32), kk, stride) == EKF_ERR_ARG
        assert go(0, 2, None, kk, stride) == EKF_ERR_ARG
        assert go(0, 2, good, None, stride) == EKF_ERR_ARG
        assert go(0, 2, good, kk, stride, c=None) == EKF_ERR_ARG
        assert (mean == 7.0).all() and (cov == 7.0).all()   # no destination was touched
        assert f.profile_passes() == passes
        for b in range(2):
            assert np.array_equal(pbase(sd, f, b), before[b])
        # still usable: the same bits again (plain NumPy destinations), without the mean, and into pinned memory
        assert go(0, 2, good, kk, stride) == 0
        assert np.array_equal(cov, ref_cov, equal_nan=True) and np.array_equal(mean, ref_mean, equal_nan=True)
        cov[:] = 7.0
        assert go(0, 2, good, kk, stride, m=None) == 0 and np.array_equal(cov, ref_cov, equal_nan=True)
        pm, pc, pk = f.joint([[5, 1, 99, 3], [7]])
        assert np.array_equal(pc, ref_cov, equal_nan=True) and np.array_equal(pm, ref_mean, equal_nan=True)
        assert list(pk) == [4, 1]
        assert go(1, 1, good[1:], kk[1:], stride) == 0 and np.array_equal(cov[0], ref_cov[1], equal_nan=True)


def test_step_unlabelled_joint_recovers_the_labels_bit_identical_to_the_labelled_run(sd):
    """The 4 x 4 grid world, seed 0: step_unlabelled(joint=True) returns the truth at every step and leaves the state of the
    labelled predict / add_landmarks / update run, bit for bit."""
    name = "4x4"
    run = aw.make_run(name, 0)[1]
    N = aw.WORLDS[name][0] ** 2
    cfg = sd.EkfConfig(motion_sigma=0.02, meas_sigma=0.03)
    n_max = 3 + 2 * N
    with sd.EkfSlam(n_max, batch=1, config=cfg) as f, sd.EkfSlam(n_max, batch=1, config=cfg) as g:
        for k, (lin, ang, vis, zr, zb) in enumerate(run):
            before = (g.size(0) - 3) // 2
            assign = f.step_unlabelled(lin, ang, zr[None, :], zb[None, :], joint=True)
            assert list(assign[0]) == list(vis), k
            g.predict(lin, ang)
            new = [q for q, w in enumerate(vis) if w >= before]
            if new:
                assert [vis[q] for q in new] == list(range(before, before + len(new)))
                x0, y0, th = g.mean(0)[:3]
                g.add_landmarks(np.array([(x0 + zr[q] * np.cos(zb[q] + th), y0 + zr[q] * np.sin(zb[q] + th)) for q in new]), 0)
            g.update([vis], [zr], [zb])
        (mf, Pf), (mg, Pg) = f.state(0), g.state(0)
        assert len(mf) == 3 + 2 * N and np.array_equal(mf, mg) and np.array_equal(Pf, Pg)


@pytest.mark.parametrize("seed", jw.SEEDS)
def test_step_unlabelled_joint_on_the_case_individual_compatibility_gets_wrong(sd, seed):
    """The scenario of tests/test_joint_cpu.py, uploaded as one state: joint=True gives no wrong label and at least m - 1
    right ones, joint=False reproduces the CPU reference's wrong ones."""
    import slam_duckietown_amd.frontend as fe
    sc = jw.make_scenario(seed)
    truth = sc["truth"]
    m = len(truth)
    nis, logdet, _, _ = aw.ref_scores(sc["mean"], sc["P"], sc["zr"], sc["zb"], jw.cfg_loose().meas_noise_diag())
    cand, cnis, mn, _ = aw.ref_candidates(nis, logdet)
    greedy, _, _ = fe.resolve_associations(cand, cnis, mn, aw.ACCEPT, aw.CREATE)
    assert int(((greedy >= 0) & (greedy != truth)).sum()) >= 1
    cfg = sd.EkfConfig(motion_sigma=jw.LOOSE, meas_sigma=jw.MEAS)
    got = {}
    for joint in (True, False):
        with sd.EkfSlam(3 + 4 * m, batch=1, config=cfg) as f:
            f.set_state(sc["mean0"], sc["P0"])
            got[joint] = np.asarray(f.step_unlabelled(sc["lin"], sc["ang"], sc["zr"][None, :], sc["zb"][None, :], joint=joint)[0])
    old = got[True] < m                                    # (labels from m on are landmarks the step created)
    assert int((old & (got[True] >= 0) & (got[True] != truth)).sum()) == 0
    assert int((got[True] == truth).sum()) >= m - 1
    matched = greedy >= 0
    assert np.array_equal(got[False][matched], greedy[matched])
    assert ((got[False][~matched] < 0) | (got[False][~matched] >= m)).all()


def test_landmark_separation_with_ranks_pending(sd):
    """N = 150 with ranks pending: the closed form from the flushed dense matrix, relative 1e-9; read-only."""
    import slam_duckietown_amd.evaluation as ev
    f, streams = three_steps(sd)
    with f:
        seen = np.unique(np.asarray(streams[0][4]).ravel())
        pairs = [(int(seen[0]), int(seen[1])), (int(seen[2]), 149), (3, int(seen[3])), (148, 147)] + \
                [(int(i), int((i + 37) % 150)) for i in range(0, 150, 4)]
        pairs = [p for p in pairs if p[0] != p[1]]
        assert len(pairs) > EKF_JMAX // 2                  # more than one joint() call
        before = pbase(sd, f, 0)
        passes = f.profile_passes()
        dist, sigma, maha = ev.landmark_separation(f, pairs, b=0)
        assert f.profile_passes() == passes and np.array_equal(pbase(sd, f, 0), before)
        f.flush()
        mu, P = f.state(0)
        for t, (i, j) in enumerate(pairs):
            a, c = 3 + 2 * i, 3 + 2 * j
            d = mu[a:a + 2] - mu[c:c + 2]
            Pd = P[a:a + 2, a:a + 2] + P[c:c + 2, c:c + 2] - P[a:a + 2, c:c + 2] - P[c:c + 2, a:a + 2]
            r = np.hypot(*d)
            assert dist[t] == pytest.approx(r, rel=TIGHT)
            assert sigma[t] == pytest.approx(np.sqrt(d @ Pd @ d) / r, rel=TIGHT)
            assert maha[t] == pytest.approx(d @ np.linalg.solve(Pd, d), rel=TIGHT)
