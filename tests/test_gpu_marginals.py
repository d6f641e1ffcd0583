"""GPU: marginal covariances without the covariance pass (ekf_download_marginals, EkfSlam.marginals).

Every case compares the query against the blocks a flushed download returns (PATH_TOL, relative Frobenius over the
stacked blocks) and, where a dense oracle is affordable, against the oracle (1e-9).  Where ranks are pending it also
checks that the query ran no pass (profile_passes) and left P_base as it was (ekf_debug_snapshot)."""
import ctypes as C

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests.conftest import path_ran
from tests.gpu_support import pbase, sd  # noqa: F401

pytestmark = pytest.mark.gpu

PATH_TOL = 1e-11
TIGHT = 1e-9
EKF_ERR_ARG = -1


def blocks_of(P, nl):
    """Pose block and the nl landmark blocks of a dense covariance."""
    lm = np.stack([P[3 + 2 * l:5 + 2 * l, 3 + 2 * l:5 + 2 * l] for l in range(nl)]) if nl else np.zeros((0, 2, 2))
    return P[:3, :3].copy(), lm


def stacked_err(got, want):
    g = np.concatenate([got[0].ravel(), got[1].ravel()])
    w = np.concatenate([want[0].ravel(), want[1].ravel()])
    return orc.rel_fro(g, w)


def query_untouched(sd, f, bs):
    """marginals() of the whole bank, asserting that it ran no pass and wrote nothing of P_base."""
    before = [pbase(sd, f, b, 1 << 24) for b in bs]
    passes = f.profile_passes()
    res = f.marginals()
    assert f.profile_passes() == passes
    for b, p in zip(bs, before):
        assert np.array_equal(pbase(sd, f, b, 1 << 24), p)
    return res


def flushed_blocks(f, b):
    """Reference: flush, then the pose block through covariance_block and the landmark blocks from the downloaded state."""
    f.flush()
    _, P = f.state(b)
    pose = f.covariance_block(0, 0, 3, 3, b)
    assert np.array_equal(pose, P[:3, :3])
    return blocks_of(P, (P.shape[0] - 3) // 2)


def check_bank(res, refs):
    pose, lms, counts = res
    for b, ref in refs.items():
        nl = len(ref[1])
        assert counts[b] == nl
        got = (pose[b], lms[b, :nl])
        assert stacked_err(got, ref) < PATH_TOL, (b, stacked_err(got, ref))
        assert np.isnan(lms[b, nl:]).all()


def test_per_step_kernels_with_ranks_pending(sd):
    """Per-step step() calls, N = 500 x 3, three steps of m = 8: against the oracle and the flushed download."""
    N, B, steps = 500, 3, 3
    n = 3 + 2 * N
    streams = [orc.synthetic_stream(N, steps, 8, 40 + t) for t in range(B)]
    cfg = orc.EkfConfig()
    oracle = []
    for s in streams:
        om, oP = s[0].copy(), np.diag(s[1])
        for k in range(steps):
            om, oP = orc.ekf_step_dense(om, oP, s[2][k], s[3][k], s[4][k], s[5][k], s[6][k], cfg)
        oracle.append(blocks_of(oP, N))
    with sd.EkfSlam(n, batch=B) as f:
        f.set_option("fused_cadence", 0)
        f.profile_enable(True)
        for b, s in enumerate(streams):
            f.set_state(s[0], np.diag(s[1]), b)
        for k in range(steps):
            f.step(np.array([s[2][k] for s in streams]), np.array([s[3][k] for s in streams]),
                   np.stack([s[4][k] for s in streams]), np.stack([s[5][k] for s in streams]),
                   np.stack([s[6][k] for s in streams]))
        res = query_untouched(sd, f, range(B))
        for b in range(B):
            assert stacked_err((res[0][b], res[1][b]), oracle[b]) < TIGHT
        one = f.marginals(1)
        assert np.array_equal(one[0], res[0][1]) and np.array_equal(one[1], res[1][1])
        passes = f.profile_passes()
        refs = {b: flushed_blocks(f, b) for b in range(B)}
        assert f.profile_passes() == passes + 1            # ranks were pending: the flush ran the pass
        check_bank(res, refs)


@pytest.mark.parametrize("N,chain", [(1250, 0), (2000, 1)])
def test_stream_pieces_ending_mid_cadence(sd, N, chain):
    """stream_run in pieces that end mid-cadence (look-ahead at N = 1250 x 1, chained at N = 2000 x 1), marginals() between
    the pieces: equal to the flushed blocks, and the run's final state bit-identical to the same pieces without queries,
    with the same cadence, chained and look-ahead counts."""
    lib = sd.load_library()
    n, steps, m = 3 + 2 * N, 22, 8
    s = orc.synthetic_stream(N, steps, m, 77)
    rng = np.random.default_rng(5)
    A = rng.normal(size=(n, 6)) * 0.3
    P0 = A @ A.T
    P0[np.arange(n), np.arange(n)] += rng.uniform(0.5, 2.0, n)
    args = tuple(np.asarray(a)[:, None] for a in (s[2], s[3], s[4], s[5], s[6]))
    pieces = [(0, 7), (7, 6), (13, 9)]                      # 56, 104 updates: both boundaries inside a cadence of 40

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
                    got.append(query_untouched(sd, f, [0]))
                elif mode == "flush":
                    got.append(flushed_blocks(f, 0))
            return got, f.state(0), f.cadence_counters(), lib.ekf_debug_chained(f._h), lib.ekf_debug_lookaheads(f._h)

    q, ref, plain = run("query"), run("flush"), run("none")
    for (pose, lms, counts), blocks in zip(q[0], ref[0]):
        assert counts[0] == N
        assert stacked_err((pose[0], lms[0]), blocks) < PATH_TOL
    assert np.array_equal(q[1][0], plain[1][0]) and np.array_equal(q[1][1], plain[1][1])
    assert q[2:] == plain[2:]
    assert q[4] > 0                                        # the look-ahead ran ...
    assert (q[3] > 0) == bool(chain)                       # ... chained where asked


def test_column_panels(sd):
    """N = 2100 (n = 4203 > 4096: P_base in column panels; landmark 2046 straddles the panel boundary)."""
    N, steps = 2100, 6
    n = 3 + 2 * N
    s = orc.synthetic_stream(N, steps, 8, 91)
    idx = s[4].copy()
    idx[:, :4] = (2040 + np.arange(4))[None, :] + 4 * np.arange(steps)[:, None] % 12   # landmarks around the boundary
    idx[:, 4:] = (idx[:, :4] + 30) % N
    with sd.EkfSlam(n, batch=1) as f:
        f.set_option("fused_cadence", 0)
        f.profile_enable(True)
        f.set_state_diag(s[0], s[1])
        for k in range(steps):
            f.step(s[2][k], s[3][k], idx[k], s[5][k], s[6][k])
        res = query_untouched(sd, f, [0])
        passes = f.profile_passes()
        check_bank(res, {0: flushed_blocks(f, 0)})
        assert f.profile_passes() == passes + 1            # ranks were pending


def test_active_bound_block_diagonal_start(sd):
    """N = 8000 x 1 from a block-diagonal start with the active bound on, landmarks first observed inside the pending window;
    landmarks beyond the bound return exactly 1e4 I."""
    N, steps, m = 8000, 7, 8
    n = 3 + 2 * N
    s = orc.synthetic_stream(N, steps, m, 13)
    diag = np.full(n, 1e4)
    diag[:3] = s[1][:3]
    idx = (np.arange(steps * m, dtype=np.int32) * 3).reshape(steps, m)   # every update a landmark never seen before
    args = tuple(np.asarray(a)[:, None] for a in (s[2], s[3], idx, s[5], s[6]))
    L = int(idx.max()) + 1
    with sd.EkfSlam(n, batch=1) as f:
        f.profile_enable(True)
        f.set_state_diag(s[0], diag)
        f.run_stream(*args)                                # 56 updates: the last 16 (new landmarks) stay pending
        pose, lms, counts = query_untouched(sd, f, [0])
        assert counts[0] == N
        assert (lms[0, L:] == np.array([[1e4, 0.0], [0.0, 1e4]])).all()
        unseen = np.setdiff1d(np.arange(L), idx.ravel())
        assert (lms[0, unseen] == np.array([[1e4, 0.0], [0.0, 1e4]])).all()
        passes = f.profile_passes()
        f.flush()
        assert f.profile_passes() == passes + 1
        lead = f.covariance_block(0, 0, 3 + 2 * L, 3 + 2 * L)
        ref = blocks_of(lead, L)
        assert stacked_err((pose[0], lms[0, :L]), ref) < PATH_TOL
        assert np.array_equal(f.covariance_block(3 + 2 * (N - 1), 3 + 2 * (N - 1), 2, 2), lms[0, N - 1])


def test_trajectories_of_different_sizes(sd):
    """A bank whose states differ in size (uploads of different n, add_landmarks): NaN padding and counts, against the
    oracle and the flushed blocks."""
    nmax = 3 + 2 * 300
    sizes = [3 + 2 * 300, 3 + 2 * 90, 3 + 2 * 201]
    B, steps = 3, 4
    streams = [orc.synthetic_stream(300, steps, 8, 500 + t) for t in range(B)]
    cfg = orc.EkfConfig()
    idx = [np.asarray(st[4]) % ((sizes[b] - 3) // 2) for b, st in enumerate(streams)]
    ostate = [(st[0][:sizes[b]].copy(), np.diag(st[1][:sizes[b]])) for b, st in enumerate(streams)]
    with sd.EkfSlam(nmax, batch=B) as f:
        f.profile_enable(True)
        f.set_option("fused_cadence", 0)
        for b in range(B):
            f.set_state_diag(ostate[b][0], np.diag(ostate[b][1]), b)
        xy = np.array([[1.0, 2.0], [-0.5, 0.25], [3.0, 1.0]])
        f.add_landmarks(xy, 1)                             # trajectory 1: 90 -> 93 landmarks
        mu1 = np.concatenate([ostate[1][0], xy.ravel()])
        P1 = np.zeros((len(mu1), len(mu1)))
        P1[:len(ostate[1][0]), :len(ostate[1][0])] = ostate[1][1]
        P1[len(ostate[1][0]):, len(ostate[1][0]):] = np.eye(6) * orc.EkfConfig().landmark_init_var
        ostate[1] = (mu1, P1)
        for k in range(steps):
            f.step(np.array([st[2][k] for st in streams]), np.array([st[3][k] for st in streams]),
                   [idx[b][k] for b in range(B)], [streams[b][5][k] for b in range(B)], [streams[b][6][k] for b in range(B)])
            for b in range(B):
                ostate[b] = orc.ekf_step_dense(*ostate[b], streams[b][2][k], streams[b][3][k], idx[b][k], streams[b][5][k],
                                               streams[b][6][k], cfg)
        pose, lms, counts = query_untouched(sd, f, range(B))
        assert list(counts) == [300, 93, 201] and lms.shape == (B, 300, 2, 2)
        for b in range(B):
            nl = counts[b]
            assert np.isnan(lms[b, nl:]).all() and not np.isnan(lms[b, :nl]).any()
            assert stacked_err((pose[b], lms[b, :nl]), blocks_of(ostate[b][1], nl)) < TIGHT
        one = f.marginals(1)
        assert one[1].shape == (93, 2, 2) and np.array_equal(one[1], lms[1, :93])
        check_bank((pose, lms, counts), {b: flushed_blocks(f, b) for b in range(B)})


def test_small_state_path_bit_identical(sd, both_paths):
    """N = 20: on the small-state path nothing is ever pending, so the query is the downloaded blocks bit for bit; on the
    general kernels at the same size it equals them to PATH_TOL.  Both against the oracle."""
    N, steps, B = 20, 12, 4
    streams = [orc.synthetic_stream(N, steps, 8, 700 + t) for t in range(B)]
    cfg = orc.EkfConfig()
    with sd.EkfSlam(3 + 2 * N, batch=B) as f:
        for b, st in enumerate(streams):
            f.set_state_diag(st[0], st[1], b)
        f.run_stream(np.stack([st[2] for st in streams], 1), np.stack([st[3] for st in streams], 1),
                     np.stack([st[4] for st in streams], 1), np.stack([st[5] for st in streams], 1),
                     np.stack([st[6] for st in streams], 1))
        pose, lms, counts = f.marginals()
        assert path_ran(f, both_paths)
        for b, st in enumerate(streams):
            om, oP = st[0].copy(), np.diag(st[1])
            for k in range(steps):
                om, oP = orc.ekf_step_dense(om, oP, st[2][k], st[3][k], st[4][k], st[5][k], st[6][k], cfg)
            assert stacked_err((pose[b], lms[b]), blocks_of(oP, N)) < TIGHT
        for b in range(B):
            blk = f.covariance_block(0, 0, 3, 3, b)
            ref = blocks_of(f.covariance(b), N)
            if both_paths == "default_path":
                assert np.array_equal(pose[b], blk) and np.array_equal(lms[b], ref[1])
            else:
                assert stacked_err((pose[b], lms[b]), (blk, ref[1])) < PATH_TOL


def test_nothing_pending_is_the_upload(sd):
    """Right after set_state nothing is pending: the query returns the uploaded blocks bit for bit."""
    N, B = 300, 2
    n = 3 + 2 * N
    rng = np.random.default_rng(1)
    with sd.EkfSlam(n, batch=B) as f:
        Ps = []
        for b in range(B):
            A = rng.normal(size=(n, 5))
            P = A @ A.T + np.diag(rng.uniform(0.5, 2.0, n))
            Ps.append(P)
            f.set_state(rng.normal(size=n), P, b)
        pose, lms, counts = f.marginals()
        for b in range(B):
            ref = blocks_of(np.triu(Ps[b]) + np.triu(Ps[b], 1).T, N)
            assert np.array_equal(pose[b], ref[0]) and np.array_equal(lms[b], ref[1])


def test_config4_shape(sd):
    """The benchmark's config-4 shape, 32 x N = 2000, after 3 steps with ranks pending."""
    N, B, steps = 2000, 32, 3
    n = 3 + 2 * N
    streams = [orc.synthetic_stream(N, steps, 8, 900 + t) for t in range(B)]
    with sd.EkfSlam(n, batch=B) as f:
        f.profile_enable(True)
        for b, st in enumerate(streams):
            f.set_state_diag(st[0], st[1], b)
        for k in range(steps):
            f.step(np.array([st[2][k] for st in streams]), np.array([st[3][k] for st in streams]),
                   np.stack([st[4][k] for st in streams]), np.stack([st[5][k] for st in streams]),
                   np.stack([st[6][k] for st in streams]))
        pose, lms, counts = query_untouched(sd, f, [0, 31])
        assert list(counts) == [N] * B
        passes = f.profile_passes()
        f.flush()
        assert f.profile_passes() == passes + 1
        for b in range(B):
            assert orc.rel_fro(pose[b], f.covariance_block(0, 0, 3, 3, b)) < PATH_TOL
        check_bank((pose, lms, counts), {b: flushed_blocks(f, b) for b in (0, 17, 31)})


def test_bad_arguments(sd):
    lib = sd.load_library()
    dp = C.POINTER(C.c_double)
    with sd.EkfSlam(3 + 2 * 100, batch=2) as f:
        mean = np.zeros(3 + 2 * 100)
        for b in range(2):
            f.set_state_diag(mean, np.ones(3 + 2 * 100), b)
        pose = np.empty((2, 9))
        lms = np.empty((2, 100, 4))
        cnt = np.empty(2, dtype=np.int32)
        pp, lp, cp = pose.ctypes.data_as(dp), lms.ctypes.data_as(dp), cnt.ctypes.data_as(C.POINTER(C.c_int))
        call = lib.ekf_download_marginals
        assert call(f._h, -1, 1, pp, lp, 100, cp) == EKF_ERR_ARG
        assert call(f._h, 0, 0, pp, lp, 100, cp) == EKF_ERR_ARG
        assert call(f._h, 1, 2, pp, lp, 100, cp) == EKF_ERR_ARG
        assert call(f._h, 0, 1, None, lp, 100, cp) == EKF_ERR_ARG
        assert call(f._h, 0, 2, pp, lp, 99, cp) == EKF_ERR_ARG
        assert call(f._h, 0, 2, pp, lp, 100, cp) == 0 and list(cnt) == [100, 100]
        assert call(f._h, 1, 1, pp, None, 0, None) == 0
        assert np.array_equal(pose[0].reshape(3, 3), np.eye(3))
