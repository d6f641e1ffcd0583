"""GPU: the innovation log (ekf_log_innovations / ekf_download_innovations, EkfSlam.log_innovations / innovations).

Every landmark update's (index, y, S, NIS) against a restatement of the oracle's sequential update that also returns y and
S (y to 1e-9 absolute, S and NIS to 1e-9 relative), where a dense oracle is affordable; beyond, against the log of the same
stream on the per-step kernels (1e-10).  Switching the log on must change nothing: same bits of mean and covariance, same
flags and scheduling counters as the same calls with the log off."""
import ctypes as C

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests.conftest import path_ran
from tests.gated_oracle import AMAX, block_err, step_log, update_log
from tests.gpu_support import final, same_bits, scheduling, sd, tag  # noqa: F401
from tests.streams import dense_start, steps_of, wandering

pytestmark = pytest.mark.gpu

EKF_ERR_ARG = -1


def check_entries(innov, k, b, idx, ys, Ss):
    """Row k, trajectory b of an Innovations log against the oracle's updates (in application order)."""
    m = len(idx)
    assert innov.m[k, b] == m
    kept = min(m, AMAX)
    assert list(innov.idx[k, b, :kept]) == [int(i) for i in idx[:kept]]
    np.testing.assert_allclose(innov.y[k, b, :kept], ys[:kept], rtol=0, atol=1e-9)
    assert block_err(innov.S[k, b, :kept], Ss[:kept]) < 1e-9
    nis = np.einsum("ji,ji->j", ys[:kept], np.linalg.solve(Ss[:kept], ys[:kept, :, None])[..., 0])
    np.testing.assert_allclose(innov.nis[k, b, :kept], nis, rtol=1e-9, atol=0)
    W = innov.idx.shape[2]
    assert (innov.idx[k, b, kept:] == -1).all()
    assert np.isnan(innov.y[k, b, kept:W]).all() and np.isnan(innov.nis[k, b, kept:W]).all()


def stream_oracle(means, starts, lin, ang, idx, zr, zb, m, cfg, B):
    """Per trajectory and stream step: (idx, y, S) of every update."""
    out = []
    for b in range(B):
        om, oP = means[b].copy(), starts[b].copy()
        rows = []
        for k in range(len(lin)):
            mb = int(m[k, b])
            om, oP, ys, Ss = step_log(om, oP, lin[k, b], ang[k, b], idx[k, b, :mb], zr[k, b, :mb], zb[k, b, :mb], cfg)
            rows.append((idx[k, b, :mb], ys, Ss))
        out.append(rows)
    return out


# ---- per-step kernels, update passes, the small-state path ---------------------------------------------------------------
@pytest.mark.parametrize("fused_step", [1, 0])
def test_per_step_kernels_against_the_oracle(sd, fused_step):
    """step() on the general kernels, N = 300 x 2, six steps of m = 8 (the single-launch step and the two-launch one):
    every entry against the oracle, and the log changes no bit of the result."""
    N, B, steps = 300, 2, 6
    n = 3 + 2 * N
    streams = [orc.synthetic_stream(N, steps, 8, 60 + t) for t in range(B)]
    cfg = orc.EkfConfig()

    def run(log):
        with sd.EkfSlam(n, batch=B) as f:
            f.set_option("small_state", 0)
            f.set_option("fused_step", fused_step)
            f.profile_enable(True)
            if log:
                f.log_innovations(16)
            for b, s in enumerate(streams):
                f.set_state_diag(s[0], s[1], b)
            for k in range(steps):
                f.step(*steps_of(streams, k))
            return (f.innovations() if log else None), final(sd, f)

    innov, on = run(True)
    _, off = run(False)
    same_bits(on, off)
    assert innov.steps.tolist() == list(range(steps)) and innov.idx.shape == (steps, B, 8)
    for b, s in enumerate(streams):
        om, oP = s[0].copy(), np.diag(s[1])
        for k in range(steps):
            om, oP, ys, Ss = step_log(om, oP, s[2][k], s[3][k], s[4][k], s[5][k], s[6][k], cfg)
            check_entries(innov, k, b, s[4][k], ys, Ss)


def test_update_with_more_than_sixteen_and_thirty_two_landmarks(sd, both_paths):
    """ekf_update with m = 20 (two update passes: one logged step), then m = 38 (three passes: the first 32 entries kept,
    the true m reported), then m = 5, on both paths (N = 38: n = 79, the largest small state)."""
    N = 38
    n = 3 + 2 * N
    rng = np.random.default_rng(21)
    mean0 = np.concatenate([[0.1, -0.2, 0.3], rng.uniform(-2, 2, 2 * N)])
    diag0 = np.concatenate([[0.05, 0.05, 0.01], np.full(2 * N, 0.2)])
    cfg = orc.EkfConfig()
    with sd.EkfSlam(n) as f:
        f.log_innovations(8)
        f.set_state_diag(mean0, diag0)
        om, oP = mean0.copy(), np.diag(diag0)
        for k, m in enumerate((20, 38, 5)):
            idx = rng.permutation(N)[:m].astype(np.int32)
            zr = rng.uniform(0.5, 2.0, m)
            zb = rng.uniform(-1.0, 1.0, m)
            f.update(idx, zr, zb)
            om, oP, ys, Ss = update_log(om, oP, idx, zr, zb, cfg)
            innov = f.innovations(k, 1)
            assert innov.steps.tolist() == [k] and innov.idx.shape[2] == min(m, AMAX)
            check_entries(innov, 0, 0, idx, ys, Ss)
        assert path_ran(f, both_paths)
        f.predict(np.array([0.01]), np.array([0.02]))          # a lone prediction is not a logged step
        om, oP = orc.predict_dense(om, oP, 0.01, 0.02, cfg)
        assert f.innovations().steps.tolist() == [0, 1, 2]
        mu, P = f.state()
    assert orc.rel_fro(mu, om) < 1e-9 and orc.rel_fro(P, oP) < 1e-9


def test_small_state_steps_against_the_oracle(sd, both_paths):
    """N = 20, step() x 6 with m = 8 on both paths (the small-state path writes the log from its own launch): against the
    oracle, and bit-identical to the same steps with the log off -- step_state()'s polled launch included."""
    N, steps = 20, 6
    n = 3 + 2 * N
    s = orc.synthetic_stream(N, steps, 8, 5)
    cfg = orc.EkfConfig()

    def run(log):
        with sd.EkfSlam(n) as f:
            if log:
                f.log_innovations(8)
            f.set_state_diag(s[0], s[1])
            states = []
            for k in range(steps):
                if k % 2:
                    states.append(f.step_state(s[2][k], s[3][k], s[4][k], s[5][k], s[6][k]))
                else:
                    f.step(s[2][k], s[3][k], s[4][k], s[5][k], s[6][k])
            assert path_ran(f, both_paths)
            return (f.innovations() if log else None), states, final(sd, f)

    innov, states_on, on = run(True)
    _, states_off, off = run(False)
    same_bits(on, off)
    for (a, pa), (b, pb) in zip(states_on, states_off):
        assert np.array_equal(a, b) and np.array_equal(pa, pb)
    assert innov.steps.tolist() == list(range(steps))
    om, oP = s[0].copy(), np.diag(s[1])
    for k in range(steps):
        om, oP, ys, Ss = step_log(om, oP, s[2][k], s[3][k], s[4][k], s[5][k], s[6][k], cfg)
        check_entries(innov, k, 0, s[4][k], ys, Ss)


def test_step_detections_with_more_than_sixteen_tags(sd):
    """ekf_step_detections with 20 distinct tags in one window (two update passes, one logged step): idx in the device
    association's order (ekf_download_tags), y and S against the oracle's association + augmentation + step."""
    rng = np.random.default_rng(8)
    cfg = orc.EkfConfig()
    ids = [int(i) for i in rng.permutation(200)[:24]]
    bx = {i: float(rng.uniform(-0.5, 0.5)) for i in ids}
    bz = {i: float(rng.uniform(0.4, 1.1)) for i in ids}
    plan = [(ids[:20], 0.004, 0.02), (ids[4:24], 0.004, 0.005), (ids[:6], 0.003, 0.02)]
    with sd.EkfSlam(3 + 2 * 40) as f:
        f.log_innovations(8)
        om, oP, oti = np.zeros(3), np.eye(3) * 0.1, {}
        for k, (win_ids, lin, ang) in enumerate(plan):
            win = [(k + 0.1 * fr, [tag(i, bx[i] + rng.normal(0, 0.004), bz[i] + rng.normal(0, 0.004)) for i in win_ids])
                   for fr in range(3)]
            f.step_detections(lin, ang, win)
            tags = orc.associate(win, oti, om, cfg)
            om, oP = orc.augment(om, oP, len(oti), tags, cfg)
            order = list(tags.keys())
            om, oP, ys, Ss = step_log(om, oP, lin, ang, order, [tags[i][4] for i in order], [tags[i][5] for i in order], cfg)
            assert list(f.tags_positions(0).keys()) == order
            check_entries(f.innovations(k, 1), 0, 0, order, ys, Ss)
        assert f.assoc_fallbacks() == 0


# ---- fused cadences --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", [1, 0])
def test_packed_cadences_on_a_variable_m_stream(sd, chain):
    """The seeded variable-m stream (m ~ uniform{0..8} per step and trajectory, N = 150 x 3, 40 steps) as packed cadences:
    steps cut by a cadence boundary, steps that observe nothing, chained (chain = 1) or look-ahead / plain solves.  Every
    entry against the oracle; the same bits and counters with the log off."""
    N, B, steps = 150, 3, 40
    n = 3 + 2 * N
    means, lin, ang, idx, zr, zb, m = wandering(N, B, steps, 8, 4208)
    starts = [dense_start(n, 4300 + t) for t in range(B)]

    def run(log):
        with sd.EkfSlam(n, batch=B) as f:
            f.set_option("active_bound", 0)
            f.set_option("chain", chain)
            f.profile_enable(True)
            if log:
                f.log_innovations(steps)
            for b in range(B):
                f.set_state(means[b], starts[b], b)
            f.run_stream(lin, ang, idx, zr, zb, m)
            return (f.innovations() if log else None), final(sd, f)

    innov, on = run(True)
    _, off = run(False)
    same_bits(on, off)
    assert on[2][0] > 1 and on[2][1] == steps                   # fused cadences ran the whole stream
    assert (on[2].chained > 0) == bool(chain)
    assert (innov.m == m).all()
    ref = stream_oracle(means, starts, lin, ang, idx, zr, zb, m, orc.EkfConfig(), B)
    for b in range(B):
        for k in range(steps):
            check_entries(innov, k, b, *ref[b][k])


@pytest.mark.parametrize("run_end_flush", [0, 1])
def test_stream_pieces_ending_mid_cadence(sd, run_end_flush):
    """stream_run in pieces whose ends fall inside a cadence and cut a step (m = 7: 40 slots end inside a step), N = 300 x 1,
    chained; with and without run_end_flush.  Against the oracle; log on / off the same bits."""
    N, steps, m = 300, 22, 7
    n = 3 + 2 * N
    s = orc.synthetic_stream(N, steps, m, 77)
    P0 = dense_start(n, 9)
    args = tuple(np.asarray(a)[:, None] for a in (s[2], s[3], s[4], s[5], s[6]))
    pieces = [(0, 7), (7, 6), (13, 9)]

    def run(log):
        with sd.EkfSlam(n) as f:
            f.set_option("run_end_flush", run_end_flush)
            f.profile_enable(True)
            if log:
                f.log_innovations(64)
            f.set_state(s[0], P0)
            f.stream_upload(*args)
            for first, count in pieces:
                f.stream_run(first, count)
            return (f.innovations() if log else None), final(sd, f)

    innov, on = run(True)
    _, off = run(False)
    same_bits(on, off)
    assert on[2][0] > 0
    cfg = orc.EkfConfig()
    om, oP = s[0].copy(), P0.copy()
    for k in range(steps):
        om, oP, ys, Ss = step_log(om, oP, s[2][k], s[3][k], s[4][k], s[5][k], s[6][k], cfg)
        check_entries(innov, k, 0, s[4][k], ys, Ss)


@pytest.mark.parametrize("N,B,steps,opts", [(2000, 1, 60, ()), (2000, 32, 25, ()), (8000, 1, 12, (("active_bound", 1),))])
def test_large_banks_against_the_per_step_kernels(sd, N, B, steps, opts):
    """Sizes the dense oracle cannot afford: the fused run's log equals the per-step kernels' log of the same stream (1e-10):
    N = 2000 x 1 (chained), 32 x N = 2000 (the headline bank), N = 8000 x 1 (column panels, the active bound, from a
    diagonal start).  With the log off the fused run gives the same bits."""
    n = 3 + 2 * N
    streams = [orc.synthetic_stream(N, steps, 8, 500 + t) for t in range(B)]
    args = tuple(np.stack([s[i] for s in streams], axis=1) for i in (2, 3, 4, 5, 6))

    def run(log, fused):
        with sd.EkfSlam(n, batch=B) as f:
            for name, v in opts:
                f.set_option(name, v)
            f.set_option("fused_cadence", fused)
            f.profile_enable(True)
            if log:
                f.log_innovations(steps)
            for b, s in enumerate(streams):
                f.set_state_diag(s[0], s[1], b)
            f.run_stream(*args)
            res = (f.innovations() if log else None), [f.mean(b) for b in range(B)], scheduling(sd, f)
            return res

    fused, ref = run(True, 1), run(True, 0)
    plain = run(False, 1)
    for a, b in zip(fused[1], plain[1]):
        assert np.array_equal(a, b)
    assert fused[2] == plain[2] and fused[2][0] > 0
    if (N, B) == (2000, 1):
        assert fused[2].chained > 0
    i, r = fused[0], ref[0]
    assert (i.m == r.m).all() and (i.idx == r.idx).all() and (i.m == 8).all()
    np.testing.assert_allclose(i.y, r.y, rtol=0, atol=1e-10)
    on = i.m[..., None] > np.arange(i.idx.shape[2])
    assert block_err(i.S[on], r.S[on]) < 1e-10
    np.testing.assert_allclose(i.nis, r.nis, rtol=1e-10, atol=0)


# ---- ring semantics -----------------------------------------------------------------------------------------------------------
def test_ring_wraps_counts_mixed_calls_and_refuses_what_it_does_not_hold(sd):
    lib = sd.load_library()
    N, n = 30, 63
    s = orc.synthetic_stream(N, 12, 4, 3)
    args = tuple(np.asarray(a)[:, None] for a in (s[2], s[3], s[4], s[5], s[6]))
    ip = C.POINTER(C.c_int)
    with sd.EkfSlam(n) as f:
        f.set_state_diag(s[0], s[1])
        with pytest.raises(sd.EkfError):                       # log off
            f.innovations(0, 0)
        f.log_innovations(5)
        f.step(s[2][0], s[3][0], s[4][0], s[5][0], s[6][0])   # step 0
        f.predict(np.array([0.01]), np.array([0.0]))          # not a step
        f.update(s[4][1], s[5][1], s[6][1])                   # step 1
        f.stream_upload(*args)
        f.stream_run(2, 5)                                    # steps 2 .. 6
        f.step_state(s[2][7], s[3][7], s[4][7], s[5][7], s[6][7])   # step 7
        logged = C.c_longlong()
        assert lib.ekf_innovation_steps(f._h, C.byref(logged)) == 0 and logged.value == 8
        innov = f.innovations()                               # the ring holds the last 5: steps 3 .. 7
        assert innov.steps.tolist() == [3, 4, 5, 6, 7] and (innov.m == 4).all()
        assert list(innov.idx[0, 0]) == list(s[4][3])         # stream step 3 is logged step 3
        assert list(innov.idx[4, 0]) == list(s[4][7])
        m = np.zeros(8, dtype=np.int32)
        for first, count in [(2, 1), (0, 5), (7, 2), (8, 1), (-1, 1), (3, -1)]:   # overwritten, future, bad
            assert lib.ekf_download_innovations(f._h, first, count, m.ctypes.data_as(ip), None, None, None, None) == EKF_ERR_ARG
        assert lib.ekf_download_innovations(f._h, 3, 5, None, None, None, None, None) == EKF_ERR_ARG      # NULL m
        assert lib.ekf_download_innovations(f._h, 3, 5, m.ctypes.data_as(ip), None, None, None, None) == 0
        assert (m[:5] == 4).all()
        assert lib.ekf_log_innovations(f._h, -1) == EKF_ERR_ARG
        f.log_innovations(3)                                  # re-enabling restarts the count
        assert f.innovations().steps.tolist() == []
        f.step(s[2][8], s[3][8], s[4][8], s[5][8], s[6][8])
        assert f.innovations().steps.tolist() == [0]
        f.log_innovations(0)
        assert lib.ekf_innovation_steps(f._h, C.byref(logged)) == 0 and logged.value == 0
        with pytest.raises(sd.EkfError):
            f.innovations(0, 0)
