"""GPU: the NIS validation gate (ekf_set_nis_gate / ekf_download_gate_counts / ekf_download_innovation_rejections,
EkfSlam.set_nis_gate / gate_counts, Innovations.rejected).

Outliers are injected into seeded streams (range + 20 m: the reference configuration's measurement noise is 0.7 m).  A gated restatement of the oracle's sequential
update skips an update whose NIS exceeds the threshold; each test asserts its own margin (every injected update's oracle NIS
at least twice the threshold, every other one at most half of it), so that rounding cannot flip a decision.  Where a dense
oracle is affordable, states, logged entries and rejection flags are compared with it; beyond, gated fused cadences against
gated per-step kernels and against an ungated run of the stream with the rejected observations removed.  A threshold no
update reaches changes nothing: same bits, flags and scheduling counters as the gate off."""
import ctypes as C

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests.conftest import path_ran
from tests.gated_oracle import AMAX, G, check_gated_entries, gated_step, gated_update, margin
from tests.gpu_support import final, same_bits, scheduling, sd, tag  # noqa: F401
from tests.streams import dense_start, inject, observed_start, wandering

pytestmark = pytest.mark.gpu

EKF_ERR_ARG = -1
INERT = 1e300           # a threshold no update reaches


def log_flags_match_nis(innov):
    on = innov.rejected >= 0
    assert ((innov.rejected == 1) == (innov.nis > G))[on].all()
    assert (innov.rejected[~on] == -1).all()


# ---- per-step kernels and the small-state path ---------------------------------------------------------------------------
def _per_step_case(N, steps, seed, where):
    s = orc.synthetic_stream(N, steps, 8, seed)
    zr, zb = inject(s[5], s[6], where)
    return observed_start(N, seed) + tuple(s[2:]), zr, zb


@pytest.mark.parametrize("fused_step", [1, 0])
def test_per_step_kernels_against_the_gated_oracle(sd, fused_step):
    """step() on the general kernels, N = 300 x 2, six steps of m = 8, outliers in both trajectories: states, log entries,
    rejection flags and counts against the gated oracle; an inert threshold gives the gate-off bits, flags and counters, and
    the outliers leave the scheduling counters as the gate-off run has them."""
    N, B, steps = 300, 2, 6
    n = 3 + 2 * N
    where = [[(1, 2), (3, 7), (4, 0)], [(2, 5), (5, 1)]]
    cases = [_per_step_case(N, steps, 60 + t, where[t]) for t in range(B)]
    cfg = orc.EkfConfig()

    def run(gate):
        with sd.EkfSlam(n, batch=B) as f:
            f.set_option("small_state", 0)
            f.set_option("fused_step", fused_step)
            f.profile_enable(True)
            f.log_innovations(16)
            if gate is not None:
                f.set_nis_gate(gate)
            for b, (s, _, _) in enumerate(cases):
                f.set_state_diag(s[0], s[1], b)
            for k in range(steps):
                f.step(np.array([c[0][2][k] for c in cases]), np.array([c[0][3][k] for c in cases]),
                       np.stack([c[0][4][k] for c in cases]), np.stack([c[1][k] for c in cases]),
                       np.stack([c[2][k] for c in cases]))
            return f.innovations(), f.gate_counts(), final(sd, f)

    off, inert, on = run(None), run(INERT), run(G)
    same_bits(inert[2], off[2])
    assert (inert[1] == 0).all() and (inert[0].rejected <= 0).all() and (off[0].rejected <= 0).all()
    assert on[2][2] == off[2][2]                                # scheduling counters
    innov = on[0]
    log_flags_match_nis(innov)
    for b, (s, zr, zb) in enumerate(cases):
        om, oP = s[0].copy(), np.diag(s[1])
        injected, nis_all, rej_all = [], [], []
        for k in range(steps):
            om, oP, ys, Ss, nis, rej = gated_step(om, oP, s[2][k], s[3][k], s[4][k], zr[k], zb[k], cfg, G)
            check_gated_entries(innov, k, b, s[4][k], ys, Ss, nis, rej)
            injected += [(k, j) in where[b] for j in range(8)]
            nis_all += list(nis)
            rej_all += list(rej)
        margin(nis_all, rej_all, injected)
        assert on[1][b] == len(where[b])
        mu, P = on[2][0][b]
        assert orc.rel_fro(mu, om) < 1e-9 and orc.rel_fro(P, oP) < 1e-9


def test_small_state_and_general_paths_against_the_gated_oracle(sd, both_paths):
    """N = 20, step() x 6 with m = 8 on both paths, step_state()'s polled launch included; with the log off (the gate in the
    small-state kernels on its own) and on."""
    N, steps = 20, 6
    n = 3 + 2 * N
    where = [(1, 3), (2, 6), (4, 1)]
    s, zr, zb = _per_step_case(N, steps, 5, where)
    cfg = orc.EkfConfig()

    def run(gate, log):
        with sd.EkfSlam(n) as f:
            f.profile_enable(True)
            if log:
                f.log_innovations(8)
            if gate is not None:
                f.set_nis_gate(gate)
            f.set_state_diag(s[0], s[1])
            for k in range(steps):
                if k % 2:
                    f.step_state(s[2][k], s[3][k], s[4][k], zr[k], zb[k])
                else:
                    f.step(s[2][k], s[3][k], s[4][k], zr[k], zb[k])
            assert path_ran(f, both_paths)
            return (f.innovations() if log else None), f.gate_counts(), final(sd, f)

    off = run(None, False)
    inert = run(INERT, False)
    same_bits(inert[2], off[2])
    on_nolog, on = run(G, False), run(G, True)
    same_bits(on_nolog[2], on[2])
    assert on[2][2] == off[2][2]
    assert on[1].tolist() == [len(where)] and on_nolog[1].tolist() == [len(where)]
    om, oP = s[0].copy(), np.diag(s[1])
    nis_all, rej_all, injected = [], [], []
    for k in range(steps):
        om, oP, ys, Ss, nis, rej = gated_step(om, oP, s[2][k], s[3][k], s[4][k], zr[k], zb[k], cfg, G)
        check_gated_entries(on[0], k, 0, s[4][k], ys, Ss, nis, rej)
        nis_all += list(nis)
        rej_all += list(rej)
        injected += [(k, j) in where for j in range(8)]
    margin(nis_all, rej_all, injected)
    mu, P = on[2][0][0]
    assert orc.rel_fro(mu, om) < 1e-9 and orc.rel_fro(P, oP) < 1e-9


def test_update_with_more_than_sixteen_and_thirty_two_landmarks(sd, both_paths):
    """ekf_update with m = 20 (two update passes), m = 38 (three passes; the log keeps 32), then m = 5, outliers in the
    second and third pass, on both paths (N = 38: n = 79)."""
    N = 38
    n = 3 + 2 * N
    rng = np.random.default_rng(21)
    mean0 = np.concatenate([[0.1, -0.2, 0.3], rng.uniform(-2, 2, 2 * N)])
    diag0 = np.concatenate([[0.05, 0.05, 0.01], np.full(2 * N, 0.2)])
    cfg = orc.EkfConfig()
    calls = []
    om = mean0.copy()
    for m in (20, 38, 5):
        idx = rng.permutation(N)[:m].astype(np.int32)
        # measurements consistent with the current mean (small noise), then the outliers
        zr, zb = np.empty(m), np.empty(m)
        for q, j in enumerate(idx):
            d = om[3 + 2 * j:5 + 2 * j] - om[0:2]
            zr[q] = np.hypot(*d) + rng.normal(0, 0.005)
            zb[q] = np.angle(np.exp(1j * (np.arctan2(d[1], d[0]) - om[2]))) + rng.normal(0, 0.005)
        where = {20: [17, 3], 38: [34, 12, 25], 5: [4]}[m]
        zr, zb = inject(zr, zb, where)
        calls.append((idx, zr, zb, where))
    with sd.EkfSlam(n) as f:
        f.log_innovations(8)
        f.set_nis_gate(G)
        f.set_state_diag(mean0, diag0)
        om, oP = mean0.copy(), np.diag(diag0)
        total = 0
        for k, (idx, zr, zb, where) in enumerate(calls):
            f.update(idx, zr, zb)
            om, oP, ys, Ss, nis, rej = gated_update(om, oP, idx, zr, zb, cfg, G)
            margin(nis, rej, [j in where for j in range(len(idx))])
            check_gated_entries(f.innovations(k, 1), 0, 0, idx, ys, Ss, nis, rej)
            total += len(where)
        assert path_ran(f, both_paths)
        assert f.gate_counts().tolist() == [total]
        mu, P = f.state()
    assert orc.rel_fro(mu, om) < 1e-9 and orc.rel_fro(P, oP) < 1e-9


def test_step_detections_with_more_than_sixteen_tags(sd):
    """ekf_step_detections with 20 distinct tags in a window (two update passes), one of them new in the second window (its
    first observation: never rejected), and a misread tag pose (mirrored behind the camera: bearing off by about pi) among
    the known ones.  (The association's 1.5 m range gate bounds what a misread can do, hence a threshold of its own.)"""
    g = 3.0
    rng = np.random.default_rng(8)
    cfg = orc.EkfConfig()
    ids = [int(i) for i in rng.permutation(200)[:24]]
    bx = {i: float(rng.uniform(-0.5, 0.5)) for i in ids}
    bz = {i: float(rng.uniform(0.4, 1.1)) for i in ids}
    plan = [(ids[:20], 0.004, 0.02, None), (ids[3:23], 0.004, 0.005, ids[6]), (ids[:6], 0.003, 0.02, ids[2])]
    with sd.EkfSlam(3 + 2 * 40) as f:
        f.log_innovations(8)
        f.set_nis_gate(g)
        om, oP, oti = np.zeros(3), np.eye(3) * 0.1, {}
        rejected = 0
        for k, (win_ids, lin, ang, bad) in enumerate(plan):
            def det(i):
                x = bx[i] + rng.normal(0, 0.004)
                return tag(i, x, -bz[i] if i == bad else bz[i] + rng.normal(0, 0.004))
            win = [(k + 0.1 * fr, [det(i) for i in win_ids]) for fr in range(3)]
            f.step_detections(lin, ang, win)
            new = [i for i in win_ids if i not in oti]
            tags = orc.associate(win, oti, om, cfg)
            om, oP = orc.augment(om, oP, len(oti), tags, cfg)
            order = list(tags.keys())
            om, oP, ys, Ss, nis, rej = gated_step(om, oP, lin, ang, order, [tags[i][4] for i in order],
                                                  [tags[i][5] for i in order], cfg, g)
            if bad is None:
                assert not rej.any() and (nis <= g / 2).all()
            else:
                margin(nis, rej, [i == oti[bad] for i in order], g)
            if k == 1:
                assert ids[22] in new and not rej[order.index(oti[ids[22]])]
            assert list(f.tags_positions(0).keys()) == order
            check_gated_entries(f.innovations(k, 1), 0, 0, order, ys, Ss, nis, rej)
            rejected += int(rej.sum())
        assert f.gate_counts().tolist() == [rejected] and rejected == 2
        mu, P = f.state()
    assert orc.rel_fro(mu, om) < 1e-9 and orc.rel_fro(P, oP) < 1e-9


# ---- fused cadences --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain,N,B,steps,hi", [(1, 150, 3, 40, 8), (0, 1250, 2, 14, 16)])
def test_packed_cadences_against_the_gated_oracle(sd, chain, N, B, steps, hi):
    """Seeded variable-m streams as packed cadences with outliers in every trajectory: chained solves (chain = 1; N = 150 x 3,
    m ~ U{0..8}, 40 steps) and look-ahead solves beside the pass (chain = 0; N = 1250 x 2 -- the look-ahead wants ~48 MB of
    covariance --, m ~ U{0..16}, 14 steps).  Against the gated oracle; inert threshold = gate-off bits and counters."""
    n = 3 + 2 * N
    means, lin, ang, idx, zr, zb, m = wandering(N, B, steps, hi, 4208 + N)
    starts = [dense_start(n, 4300 + t) for t in range(B)]
    where = []
    rng = np.random.default_rng(17)
    for k in range(5, steps, 4):
        for b in range(B):
            if m[k, b] > 0 and rng.random() < 0.6:
                where.append((k, b, int(rng.integers(0, m[k, b]))))
    zr, zb = inject(zr, zb, where)

    def run(gate):
        with sd.EkfSlam(n, batch=B) as f:
            f.set_option("active_bound", 0)
            f.set_option("chain", chain)
            f.profile_enable(True)
            f.log_innovations(steps)
            if gate is not None:
                f.set_nis_gate(gate)
            for b in range(B):
                f.set_state(means[b], starts[b], b)
            f.run_stream(lin, ang, idx, zr, zb, m)
            return f.innovations(), f.gate_counts(), final(sd, f)

    off, inert, on = run(None), run(INERT), run(G)
    same_bits(inert[2], off[2])
    assert on[2][2] == off[2][2]
    assert on[2][2].cadences > 1 and on[2][2].covered == steps
    if chain:
        assert on[2][2].chained > 0
    else:
        assert on[2][2].lookaheads > 0
    log_flags_match_nis(on[0])
    cfg = orc.EkfConfig()
    for b in range(B):
        om, oP = means[b].copy(), starts[b].copy()
        nis_all, rej_all, injected = [], [], []
        for k in range(steps):
            mb = int(m[k, b])
            om, oP, ys, Ss, nis, rej = gated_step(om, oP, lin[k, b], ang[k, b], idx[k, b, :mb], zr[k, b, :mb], zb[k, b, :mb],
                                                  cfg, G)
            check_gated_entries(on[0], k, b, idx[k, b, :mb], ys, Ss, nis, rej)
            nis_all += list(nis)
            rej_all += list(rej)
            injected += [(k, b, j) in where for j in range(mb)]
        margin(nis_all, rej_all, injected)
        assert on[1][b] == sum(1 for w in where if w[1] == b)
        mu, P = on[2][0][b]
        assert orc.rel_fro(mu, om) < 1e-9 and orc.rel_fro(P, oP) < 1e-9


@pytest.mark.parametrize("run_end_flush", [0, 1])
def test_stream_pieces_ending_mid_cadence(sd, run_end_flush):
    """stream_run in pieces whose ends fall inside a cadence and cut a step, N = 300 x 1, chained, outliers in cut steps:
    against the gated oracle; inert threshold = gate-off bits and counters."""
    N, steps, mm = 300, 22, 7
    n = 3 + 2 * N
    s = orc.synthetic_stream(N, steps, mm, 77)
    where = [(5, 5), (6, 0), (12, 6), (17, 3)]
    zr, zb = inject(s[5], s[6], where)
    P0 = dense_start(n, 9)
    args = tuple(np.asarray(a)[:, None] for a in (s[2], s[3], s[4], zr, zb))
    pieces = [(0, 7), (7, 6), (13, 9)]

    def run(gate):
        with sd.EkfSlam(n) as f:
            f.set_option("run_end_flush", run_end_flush)
            f.profile_enable(True)
            f.log_innovations(64)
            if gate is not None:
                f.set_nis_gate(gate)
            f.set_state(s[0], P0)
            f.stream_upload(*args)
            for first, count in pieces:
                f.stream_run(first, count)
            return f.innovations(), f.gate_counts(), final(sd, f)

    off, inert, on = run(None), run(INERT), run(G)
    same_bits(inert[2], off[2])
    assert on[2][2] == off[2][2] and on[2][2].cadences > 0
    cfg = orc.EkfConfig()
    om, oP = s[0].copy(), P0.copy()
    nis_all, rej_all, injected = [], [], []
    for k in range(steps):
        om, oP, ys, Ss, nis, rej = gated_step(om, oP, s[2][k], s[3][k], s[4][k], zr[k], zb[k], cfg, G)
        check_gated_entries(on[0], k, 0, s[4][k], ys, Ss, nis, rej)
        nis_all += list(nis)
        rej_all += list(rej)
        injected += [(k, j) in where for j in range(mm)]
    margin(nis_all, rej_all, injected)
    assert on[1].tolist() == [len(where)]
    mu, P = on[2][0][0]
    assert orc.rel_fro(mu, om) < 1e-9 and orc.rel_fro(P, oP) < 1e-9


@pytest.mark.parametrize("N,B,steps,opts", [(2000, 1, 40, ()), (2000, 32, 16, ()), (8000, 1, 10, (("active_bound", 1),))])
def test_large_banks_gated_equal_per_step_and_outliers_removed(sd, N, B, steps, opts):
    """Sizes the dense oracle cannot afford (N = 2000 x 1 chained, 32 x N = 2000, N = 8000 x 1 with the active bound): gated
    fused cadences equal gated per-step kernels, and both equal an ungated run of the stream with the rejected observations
    removed (means, 1e-10); an inert threshold gives the gate-off bits and counters."""
    n = 3 + 2 * N
    streams = [observed_start(N, 500 + t) + tuple(orc.synthetic_stream(N, steps, 8, 500 + t)[2:]) for t in range(B)]
    lin, ang, idx, zr, zb = (np.stack([s[i] for s in streams], axis=1) for i in (2, 3, 4, 5, 6))
    m = np.full((steps, B), 8, dtype=np.int32)
    where = [(k, b, (3 * k + b) % 8) for k in range(4, steps, 5) for b in range(B)]
    zr, zb = inject(zr, zb, where)

    def run(gate, fused, lin=lin, ang=ang, idx=idx, zr=zr, zb=zb, m=m):
        with sd.EkfSlam(n, batch=B) as f:
            for name, v in opts:
                f.set_option(name, v)
            f.set_option("fused_cadence", fused)
            f.profile_enable(True)
            f.log_innovations(steps)
            if gate is not None:
                f.set_nis_gate(gate)
            for b, s in enumerate(streams):
                f.set_state_diag(s[0], s[1], b)
            f.run_stream(lin, ang, idx, zr, zb, m)
            return f.innovations(), f.gate_counts(), [f.mean(b) for b in range(B)], None, scheduling(sd, f)

    fused, per_step = run(G, 1), run(G, 0)
    off, inert = run(None, 1), run(INERT, 1)
    for a, b in zip(off[2], inert[2]):
        assert np.array_equal(a, b)
    assert off[4] == inert[4] == fused[4] and fused[4][0] > 0
    if (N, B) == (2000, 1):
        assert fused[4][2] > 0                                  # chained
    rej = fused[0].rejected
    assert (rej == per_step[0].rejected).all()
    assert int((rej == 1).sum()) == len(where) and fused[1].tolist() == per_step[1].tolist()
    for (k, b, j) in where:
        assert rej[k, b, j] == 1
    # the same stream with the rejected observations removed, ungated
    keep = rej != 1
    idx2, zr2, zb2 = np.zeros_like(idx), np.zeros_like(zr), np.zeros_like(zb)
    m2 = keep.sum(axis=2).astype(np.int32)
    for k in range(steps):
        for b in range(B):
            sel = np.nonzero(keep[k, b])[0]
            idx2[k, b, :len(sel)], zr2[k, b, :len(sel)], zb2[k, b, :len(sel)] = idx[k, b, sel], zr[k, b, sel], zb[k, b, sel]
    removed = run(None, 1, idx=idx2, zr=zr2, zb=zb2, m=m2)
    for b in range(B):
        scale = np.abs(per_step[2][b]).max()
        assert np.abs(fused[2][b] - per_step[2][b]).max() <= 1e-10 * scale
        assert np.abs(removed[2][b] - per_step[2][b]).max() <= 1e-10 * scale
    on = fused[0].rejected >= 0
    np.testing.assert_allclose(fused[0].nis[on], per_step[0].nis[on], rtol=1e-10, atol=0)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_abi_arguments_counts_and_clearing(sd):
    lib = sd.load_library()
    N, n = 30, 63
    s = observed_start(N, 3) + tuple(orc.synthetic_stream(N, 8, 4, 3)[2:])
    zr, zb = inject(s[5], s[6], [(2, 1), (5, 3)])
    ll = C.POINTER(C.c_longlong)
    with sd.EkfSlam(n, batch=2) as f:
        for bad in (0.0, -1.0, float("nan"), float("-inf")):
            assert lib.ekf_set_nis_gate(f._h, bad) == EKF_ERR_ARG
        cnt = np.zeros(2, dtype=np.int64)
        for b0, count in ((0, 3), (-1, 1), (2, 1), (0, 0)):
            assert lib.ekf_download_gate_counts(f._h, b0, count, cnt.ctypes.data_as(ll)) == EKF_ERR_ARG
        rej = np.zeros(AMAX * 2, dtype=np.int32)
        assert lib.ekf_download_innovation_rejections(f._h, 0, 0, rej.ctypes.data_as(C.POINTER(C.c_int))) != 0   # log off
        assert f.gate_counts().tolist() == [0, 0]                # never switched on
        for b in range(2):
            f.set_state_diag(s[0], s[1], b)
        f.set_nis_gate(confidence=0.999999999)                  # chi2_2 quantile: 41.4
        f.log_innovations(8)
        for k in range(8):
            f.step(np.full(2, s[2][k]), np.full(2, s[3][k]), np.stack([s[4][k]] * 2), np.stack([zr[k], s[5][k]]),
                   np.stack([zb[k], s[6][k]]))
        assert f.gate_counts().tolist() == [2, 0]
        innov = f.innovations()
        assert innov.rejected.shape == innov.nis.shape and int((innov.rejected == 1).sum()) == 2
        assert innov.rejected[2, 0, 1] == 1 and innov.rejected[5, 0, 3] == 1
        f.set_nis_gate(G)                                       # clears the counters
        assert f.gate_counts().tolist() == [0, 0]
        f.set_nis_gate(None)                                    # off
        f.step(np.full(2, s[2][0]), np.full(2, s[3][0]), np.stack([s[4][0]] * 2), np.stack([zr[2]] * 2),
               np.stack([zb[2]] * 2))
        assert f.gate_counts().tolist() == [0, 0] and (f.innovations().rejected[-1] <= 0).all()
