"""Per-trajectory noise constants (ekf_set_noise / EkfSlam.set_noise) against the oracle run under each trajectory's own
EkfConfig(motion_sigma, meas_sigma), on every path that predicts or updates; the table off is today's bits; the tuning
sweep (evaluation.tune_noise) against separate handles and on a stream with known noise."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests.conftest import path_ran
from tests.gated_oracle import AMAX, block_err, gated_step, margin
from tests.gpu_support import counters, final, same_bits, sd  # noqa: F401
from tests.streams import dense_start, inject, observed_start, wandering

pytestmark = pytest.mark.gpu

EKF_ERR_ARG = -1
G = 25.0
BASE = orc.EkfConfig()


def sigmas(B, seed):
    """Distinct noise rows; trajectory 0 keeps the handle's constants."""
    rng = np.random.default_rng(seed)
    ms = rng.uniform(0.03, 0.3, B)
    qs = rng.uniform(0.2, 1.5, B)
    ms[0], qs[0] = BASE.motion_sigma, BASE.meas_sigma
    return ms, qs


def cfg_of(ms, qs, b):
    return orc.EkfConfig(motion_sigma=float(ms[b]), meas_sigma=float(qs[b]))


def oracle_stream(mean0, P0, lin, ang, idx, zr, zb, m, cfgs, g=math.inf, switch=None):
    """Per trajectory: the final state and, per step, (y, S, NIS, rejected) of every update.  switch = (k, cfgs2): steps
    k.. run under cfgs2."""
    out = []
    for b in range(len(cfgs)):
        om, oP = mean0[b].copy(), P0[b].copy()
        rows = []
        for k in range(len(lin)):
            cfg = switch[1][b] if switch is not None and k >= switch[0] else cfgs[b]
            mb = int(m[k, b])
            om, oP, ys, Ss, nis, rej = gated_step(om, oP, lin[k, b], ang[k, b], idx[k, b, :mb], zr[k, b, :mb], zb[k, b, :mb],
                                                  cfg, g)
            rows.append((ys, Ss, nis, rej))
        out.append((om, oP, rows))
    return out


def check_log(innov, orc_out, m, tol=1e-9):
    for b, (_, _, rows) in enumerate(orc_out):
        for k, (ys, Ss, nis, rej) in enumerate(rows):
            kept = min(int(m[k, b]), AMAX)
            assert innov.m[k, b] == m[k, b]
            np.testing.assert_allclose(innov.y[k, b, :kept], ys[:kept], rtol=0, atol=1e-9)
            assert block_err(innov.S[k, b, :kept], Ss[:kept]) < tol
            np.testing.assert_allclose(innov.nis[k, b, :kept], nis[:kept], rtol=tol, atol=0)
            assert innov.rejected[k, b, :kept].tolist() == [int(r) for r in rej[:kept]]


def check_states(f, orc_out, tol=1e-10):
    for b, (om, oP, _) in enumerate(orc_out):
        mu, P = f.state(b)
        assert orc.rel_fro(mu, om) < tol and orc.rel_fro(P, oP) < tol, (b, orc.rel_fro(mu, om), orc.rel_fro(P, oP))


def tiled(N, B, steps, seed, hi=8):
    means, lin, ang, idx, zr, zb, m = wandering(N, B, steps, hi, seed)
    return means, lin, ang, idx, zr, zb, m


# ---- 1. distinct rows on every path -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["step", "predict_update", "step_state"])
def test_per_step_calls_distinct_rows(sd, both_paths, how):
    """step / predict + update / step_state (ekf_step_fetch) with a distinct noise row per trajectory, on the small-state
    path and on the general per-step kernels; state and innovation log against each trajectory's oracle."""
    N, B, steps = 20, 4, 12
    n = 3 + 2 * N
    means, lin, ang, idx, zr, zb, m = tiled(N, B, steps, 5100)
    P0 = [dense_start(n, 5200 + b) for b in range(B)]
    ms, qs = sigmas(B, 1)
    with sd.EkfSlam(n, batch=B) as f:
        f.set_noise(ms, qs)
        got_m, got_q = f.noise()
        assert np.array_equal(got_m, ms) and np.array_equal(got_q, qs)
        f.log_innovations(steps)
        for b in range(B):
            f.set_state(means[b], P0[b], b)
        for k in range(steps):
            obs = ([idx[k, b, :m[k, b]] for b in range(B)], [zr[k, b, :m[k, b]] for b in range(B)],
                   [zb[k, b, :m[k, b]] for b in range(B)])
            if how == "step":
                f.step(lin[k], ang[k], *obs)
            elif how == "predict_update":
                f.predict(lin[k], ang[k])
                f.update(*obs)
            else:
                f.step_state(lin[k], ang[k], *obs, b=k % B)
        ref = oracle_stream(means, P0, lin, ang, idx, zr, zb, m, [cfg_of(ms, qs, b) for b in range(B)])
        check_states(f, ref)
        if how != "predict_update":
            check_log(f.innovations(), ref, m)
        assert path_ran(f, both_paths)


@pytest.mark.parametrize("chain,N,B,steps,hi", [(1, 150, 3, 40, 8), (0, 1250, 2, 14, 16)])
def test_packed_cadences_distinct_rows(sd, chain, N, B, steps, hi):
    """Fused cadences: chained solves (chain = 1) and look-ahead solves beside the pass (chain = 0), distinct rows."""
    n = 3 + 2 * N
    means, lin, ang, idx, zr, zb, m = tiled(N, B, steps, 4208 + N, hi)
    P0 = [dense_start(n, 4300 + t) for t in range(B)]
    ms, qs = sigmas(B, 2)
    ms[0] *= 1.5                                             # (every row distinct from the handle's here)
    with sd.EkfSlam(n, batch=B) as f:
        f.set_option("active_bound", 0)
        f.set_option("chain", chain)
        f.profile_enable(True)
        f.log_innovations(steps)
        f.set_noise(ms, qs)
        for b in range(B):
            f.set_state(means[b], P0[b], b)
        f.run_stream(lin, ang, idx, zr, zb, m)
        c = counters(sd, f)
        assert c.cadences > 1 and c.covered == steps
        assert (c.chained > 0) if chain else (c.lookaheads > 0)
        ref = oracle_stream(means, P0, lin, ang, idx, zr, zb, m, [cfg_of(ms, qs, b) for b in range(B)])
        check_log(f.innovations(), ref, m)
        check_states(f, ref)


def test_active_bound_with_column_panels(sd):
    """n > 4096 (column panels), the active bound on: a few cadences of two trajectories with their own noise."""
    N, B, steps = 2100, 1, 8
    n = 3 + 2 * N
    means, lin, ang, idx, zr, zb, m = tiled(N, B, steps, 7100, 4)
    P0 = [np.diag(np.r_[np.full(3, 0.01), np.full(2 * N, 1.0)]) for _ in range(B)]
    ms, qs = np.array([0.05]), np.array([0.4])
    with sd.EkfSlam(n, batch=B) as f:
        f.set_option("active_bound", 1)
        f.set_noise(ms, qs)
        for b in range(B):
            f.set_state_diag(means[b], np.diag(P0[b]), b)
        f.run_stream(lin, ang, idx, zr, zb, m)
        ref = oracle_stream(means, P0, lin, ang, idx, zr, zb, m, [cfg_of(ms, qs, b) for b in range(B)])
        check_states(f, ref, tol=1e-10)


def test_small_state_bank_of_128(sd, both_paths):
    """A bank of 128 at N = 20 (the small-state bank forms) with a distinct row per trajectory; every trajectory checked."""
    N, B, steps = 20, 128, 10
    n = 3 + 2 * N
    means, lin, ang, idx, zr, zb, m = tiled(N, B, steps, 9100, 6)
    P0 = [np.diag(np.r_[np.full(3, 0.01), np.full(2 * N, 1.0)]) for _ in range(B)]
    ms, qs = sigmas(B, 3)
    with sd.EkfSlam(n, batch=B) as f:
        f.set_noise(ms, qs)
        f.log_innovations(steps)
        for b in range(B):
            f.set_state_diag(means[b], np.diag(P0[b]), b)
        f.run_stream(lin, ang, idx, zr, zb, m)
        ref = oracle_stream(means, P0, lin, ang, idx, zr, zb, m, [cfg_of(ms, qs, b) for b in range(B)])
        check_states(f, ref)
        check_log(f.innovations(), ref, m)
        assert path_ran(f, both_paths)


# ---- 2. the table off is today's bits ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain,N,B,steps", [(1, 150, 3, 24), (0, 20, 4, 12)])
def test_table_off_is_todays_bits(sd, chain, N, B, steps, capsys):
    n = 3 + 2 * N
    means, lin, ang, idx, zr, zb, m = tiled(N, B, steps, 3300 + N, 8)
    P0 = [dense_start(n, 3400 + t) for t in range(B)]
    ms, qs = sigmas(B, 4)

    def run(setup):
        with sd.EkfSlam(n, batch=B) as f:
            f.set_option("chain", chain)
            f.profile_enable(True)
            setup(f)
            for b in range(B):
                f.set_state(means[b], P0[b], b)
            f.run_stream(lin, ang, idx, zr, zb, m)
            return final(sd, f)

    fresh = run(lambda f: None)
    same_bits(run(lambda f: (f.set_noise(ms, qs), f.set_noise())), fresh)
    same_bits(run(lambda f: f.set_noise(BASE.motion_sigma, BASE.meas_sigma)), fresh)
    mixed = run(lambda f: f.set_noise(ms, qs))               # trajectory 0's row is the handle's constants
    (mu0, P0a), (mu1, P1a) = mixed[0][0], fresh[0][0]
    assert orc.rel_fro(mu0, mu1) < 1e-12 and orc.rel_fro(P0a, P1a) < 1e-12
    assert mixed[2] == fresh[2]
    with capsys.disabled():
        print(f"\n[noise bank] mixed bank, handle-constant row bit-identical to no table (chain={chain}, N={N}): "
              f"{np.array_equal(mu0, mu1) and np.array_equal(P0a, P1a)}")


# ---- 3. a change between two pieces ----------------------------------------------------------------------------------------------
def test_change_between_chained_stream_pieces(sd):
    N, B, steps, k = 150, 3, 32, 13
    n = 3 + 2 * N
    means, lin, ang, idx, zr, zb, m = tiled(N, B, steps, 6100, 8)
    P0 = [dense_start(n, 6200 + t) for t in range(B)]
    ms, qs = sigmas(B, 5)
    ms2, qs2 = ms[::-1].copy() * 0.7, qs[::-1].copy() * 1.3
    with sd.EkfSlam(n, batch=B) as f:
        f.set_option("chain", 1)
        f.profile_enable(True)
        f.set_noise(ms, qs)
        for b in range(B):
            f.set_state(means[b], P0[b], b)
        f.stream_upload(lin, ang, idx, zr, zb, m)
        f.stream_run(0, k)
        f.set_noise(ms2, qs2)
        f.stream_run(k, steps - k)
        assert counters(sd, f).chained > 0
        ref = oracle_stream(means, P0, lin, ang, idx, zr, zb, m, [cfg_of(ms, qs, b) for b in range(B)],
                            switch=(k, [cfg_of(ms2, qs2, b) for b in range(B)]))
        check_states(f, ref)


def test_change_between_per_step_calls_with_ranks_pending(sd, general_kernels):
    N, B, steps, k = 300, 2, 10, 4
    n = 3 + 2 * N
    means, lin, ang, idx, zr, zb, m = tiled(N, B, steps, 6300, 8)
    P0 = [dense_start(n, 6400 + t) for t in range(B)]
    ms, qs = sigmas(B, 6)
    ms2, qs2 = ms * 2.0, qs * 0.5
    with sd.EkfSlam(n, batch=B) as f:
        f.set_noise(ms, qs)
        for b in range(B):
            f.set_state(means[b], P0[b], b)
        for t in range(steps):
            if t == k:
                f.set_noise(ms2, qs2)                        # (ranks of steps 0..k-1 are pending: no flush between)
            f.step(lin[t], ang[t], [idx[t, b, :m[t, b]] for b in range(B)], [zr[t, b, :m[t, b]] for b in range(B)],
                   [zb[t, b, :m[t, b]] for b in range(B)])
        ref = oracle_stream(means, P0, lin, ang, idx, zr, zb, m, [cfg_of(ms, qs, b) for b in range(B)],
                            switch=(k, [cfg_of(ms2, qs2, b) for b in range(B)]))
        check_states(f, ref)


# ---- 4. the NIS gate under each trajectory's noise -----------------------------------------------------------------------------
def test_gate_with_per_trajectory_noise(sd, both_paths):
    N, B, steps = 20, 3, 16
    n = 3 + 2 * N
    s = [orc.synthetic_stream(N, steps, 8, 11 + b) for b in range(B)]
    starts = [observed_start(N, 11 + b) for b in range(B)]
    lin = np.stack([x[2] for x in s], 1)
    ang = np.stack([x[3] for x in s], 1)
    idx = np.stack([np.asarray(x[4]) for x in s], 1).astype(np.int32)
    zr = np.stack([np.asarray(x[5]) for x in s], 1)
    zb = np.stack([np.asarray(x[6]) for x in s], 1)
    m = np.full((steps, B), idx.shape[2], dtype=np.int32)
    where = [(k, b, (k + b) % 8) for k in range(3, steps, 4) for b in range(B)]
    zr, zb = inject(zr, zb, where)
    ms, qs = np.array([0.1, 0.12, 0.15]), np.array([0.7, 0.85, 1.0])
    with sd.EkfSlam(n, batch=B) as f:
        f.set_noise(ms, qs)
        f.set_nis_gate(G)
        f.log_innovations(steps)
        for b in range(B):
            f.set_state_diag(starts[b][0], starts[b][1], b)
        f.run_stream(lin, ang, idx, zr, zb, m)
        P0 = [np.diag(st[1]) for st in starts]
        ref = oracle_stream([st[0] for st in starts], P0, lin, ang, idx, zr, zb, m, [cfg_of(ms, qs, b) for b in range(B)], g=G)
        check_states(f, ref)
        check_log(f.innovations(), ref, m)
        counts = f.gate_counts()
        for b in range(B):
            nis = np.concatenate([r[2] for r in ref[b][2]])
            rej = np.concatenate([r[3] for r in ref[b][2]])
            injected = [(k, b, j) in where for k in range(steps) for j in range(m[k, b])]
            margin(nis, rej, injected)
            assert counts[b] == rej.sum()
        assert path_ran(f, both_paths)


# ---- 5. marginals mid-cadence --------------------------------------------------------------------------------------------------
def test_marginals_mid_cadence_equal_flushed_blocks(sd):
    N, B, steps = 150, 2, 11
    n = 3 + 2 * N
    means, lin, ang, idx, zr, zb, m = tiled(N, B, steps, 8100, 8)
    P0 = [dense_start(n, 8200 + t) for t in range(B)]
    ms, qs = sigmas(B, 8)
    ms[0] *= 0.5
    with sd.EkfSlam(n, batch=B) as f:
        f.set_noise(ms, qs)
        for b in range(B):
            f.set_state(means[b], P0[b], b)
        f.stream_upload(lin, ang, idx, zr, zb, m)
        f.stream_run(0, steps)
        pose, lms, cnt = f.marginals()
        for b in range(B):
            _, P = f.state(b)
            assert orc.rel_fro(pose[b], P[:3, :3]) < 1e-10
            for j in range(int(cnt[b])):
                t = 3 + 2 * j
                assert orc.rel_fro(lms[b, j], P[t:t + 2, t:t + 2]) < 1e-10


# ---- 6, 7. the tuning sweep ------------------------------------------------------------------------------------------------------
def test_tune_noise_equals_separate_handles(sd):
    import slam_duckietown_amd.evaluation as ev
    N, steps = 12, 40
    n = 3 + 2 * N
    means, lin, ang, idx, zr, zb, m = tiled(N, 1, steps, 9300, 6)
    mean0 = means[0]
    diag0 = np.r_[np.full(3, 1e-3), np.full(2 * N, 0.05)]
    mgrid, qgrid = np.array([0.05, 0.1, 0.2]), np.array([0.3, 0.7, 1.2])
    stream = (lin[:, 0], ang[:, 0], idx[:, 0], zr[:, 0], zb[:, 0], m[:, 0])
    res = ev.tune_noise(stream, mgrid, qgrid, mean0, diag0)
    assert res.bank_sizes == (9,) and res.loglik.shape == (3, 3) and res.traj_bounds.shape == (3, 3, 2)
    for i, s in enumerate(mgrid):
        for j, q in enumerate(qgrid):
            with sd.EkfSlam(n, batch=1, config=sd.EkfConfig(motion_sigma=float(s), meas_sigma=float(q))) as f:
                f.set_state_diag(mean0, diag0)
                f.log_innovations(steps)
                f.run_stream(lin[:, :1], ang[:, :1], idx[:, :1], zr[:, :1], zb[:, :1], m[:, :1])
                want = ev.nis_consistency(f.innovations(0, steps)).loglik[0]
            assert abs(res.loglik[i, j] - want) <= 1e-9 * abs(want), (s, q, res.loglik[i, j], want)
    assert res.best == (float(mgrid[np.unravel_index(np.argmax(res.loglik), res.loglik.shape)[0]]),
                        float(qgrid[np.unravel_index(np.argmax(res.loglik), res.loglik.shape)[1]]))
    two = ev.tune_noise(stream, mgrid, qgrid, mean0, diag0, bank_size=4)     # several banks: the same grid
    assert two.bank_sizes == (3, 3, 3)
    np.testing.assert_allclose(two.loglik, res.loglik, rtol=1e-12, atol=0)


def test_tune_noise_finds_the_generating_pair(sd):
    """A stream drawn from the reference's own noise model (pose noise R = diag(s^2, s^2, (s/2)^2) per step, range and bearing
    noise Q = diag(q^2, q^2)): the generating pair has a clearly larger loglik than pairs 4 x away in either direction."""
    import slam_duckietown_amd.evaluation as ev
    sm, sq = 0.02, 0.05
    N, steps = 12, 300
    rng = np.random.default_rng(2024)
    ang_ = np.linspace(0, 2 * np.pi, N, endpoint=False)
    lm = np.stack([2.0 * np.cos(ang_), 2.0 * np.sin(ang_)], 1)
    cfg = orc.EkfConfig(motion_sigma=sm, meas_sigma=sq)
    lin = np.full(steps, 0.02)
    ang = np.full(steps, 0.03)
    idx = np.zeros((steps, 4), dtype=np.int32)
    zr, zb = np.zeros((steps, 4)), np.zeros((steps, 4))
    pose = np.zeros(3)
    R = np.sqrt(cfg.motion_noise_diag())
    for k in range(steps):
        pose, _ = orc.motion_model(pose, lin[k], ang[k], cfg)
        pose = pose + rng.normal(0.0, 1.0, 3) * R
        d = lm - pose[:2]
        dist = np.hypot(d[:, 0], d[:, 1])
        vis = np.argsort(dist)[:4]
        idx[k] = vis
        zr[k] = dist[vis] + rng.normal(0.0, sq, 4)
        b_ = np.arctan2(d[vis, 1], d[vis, 0]) - pose[2] + rng.normal(0.0, sq, 4)
        zb[k] = np.arctan2(np.sin(b_), np.cos(b_))
    mean0 = np.r_[np.zeros(3), lm.ravel()]
    diag0 = np.r_[np.full(3, 1e-8), np.full(2 * N, 1e-8)]
    grid_m = np.array([sm / 4, sm, sm * 4])
    grid_q = np.array([sq / 4, sq, sq * 4])
    res = ev.tune_noise((lin, ang, idx, zr, zb), grid_m, grid_q, mean0, diag0)
    assert res.best == (sm, sq)
    centre = res.loglik[1, 1]
    for i, j in [(0, 1), (2, 1), (1, 0), (1, 2)]:
        assert centre - res.loglik[i, j] > 20.0, (i, j, centre, res.loglik[i, j])


# ---- 8. arguments -----------------------------------------------------------------------------------------------------------------
def test_abi_arguments_and_handle_stays_usable(sd):
    lib = sd.load_library()
    N, B = 20, 3
    n = 3 + 2 * N
    dp = C.POINTER(C.c_double)
    with sd.EkfSlam(n, batch=B) as f:
        ok = np.array([0.1, 0.2, 0.3])
        bad = [((-1, 1, ok, ok), "range"), ((2, 2, ok, ok), "range"), ((0, 0, ok, ok), "range"),
               ((0, 3, np.array([0.1, np.nan, 0.1]), ok), "motion_sigma[1] is not finite"),
               ((0, 3, np.array([0.1, -0.1, 0.1]), ok), "motion_sigma[1] < 0"),
               ((0, 3, ok, np.array([0.1, 0.1, 0.0])), "meas_sigma[2] <= 0"),
               ((0, 3, ok, np.array([np.inf, 0.1, 0.1])), "meas_sigma[0] is not finite")]
        for (b0, cnt, a, q), msg in bad:
            rc = lib.ekf_set_noise(f._h, b0, cnt, a.ctypes.data_as(dp), q.ctypes.data_as(dp))
            assert rc == EKF_ERR_ARG and msg in lib.ekf_last_error(f._h).decode()
        got = f.noise()
        assert (got[0] == BASE.motion_sigma).all() and (got[1] == BASE.meas_sigma).all()   # nothing changed
        assert lib.ekf_set_noise(f._h, 1, 2, None, np.array([0.5, 0.6]).ctypes.data_as(dp)) == 0
        got = f.noise()
        assert got[0].tolist() == [BASE.motion_sigma] * 3 and got[1].tolist() == [BASE.meas_sigma, 0.5, 0.6]
        out = np.zeros(1)
        assert lib.ekf_get_noise(f._h, 3, 1, out.ctypes.data_as(dp), None) == EKF_ERR_ARG
        for wrong in (dict(motion_sigma=[0.1, 0.2]), dict(meas_sigma=0.0), dict(motion_sigma=np.nan)):
            with pytest.raises(ValueError):
                f.set_noise(**wrong)
        mean0, diag0 = np.zeros(n), np.r_[np.full(3, 0.01), np.full(2 * N, 1.0)]
        f.set_state_diag(mean0, diag0, 0)
        f.step(0.01, 0.02, [[0], [], []], [[1.0], [], []], [[0.1], [], []])   # usable
        om, oP = orc.ekf_step_dense(mean0, np.diag(diag0), 0.01, 0.02, [0], [1.0], [0.1], BASE)
        mu, P = f.state(0)
        assert orc.rel_fro(mu, om) < 1e-10 and orc.rel_fro(P, oP) < 1e-10
