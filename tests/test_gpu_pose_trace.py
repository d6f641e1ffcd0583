"""GPU: the pose log (ekf_log_poses / ekf_download_poses, EkfSlam.log_poses / poses).

Row k against the oracle stepped one step at a time -- (mu[:3], P[:3, :3]) after oracle step k: the mean to 1e-9 absolute,
the block to 1e-9 relative -- where a dense oracle is affordable; beyond (N = 2000), against the trace of the same stream
on the per-step kernels (parity_blocks.PATH_CORR_TOL).  Two invariants on every case: switching the log on changes no bit
of mean, covariance, flags or scheduling counters, and the last row is the filter (mean bit for bit, block to 1e-10)."""
import ctypes as C

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests.conftest import path_ran
from tests.parity_blocks import PATH_CORR_TOL
from tests.gpu_support import counters, final, same_bits, sd, tag  # noqa: F401
from tests.streams import dense_start, steps_of

pytestmark = pytest.mark.gpu

EKF_ERR_ARG = -1
EKF_ERR_STATE = -3


# ---- helpers -----------------------------------------------------------------------------------------------------------------
G = 13.8                                                    # NIS gate of the gated cases: the chi-square(2) quantile at 0.999
SLOTS = 40                                                  # landmark updates a cadence takes: "rank_limit" / 2, set by the tests


def variable_bank(N, B, steps, hi, seed):
    """synthetic.variable_stream per trajectory, stacked: means, lin (steps, B), ang, idx (steps, B, hi), zr, zb, m (steps, B)."""
    from slam_duckietown_amd import synthetic as syn
    st = [syn.variable_stream(N, steps, 0, hi, seed + b) for b in range(B)]
    return ([s[0] for s in st],) + tuple(np.stack([s[i] for s in st], axis=1) for i in (2, 3, 4, 5, 6, 7))


def gated_step_count(mean, cov, lin, ang, idx, ranges, bearings, cfg, g=np.inf):
    """The oracle's step (predict_dense, then update_dense's sequential updates) with the NIS gate: an update whose NIS
    exceeds g leaves mean and covariance as they are.  Returns the state and the number of rejections."""
    mean, cov = orc.predict_dense(mean, cov, lin, ang, cfg)
    n, rejected = len(mean), 0
    mean = np.array(mean, dtype=float)
    Q = np.diag(cfg.meas_noise_diag())
    for j, zr, zb in zip(idx, ranges, bearings):
        t = 3 + 2 * int(j)
        y, h5 = orc.innovation_and_h5(mean[0:3], mean[t:t + 2], zr, zb)
        y = np.asarray(y, dtype=float).ravel()
        H = np.zeros((2, n))
        H[:, 0:3] = h5[:, 0:3]
        H[:, t:t + 2] = h5[:, 3:5]
        HP = H @ cov
        S = HP @ H.T + Q
        if float(y @ np.linalg.solve(S, y)) > g:
            rejected += 1
            continue
        K = HP.T @ np.linalg.inv(S)
        mean = mean + K @ y
        cov = cov - K @ HP
    return mean, cov, rejected


def blk_err(got, want):
    got, want = np.asarray(got).reshape(-1, 9), np.asarray(want).reshape(-1, 9)
    return float(np.max(np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)))


def check_rows(trace, b, ref, rows=None, mean_tol=1e-9, blk_tol=1e-9):
    """Rows of trajectory b against ref = [(mu3, P33), ...] (ref[k] belongs to logged step trace.first + row)."""
    rows = range(trace.mean.shape[0]) if rows is None else rows
    for r in rows:
        mu3, P33 = ref[trace.first + r]
        err_m = float(np.max(np.abs(trace.mean[r, b] - mu3)))
        err_b = blk_err(trace.cov[r, b], P33)
        print(f"row {trace.first + r} b {b}: mean {err_m:.2e} block {err_b:.2e}")
        assert err_m <= mean_tol and err_b < blk_tol, (trace.first + r, b, err_m, err_b)
        assert np.array_equal(trace.cov[r, b], trace.cov[r, b].T)


def last_row_is_the_filter(f, trace):
    """The trace's last row against the handle: mean()[:3] bit for bit; marginals' pose and the flushed block to 1e-10."""
    for b in range(f.batch):
        assert np.array_equal(trace.mean[-1, b], f.mean(b)[:3])
        assert blk_err(trace.cov[-1, b], f.marginals(b)[0]) < 1e-10
    f.flush()
    for b in range(f.batch):
        assert blk_err(trace.cov[-1, b], f.covariance_block(0, 0, 3, 3, b)) < 1e-10


def oracle_rows(mean0, P0, lin, ang, idx, zr, zb, m, cfg):
    om, oP, rows = mean0.copy(), P0.copy(), []
    for k in range(len(lin)):
        mk = int(m[k])
        om, oP = orc.ekf_step_dense(om, oP, lin[k], ang[k], idx[k][:mk], zr[k][:mk], zb[k][:mk], cfg)
        rows.append((om[:3].copy(), oP[:3, :3].copy()))
    return rows


# ---- per-step kernels -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused_step", [1, 0])
def test_per_step_kernels_against_the_oracle(sd, fused_step):
    """step() on the general kernels, N = 300 x 2: steps with m = 8, steps with m = 0 (k_predict_rc once nothing is pending,
    the generic kernels while ranks are), then a lone predict / update pair: two rows."""
    N, B, steps = 300, 2, 6
    n = 3 + 2 * N
    streams = [orc.synthetic_stream(N, steps, 8, 60 + t) for t in range(B)]
    cfg = orc.EkfConfig()
    none = (np.zeros((B, 0), dtype=np.int32), np.zeros((B, 0)), np.zeros((B, 0)))

    def run(log):
        with sd.EkfSlam(n, batch=B) as f:
            f.set_option("small_state", 0)
            f.set_option("fused_step", fused_step)
            f.profile_enable(True)
            if log:
                f.log_poses(16)
            for b, s in enumerate(streams):
                f.set_state_diag(s[0], s[1], b)
            lin, ang, idx, zr, zb = steps_of(streams, 0)
            f.step(lin, ang, *none)                            # nothing pending: k_predict_rc
            for k in range(steps):
                a = steps_of(streams, k)
                if k == 3:
                    f.step(a[0], a[1], *none)                  # ranks pending: the generic kernels, m = 0
                f.step(*a)
            f.flush()
            passes = f.profile_passes()
            f.step(lin, ang, *none)                            # nothing pending again: k_predict_rc, no rank appended ...
            f.flush()
            assert f.profile_passes() == passes                # ... so there is nothing for a pass to apply
            f.predict(lin, ang)
            f.update(idx, zr, zb)
            assert sd.load_library().ekf_debug_small_launches(f._h) == 0 and f.cadence_counters() == (0, 0)
            trace = f.poses() if log else None
            if log:
                assert f.pose_steps == steps + 5
                last_row_is_the_filter(f, trace)
            return trace, final(sd, f, counters)

    trace, on = run(True)
    _, off = run(False)
    same_bits(on, off)
    assert trace.first == 0 and trace.mean.shape == (steps + 5, B, 3) and trace.cov.shape == (steps + 5, B, 3, 3)
    for b, s in enumerate(streams):
        om, oP, ref = s[0].copy(), np.diag(s[1]), []

        def put():
            ref.append((om[:3].copy(), oP[:3, :3].copy()))
        om, oP = orc.predict_dense(om, oP, s[2][0], s[3][0], cfg); put()
        for k in range(steps):
            if k == 3:
                om, oP = orc.predict_dense(om, oP, s[2][k], s[3][k], cfg); put()
            om, oP = orc.ekf_step_dense(om, oP, s[2][k], s[3][k], s[4][k], s[5][k], s[6][k], cfg); put()
        om, oP = orc.predict_dense(om, oP, s[2][0], s[3][0], cfg); put()
        om, oP = orc.predict_dense(om, oP, s[2][0], s[3][0], cfg); put()
        om, oP = orc.update_dense(om, oP, s[4][0], s[5][0], s[6][0], cfg); put()
        check_rows(trace, b, ref)


def test_update_with_more_than_sixteen_and_thirty_two_landmarks(sd, both_paths):
    """update with m = 20, 38 and 5 (two, three and one pass): ONE row each, the state after the last pass."""
    N = 38
    n = 3 + 2 * N
    rng = np.random.default_rng(21)
    mean0 = np.concatenate([[0.1, -0.2, 0.3], rng.uniform(-2, 2, 2 * N)])
    diag0 = np.concatenate([[0.05, 0.05, 0.01], np.full(2 * N, 0.2)])
    cfg = orc.EkfConfig()
    with sd.EkfSlam(n) as f:
        f.log_poses(8)
        f.set_state_diag(mean0, diag0)
        om, oP, ref = mean0.copy(), np.diag(diag0), []
        for m in (20, 38, 5):
            idx = rng.permutation(N)[:m].astype(np.int32)
            zr, zb = rng.uniform(0.5, 2.0, m), rng.uniform(-1.0, 1.0, m)
            f.update(idx, zr, zb)
            om, oP = orc.update_dense(om, oP, idx, zr, zb, cfg)
            ref.append((om[:3].copy(), oP[:3, :3].copy()))
        assert path_ran(f, both_paths)
        trace = f.poses()
        assert f.pose_steps == 3 and trace.mean.shape[0] == 3
        check_rows(trace, 0, ref)
        last_row_is_the_filter(f, trace)


def test_small_state_steps_and_stream(sd, both_paths):
    """N = 20: step() / step_state() alternately, then the same stream as run_stream (the small-state path: one launch)."""
    N, steps = 20, 6
    n = 3 + 2 * N
    s = orc.synthetic_stream(N, steps, 8, 5)
    cfg = orc.EkfConfig()
    ref = oracle_rows(s[0], np.diag(s[1]), s[2], s[3], s[4], s[5], s[6], np.full(steps, 8), cfg)

    def run(log, stream):
        with sd.EkfSlam(n) as f:
            if log:
                f.log_poses(8)
            f.set_state_diag(s[0], s[1])
            if stream:
                f.run_stream(s[2], s[3], s[4], s[5], s[6])
            else:
                for k in range(steps):
                    (f.step_state if k % 2 else f.step)(s[2][k], s[3][k], s[4][k], s[5][k], s[6][k])
            assert path_ran(f, both_paths)
            trace = f.poses() if log else None
            if log:
                last_row_is_the_filter(f, trace)
            return trace, final(sd, f, counters)

    for stream in (False, True):
        trace, on = run(True, stream)
        _, off = run(False, stream)
        same_bits(on, off)
        assert trace.first == 0 and trace.mean.shape[0] == steps
        check_rows(trace, 0, ref)
    # a ring smaller than the launch's steps, the stream in two pieces: the last four rows, numbered on
    with sd.EkfSlam(n) as f:
        f.log_poses(4)
        f.set_state_diag(s[0], s[1])
        f.stream_upload(s[2], s[3], s[4], s[5], s[6])
        f.stream_run(0, 1)
        f.stream_run(1, steps - 1)
        assert path_ran(f, both_paths)
        short = f.poses()
        assert f.pose_steps == steps and short.first == steps - 4 and short.mean.shape[0] == 4
        check_rows(short, 0, ref)
        last_row_is_the_filter(f, short)


# ---- fused cadences --------------------------------------------------------------------------------------------------------
def packing(m, slots=SLOTS):
    """(steps cut by a cadence boundary, cadences) of one trajectory under the documented packing: whole steps while they fit
    `slots` landmark updates, then as many landmarks of the next step as still fit.  The cadence count is checked against
    the handle's, so that a planner that packs otherwise fails the test instead of emptying the cut-step assertion."""
    cuts, cads, used = 0, 1, 0
    for mk in m:
        left = int(mk)
        while used + left > slots:
            room = slots - used
            if room > 0:
                cuts += 1
                left -= room
            cads += 1
            used = 0
        used += left
    return cuts, cads


@pytest.mark.parametrize("chain", [1, 0])
def test_packed_cadences_on_a_variable_m_stream(sd, chain):
    """m ~ uniform{0..8} per step and trajectory, N = 150 x 3, 40 steps as packed cadences: steps cut by a cadence boundary,
    steps observing nothing, chained or look-ahead / plain solves; then with a ring smaller than one cadence's steps."""
    N, B, steps = 150, 3, 40
    n = 3 + 2 * N
    means, lin, ang, idx, zr, zb, m = variable_bank(N, B, steps, 8, 4208)
    starts = [dense_start(n, 4300 + t) for t in range(B)]
    packs = [packing(m[:, b]) for b in range(B)]
    assert sum(p[0] for p in packs) > 0 and (m == 0).any()

    def run(log):
        with sd.EkfSlam(n, batch=B) as f:
            f.set_option("active_bound", 0)
            f.set_option("chain", chain)
            f.set_option("rank_limit", 2 * SLOTS)
            f.profile_enable(True)
            if log:
                f.log_poses(log)
            for b in range(B):
                f.set_state(means[b], starts[b], b)
            f.run_stream(lin, ang, idx, zr, zb, m)
            trace = f.poses() if log else None
            if log:
                assert f.pose_steps == steps
                last_row_is_the_filter(f, trace)
            return trace, final(sd, f, counters)

    trace, on = run(steps)
    _, off = run(0)
    same_bits(on, off)
    assert on[2][0] == max(p[1] for p in packs) and on[2][1] == steps   # fused cadences ran the whole stream, cut as restated
    assert (on[2].chained > 0) == bool(chain)
    short, on3 = run(3)                                         # cap below one cadence's steps: the last three rows
    same_bits(on3, off)
    assert short.first == steps - 3 and short.mean.shape[0] == 3
    cfg = orc.EkfConfig()
    for b in range(B):
        ref = oracle_rows(means[b], starts[b], lin[:, b], ang[:, b], idx[:, b], zr[:, b], zb[:, b], m[:, b], cfg)
        check_rows(trace, b, ref)
        check_rows(short, b, ref)


@pytest.mark.parametrize("run_end_flush", [0, 1])
def test_stream_pieces_ending_mid_cadence(sd, run_end_flush):
    """stream_run in pieces whose ends fall inside a cadence (m = 7: 40 slots end inside a step), N = 300 x 1, with a step()
    between two pieces: row numbering continues across pieces and calls."""
    N, steps, m = 300, 22, 7
    n = 3 + 2 * N
    s = orc.synthetic_stream(N, steps, m, 77)
    P0 = dense_start(n, 9)
    args = tuple(np.asarray(a)[:, None] for a in (s[2], s[3], s[4], s[5], s[6]))
    cfg = orc.EkfConfig()

    def run(log):
        with sd.EkfSlam(n) as f:
            f.set_option("run_end_flush", run_end_flush)
            f.profile_enable(True)
            if log:
                f.log_poses(64)
            f.set_state(s[0], P0)
            f.stream_upload(*args)
            f.stream_run(0, 7)
            f.stream_run(7, 6)
            f.step(s[2][0], s[3][0], s[4][0], s[5][0], s[6][0])
            f.stream_run(13, 9)
            trace = f.poses() if log else None
            if log:
                assert f.pose_steps == steps + 1
                last_row_is_the_filter(f, trace)
            return trace, final(sd, f, counters)

    trace, on = run(True)
    _, off = run(False)
    same_bits(on, off)
    assert on[2][0] > 0
    om, oP, ref = s[0].copy(), P0.copy(), []
    order = list(range(13)) + [0] + list(range(13, steps))
    for k in order:
        om, oP = orc.ekf_step_dense(om, oP, s[2][k], s[3][k], s[4][k], s[5][k], s[6][k], cfg)
        ref.append((om[:3].copy(), oP[:3, :3].copy()))
    check_rows(trace, 0, ref)


@pytest.mark.parametrize("N,B,steps,opts,what", [(2000, 1, 30, (), "chained"), (2000, 1, 30, (("chain", 0), ("active_bound", 0)), "lookahead"),
                                                 (2000, 32, 25, (("active_bound", 0),), "w_from_v"), (8000, 1, 12, (("active_bound", 1),), "bound")])
def test_large_banks_against_the_per_step_kernels(sd, N, B, steps, opts, what):
    """Sizes the dense oracle cannot afford, m = 8: the fused run's trace against the trace of the same stream on the
    per-step kernels (step() in a loop).  N = 2000 x 1 chained; the same with chain = 0 (the look-ahead solve beside the
    pass); 32 x N = 2000 (the row-slab pass with W formed from V); N = 8000 x 1 with the active bound (column panels)."""
    n = 3 + 2 * N
    streams = [orc.synthetic_stream(N, steps, 8, 500 + t) for t in range(B)]
    args = tuple(np.stack([s[i] for s in streams], axis=1) for i in (2, 3, 4, 5, 6))

    def run(log, fused):
        with sd.EkfSlam(n, batch=B) as f:
            for name, v in opts:
                f.set_option(name, v)
            f.profile_enable(True)
            if log:
                f.log_poses(steps)
            for b, s in enumerate(streams):
                f.set_state_diag(s[0], s[1], b)
            if fused:
                f.run_stream(*args)
            else:
                for k in range(steps):
                    f.step(*steps_of(streams, k))
            res = (f.poses() if log else None), [f.mean(b) for b in range(B)], [f.flags(b) for b in range(B)], counters(sd, f)
            if log:
                last_row_is_the_filter(f, res[0])
            return res

    fused, plain, ref = run(True, True), run(False, True), run(True, False)
    for a, b in zip(fused[1], plain[1]):
        assert np.array_equal(a, b)
    assert fused[2] == plain[2] and fused[3] == plain[3]
    cnt = fused[3]
    assert cnt[0] > 0 and cnt[1] == steps and ref[3][0] == 0 and ref[3][2] == 0
    if what == "chained":
        assert cnt[2] > 0
    elif what == "lookahead":
        assert cnt[2] == 0 and cnt[3] > 0
    elif what == "w_from_v":
        assert cnt[7] > 0 and "k_flush_rs" in cnt[8]
    else:
        assert (fused[1][0][3 + 2 * 8 * steps:] == streams[0][0][3 + 2 * 8 * steps:]).all()   # beyond the bound: untouched
    for b in range(B):
        rows = [(ref[0].mean[k, b], ref[0].cov[k, b]) for k in range(steps)]
        check_rows(fused[0], b, rows, mean_tol=PATH_CORR_TOL, blk_tol=PATH_CORR_TOL)


# ---- the NIS gate, the noise bank, the device-side association ---------------------------------------------------------------
def _outliers(zr, m, seed, first=5, every=4):
    """Range + 20 m at seeded (step, trajectory, landmark) positions; returns the new ranges and the number per trajectory."""
    zr = np.array(zr, dtype=float)
    rng = np.random.default_rng(seed)
    count = np.zeros(m.shape[1], dtype=int)
    for k in range(first, m.shape[0], every):
        for b in range(m.shape[1]):
            if m[k, b] > 0 and rng.random() < 0.7:
                zr[k, b, int(rng.integers(0, m[k, b]))] += 20.0
                count[b] += 1
    return zr, count


@pytest.mark.parametrize("chain", [1, 0])
def test_packed_cadences_with_the_gate_and_a_noise_bank(sd, chain):
    """Packed cadences, N = 150 x 3, variable m, outliers in the stream, the NIS gate on and a distinct noise row per
    trajectory (k_solve_cad_plog's GATE and NZ instantiations, a rejected last landmark included): rows against the oracle
    run with the same gate and each trajectory's own noise."""
    N, B, steps = 150, 3, 40
    n = 3 + 2 * N
    means, lin, ang, idx, zr, zb, m = variable_bank(N, B, steps, 8, 5208)
    zr, injected = _outliers(zr, m, 17)
    last = int(np.max(np.nonzero(m[:, 0])[0]))                 # trajectory 0's last observing step: reject its LAST landmark
    zr[last, 0, m[last, 0] - 1] += 20.0
    starts = [dense_start(n, 5300 + t) for t in range(B)]
    ms, qs = np.array([0.1, 0.05, 0.2]), np.array([1.0, 0.5, 1.4])
    base = orc.EkfConfig()
    ms[0], qs[0] = base.motion_sigma, base.meas_sigma

    def run(log, gate, noise):
        with sd.EkfSlam(n, batch=B) as f:
            f.set_option("active_bound", 0)
            f.set_option("chain", chain)
            f.profile_enable(True)
            if gate:
                f.set_nis_gate(G)
            if noise:
                f.set_noise(ms, qs)
            if log:
                f.log_poses(steps)
            for b in range(B):
                f.set_state(means[b], starts[b], b)
            f.run_stream(lin, ang, idx, zr, zb, m)
            trace = f.poses() if log else None
            rejected = f.gate_counts().tolist() if gate else None
            if log:
                last_row_is_the_filter(f, trace)
            return trace, rejected, final(sd, f, counters)

    for gate, noise in ((True, True), (True, False), (False, True)):
        trace, rejected, on = run(True, gate, noise)
        _, rejected_off, off = run(False, gate, noise)
        same_bits(on, off)
        assert rejected == rejected_off and on[2][0] > 1 and on[2][1] == steps
        for b in range(B):
            cfg = orc.EkfConfig(motion_sigma=float(ms[b]), meas_sigma=float(qs[b])) if noise else base
            om, oP, ref, nrej = means[b].copy(), starts[b].copy(), [], 0
            for k in range(steps):
                mb = int(m[k, b])
                om, oP, r = gated_step_count(om, oP, lin[k, b], ang[k, b], idx[k, b, :mb], zr[k, b, :mb], zb[k, b, :mb], cfg,
                                             G if gate else np.inf)
                nrej += r
                ref.append((om[:3].copy(), oP[:3, :3].copy()))
            if gate:
                assert rejected[b] == nrej and nrej >= injected[b] > 0
            check_rows(trace, b, ref)


def test_small_state_with_the_gate_and_a_noise_bank(sd, both_paths):
    """N = 20 x 3, step() then run_stream with outliers, the gate on and a noise row per trajectory (the small-state
    kernels' NZ forms with the pose log): rows against the gated oracle under each trajectory's noise."""
    N, B, steps = 20, 3, 14
    n = 3 + 2 * N
    means, lin, ang, idx, zr, zb, m = variable_bank(N, B, steps, 8, 6100)
    zr, injected = _outliers(zr, m, 3, first=2, every=3)
    starts = [dense_start(n, 6200 + t) for t in range(B)]
    ms, qs = np.array([0.1, 0.05, 0.2]), np.array([1.0, 0.5, 1.4])

    def run(log):
        with sd.EkfSlam(n, batch=B) as f:
            f.set_nis_gate(G)
            f.set_noise(ms, qs)
            if log:
                f.log_poses(steps)
            for b in range(B):
                f.set_state(means[b], starts[b], b)
            for k in range(4):
                f.step(lin[k], ang[k], *([a[k, b, :m[k, b]] for b in range(B)] for a in (idx, zr, zb)))
            f.stream_upload(lin, ang, idx, zr, zb, m)
            f.stream_run(4, steps - 4)
            assert path_ran(f, both_paths)
            trace = f.poses() if log else None
            rejected = f.gate_counts().tolist()
            if log:
                last_row_is_the_filter(f, trace)
            return trace, rejected, final(sd, f, counters)

    trace, rejected, on = run(True)
    _, rejected_off, off = run(False)
    same_bits(on, off)
    assert rejected == rejected_off and sum(rejected) > 0
    for b in range(B):
        cfg = orc.EkfConfig(motion_sigma=float(ms[b]), meas_sigma=float(qs[b]))
        om, oP, ref, nrej = means[b].copy(), starts[b].copy(), [], 0
        for k in range(steps):
            mb = int(m[k, b])
            om, oP, r = gated_step_count(om, oP, lin[k, b], ang[k, b], idx[k, b, :mb], zr[k, b, :mb], zb[k, b, :mb], cfg, G)
            nrej += r
            ref.append((om[:3].copy(), oP[:3, :3].copy()))
        assert rejected[b] == nrej
        check_rows(trace, b, ref)


def test_step_detections_with_more_than_sixteen_tags(sd, both_paths):
    """ekf_step_detections with 20 distinct tags in a window (two update passes: ONE row), then 20 again and 6: rows against
    the oracle's association + augmentation + step, on both paths."""
    rng = np.random.default_rng(8)
    cfg = orc.EkfConfig()
    ids = [int(i) for i in rng.permutation(200)[:24]]
    bx = {i: float(rng.uniform(-0.5, 0.5)) for i in ids}
    bz = {i: float(rng.uniform(0.4, 1.1)) for i in ids}
    plan = [(ids[:20], 0.004, 0.02), (ids[4:24], 0.004, 0.005), (ids[:6], 0.003, 0.02)]
    wins = [[(k + 0.1 * fr, [tag(i, bx[i] + rng.normal(0, 0.004), bz[i] + rng.normal(0, 0.004)) for i in win_ids])
             for fr in range(3)] for k, (win_ids, _, _) in enumerate(plan)]

    def run(log):
        with sd.EkfSlam(3 + 2 * 30) as f:
            if log:
                f.log_poses(8)
            for (_, lin, ang), win in zip(plan, wins):
                f.step_detections(lin, ang, win)
            assert path_ran(f, both_paths) and f.assoc_fallbacks() == 0
            trace = f.poses() if log else None
            if log:
                assert f.pose_steps == len(plan)
                last_row_is_the_filter(f, trace)
            return trace, final(sd, f, counters)

    trace, on = run(True)
    _, off = run(False)
    same_bits(on, off)
    om, oP, oti, ref = np.zeros(3), np.eye(3) * 0.1, {}, []
    for (_, lin, ang), win in zip(plan, wins):
        tags = orc.associate(win, oti, om, cfg)
        om, oP = orc.augment(om, oP, len(oti), tags, cfg)
        order = list(tags.keys())
        om, oP = orc.ekf_step_dense(om, oP, lin, ang, order, [tags[i][4] for i in order], [tags[i][5] for i in order], cfg)
        ref.append((om[:3].copy(), oP[:3, :3].copy()))
    check_rows(trace, 0, ref)


# ---- the ring, the counters, both logs ---------------------------------------------------------------------------------------
def test_ring_wrap_mixed_calls_and_refused_ranges(sd):
    """capacity 5 for 3 step() + 12 stream steps + 1 predict on N = 300: the last five rows, refused ranges, log off."""
    N, steps = 300, 12
    n = 3 + 2 * N
    s = orc.synthetic_stream(N, steps, 8, 31)
    cfg = orc.EkfConfig()
    lib = sd.load_library()
    with sd.EkfSlam(n) as f:
        with pytest.raises(sd.EkfError):
            f.poses()
        assert lib.ekf_download_poses(f._h, 0, 0, None, None) == EKF_ERR_STATE
        f.log_poses(5)
        f.set_state_diag(s[0], s[1])
        om, oP, ref = s[0].copy(), np.diag(s[1]), []
        for k in list(range(3)) + list(range(steps)):
            om, oP = orc.ekf_step_dense(om, oP, s[2][k], s[3][k], s[4][k], s[5][k], s[6][k], cfg)
            ref.append((om[:3].copy(), oP[:3, :3].copy()))
        om, oP = orc.predict_dense(om, oP, 0.01, 0.02, cfg)
        ref.append((om[:3].copy(), oP[:3, :3].copy()))
        for k in range(3):
            f.step(s[2][k], s[3][k], s[4][k], s[5][k], s[6][k])
        f.run_stream(*(np.asarray(a)[:, None] for a in (s[2], s[3], s[4], s[5], s[6])))
        f.predict(np.array([0.01]), np.array([0.02]))
        assert f.pose_steps == 16
        trace = f.poses()
        assert trace.first == 11 and trace.mean.shape[0] == 5
        check_rows(trace, 0, ref)
        two = f.poses(13, 2)
        assert two.first == 13 and np.array_equal(two.mean, trace.mean[2:4]) and np.array_equal(two.cov, trace.cov[2:4])
        buf, cov = np.zeros(3 * 6), np.zeros(9 * 6)
        dp = C.POINTER(C.c_double)
        for first, count in ((10, 2), (15, 2), (-1, 1), (12, -1)):
            assert lib.ekf_download_poses(f._h, first, count, buf.ctypes.data_as(dp), cov.ctypes.data_as(dp)) == EKF_ERR_ARG
        assert lib.ekf_download_poses(f._h, 12, 2, buf.ctypes.data_as(dp), None) == 0      # cov may be NULL
        assert np.array_equal(buf[:6].reshape(2, 3), trace.mean[1:3, 0])
        last_row_is_the_filter(f, trace)
        f.log_poses(0)
        assert lib.ekf_download_poses(f._h, 0, 0, None, None) == EKF_ERR_STATE


def test_both_logs_together_equal_each_alone(sd):
    """The innovation log and the pose log on together, packed cadences N = 150 x 2: each equals what it gives alone."""
    N, B, steps = 150, 2, 24
    n = 3 + 2 * N
    means, lin, ang, idx, zr, zb, m = variable_bank(N, B, steps, 8, 77)
    starts = [dense_start(n, 500 + t) for t in range(B)]

    def run(innov, pose):
        with sd.EkfSlam(n, batch=B) as f:
            f.profile_enable(True)
            if innov:
                f.log_innovations(steps + 1)
            if pose:
                f.log_poses(steps + 1)
            for b in range(B):
                f.set_state(means[b], starts[b], b)
            f.predict(lin[0], ang[0])                          # a row of the pose log, no step of the innovation log
            f.run_stream(lin, ang, idx, zr, zb, m)
            return (f.innovations() if innov else None), (f.poses() if pose else None), final(sd, f, counters)

    i2, p2, both = run(True, True)
    i1, _, a = run(True, False)
    _, p1, b_ = run(False, True)
    same_bits(both, a)
    same_bits(both, b_)
    assert len(i2.steps) == steps and p2.mean.shape[0] == steps + 1
    assert np.array_equal(p1.mean, p2.mean) and np.array_equal(p1.cov, p2.cov)
    for x, y in zip(i1, i2):
        assert np.array_equal(x, y, equal_nan=True)


def test_trajectory_ate_from_the_trace_equals_the_step_by_step_run(sd):
    """A bank of 4 on one truth path: run_stream + one poses() call gives the ATE that step() + mean() after every step gives."""
    from slam_duckietown_amd.evaluation import ate_rmse, trajectory_ate
    N, B, steps = 150, 4, 30
    n = 3 + 2 * N
    means, lin, ang, idx, zr, zb, m = variable_bank(N, B, steps, 8, 901)
    cfg = orc.EkfConfig()
    pose, truth = np.zeros(3), []
    for k in range(steps):
        pose, _ = orc.motion_model(pose, lin[k, 0], ang[k, 0], cfg)
        truth.append(pose[:2].copy())
    truth = np.array(truth)
    diag = np.concatenate([[0.01, 0.01, 0.01], np.full(2 * N, 0.3)])
    with sd.EkfSlam(n, batch=B) as f:
        f.log_poses(steps)
        for b in range(B):
            f.set_state_diag(means[b], diag, b)
        f.run_stream(lin, ang, idx, zr, zb, m)
        got = trajectory_ate(f.poses(), truth)
    with sd.EkfSlam(n, batch=B) as f:
        for b in range(B):
            f.set_state_diag(means[b], diag, b)
        path = []
        for k in range(steps):
            f.step(lin[k], ang[k], *([a[k, b, :m[k, b]] for b in range(B)] for a in (idx, zr, zb)))
            path.append([f.mean(b)[:2] for b in range(B)])
    path = np.array(path)
    want = np.array([ate_rmse(path[:, b], truth) for b in range(B)])
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-9)
