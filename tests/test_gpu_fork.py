"""GPU: device-side forks (ekf_copy_trajectories, EkfSlam.fork / copy_from; k_copy_traj in csrc/ekf_copy.hip).

A copy is exact and moves stored values only: every case compares mean and covariance bit for bit with the download of the
source taken just before, then, where the filters go on, twins with each other bit for bit and with the oracle run from that
download.  Each case names the path that ran (path_ran, cadence_counters / ekf_debug_chained, last_pass)."""
import ctypes as C

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests import fork_model as fm
from tests.conftest import path_ran
from tests.gated_oracle import gated_step
from tests.gpu_support import raw00, same, sd, tag  # noqa: F401

pytestmark = pytest.mark.gpu

TIGHT = 1e-10          # the project's bar for a run against the oracle (tests/test_gpu_remove_landmarks.py)
ORDER = 1e-11          # what the header guarantees between orders of summation
EKF_ERR_ARG = -1
FUZZ_RUNS = 4          # interleavings of the seeded soak (test_seeded_fuzz_against_the_model)
FUZZ_OPS = 24


def bank(x, B):
    """One trajectory's stream array [steps, ...] as a bank's [steps, B, ...]: every column the same."""
    return np.repeat(x[:, None], B, 1)


def run_columns(f, lin, ang, idx, zr, zb, k0, k1):
    B = f.batch
    f.stream_upload(bank(lin[k0:k1], B), bank(ang[k0:k1], B), bank(idx[k0:k1], B), bank(zr[k0:k1], B), bank(zb[k0:k1], B))
    f.stream_run(0, k1 - k0)


def oracle_run(state, lin, ang, idx, zr, zb, cfg=None):
    cfg = cfg or orc.EkfConfig()
    om, oP = state
    for k in range(len(lin)):
        om, oP = orc.ekf_step_structured(om, oP, lin[k], ang[k], idx[k], zr[k], zb[k], cfg)
    return om, oP


def mapped_bank(sd, N, B, m, steps, total, seed):
    """A bank of B trajectories with distinct starts after `steps` steps of one synthetic stream (of `total` steps)."""
    s = orc.synthetic_stream(N, total, m, seed)
    f = sd.EkfSlam(3 + 2 * N, batch=B)
    for b in range(B):
        f.set_state_diag(s[0] + 0.01 * b, s[1], b)
    run_columns(f, *s[2:], 0, steps)
    return f, s


# ---- 1-3: a bank of N = 500 -----------------------------------------------------------------------------------------------
def forked_500(sd):
    f, s = mapped_bank(sd, 500, 4, 7, 60, 140, 3)
    assert f.cadence_counters()[0] > 0 and path_ran(f, "general_kernels")
    pending = raw00(sd, f)
    before = f.state(0)
    assert pending != before[1][0, 0]                              # the download applied ranks that were pending
    assert not same(f.state(1), before)
    return f, s, before


def test_bit_exact_with_ranks_pending(sd):
    """N = 500 x 4, 60 stream steps of 7 landmarks (packed cadences of 40 updates: the last one's ranks stay pending)."""
    lib = sd.load_library()
    with sd.EkfSlam(3 + 2 * 500, batch=4) as f:
        s = orc.synthetic_stream(500, 60, 7, 3)
        for b in range(4):
            f.set_state_diag(s[0] + 0.01 * b, s[1], b)
        run_columns(f, *s[2:], 0, 60)
        assert f.cadence_counters()[0] > 0 and path_ran(f, "general_kernels")
        print("case 1: cadences", f.cadence_counters(), "chained", lib.ekf_debug_chained(f._h), "pass", f.last_pass())
        pending = raw00(sd, f)
        f2, _ = mapped_bank(sd, 500, 4, 7, 60, 60, 3)             # the same run: its download is what the fork must give
        with f2:
            before = f2.state(0)
        assert pending != before[1][0, 0]                          # ranks are pending when the fork is called
        f.fork(0)
        for b in range(4):
            assert same(f.state(b), before), b
            assert f.size(b) == 3 + 2 * 500 and f.flags(b) == 0


def test_twins_stay_twins(sd):
    lib = sd.load_library()
    f, s, before = forked_500(sd)
    with f:
        f.fork(0)
        cad0, ch0 = f.cadence_counters()[0], lib.ekf_debug_chained(f._h)
        run_columns(f, *s[2:], 60, 140)
        got = [f.state(b) for b in range(4)]
        cad, ch = f.cadence_counters()[0] - cad0, lib.ekf_debug_chained(f._h) - ch0
        print("case 2: cadences", cad, "chained", ch, "pass", f.last_pass())
        assert cad > 0 and path_ran(f, "general_kernels")
        assert ch > 0                                              # 4 x N = 500 chains its solves: the twins ran chained cadences
        assert all(f.flags(b) == 0 for b in range(4))
    for b in range(1, 4):
        assert same(got[b], got[0]), b
    om, oP = oracle_run(before, *[a[60:140] for a in s[2:]])
    assert orc.rel_fro(got[0][0], om) < TIGHT and orc.rel_fro(got[0][1], oP) < TIGHT


def test_fork_equals_download_and_upload(sd):
    f, s, before = forked_500(sd)
    with f, sd.EkfSlam(3 + 2 * 500, batch=4) as g:
        f.fork(0)
        for b in range(4):
            g.set_state(*before, b)
        for b in range(4):
            assert same(f.state(b), g.state(b))
        run_columns(f, *s[2:], 60, 140)
        run_columns(g, *s[2:], 60, 140)
        assert f.cadence_counters()[0] > 0 and g.cadence_counters()[0] > 0
        for b in range(4):
            (mf, Pf), (mg, Pg) = f.state(b), g.state(b)
            assert orc.rel_fro(mf, mg) < ORDER and orc.rel_fro(Pf, Pg) < ORDER, b


# ---- 4: small states --------------------------------------------------------------------------------------------------------
def test_small_state_both_paths(sd, both_paths):
    f, s = mapped_bank(sd, 20, 8, 6, 25, 55, 4)
    with f:
        assert path_ran(f, both_paths)
        before = f.state(0)
        assert not same(f.state(5), before)
        f.fork(0)
        for b in range(8):
            assert same(f.state(b), before) and f.flags(b) == 0
        run_columns(f, *s[2:], 25, 55)
        got = [f.state(b) for b in range(8)]
        assert path_ran(f, both_paths)
    for b in range(1, 8):
        assert same(got[b], got[0]), b
    om, oP = oracle_run(before, *[a[25:55] for a in s[2:]])
    assert orc.rel_fro(got[0][0], om) < TIGHT and orc.rel_fro(got[0][1], oP) < TIGHT


# ---- 5, 6: handles, layouts, column panels ------------------------------------------------------------------------------------
def test_across_handles_and_layouts(sd):
    """ld = 1024 -> ld = 2048 (a bank) and -> column panels (n_max = 4203)."""
    N = 500
    s = orc.synthetic_stream(N, 31, 8, 5)
    big = orc.synthetic_stream(700, 1, 8, 6)
    with sd.EkfSlam(3 + 2 * N) as src, sd.EkfSlam(3 + 2 * 700, batch=2) as mid, sd.EkfSlam(3 + 2 * 2100) as wide:
        src.set_state_diag(s[0], s[1])
        run_columns(src, *s[2:], 0, 30)
        assert src.cadence_counters()[0] > 0
        before = src.state()
        # the other direction first: a state that does not fit changes nothing
        mid.set_state_diag(big[0], big[1], 0)
        with pytest.raises(sd.EkfError, match="n_max"):
            src.copy_from(mid, 0, 0)
        assert sd.load_library().ekf_copy_trajectories(src._h, (C.c_int * 1)(0), mid._h, (C.c_int * 1)(0), 1) == EKF_ERR_ARG
        assert same(src.state(), before) and src.size() == 3 + 2 * N
        mid.copy_from(src, [0, 0], [0, 1])
        wide.copy_from(src)
        for h, bs in ((mid, (0, 1)), (wide, (0,))):
            for b in bs:
                assert h.size(b) == 3 + 2 * N and same(h.state(b), before) and h.flags(b) == 0
        k = 30
        src.step(s[2][k], s[3][k], s[4][k], s[5][k], s[6][k])
        want = src.state()
        obs = [s[4][k]] * 2, [s[5][k]] * 2, [s[6][k]] * 2
        mid.step(s[2][k], s[3][k], *obs)
        wide.step(s[2][k], s[3][k], s[4][k], s[5][k], s[6][k])
        for h, bs in ((mid, (0, 1)), (wide, (0,))):
            for b in bs:
                mu, P = h.state(b)
                assert orc.rel_fro(mu, want[0]) < ORDER and orc.rel_fro(P, want[1]) < ORDER
    om, oP = oracle_run(before, *[a[30:31] for a in s[2:]])
    assert orc.rel_fro(want[0], om) < TIGHT and orc.rel_fro(want[1], oP) < TIGHT


def test_across_the_panel_boundary_at_size(sd):
    """N = 2100 x 2: rows and ld = 4224, two column panels; columns beyond 4096 correlated with the rest."""
    N = 2100
    n = 3 + 2 * N
    rng = np.random.default_rng(5)
    A = rng.normal(size=(n, 4)) * 0.2
    P0 = A @ A.T + np.diag(rng.uniform(0.5, 2.0, n))
    s = orc.synthetic_stream(N, 6, 8, 5)
    with sd.EkfSlam(n, batch=2) as f:
        f.set_state(s[0], P0, 0)
        f.set_state_diag(s[0] + 0.01, s[1], 1)
        run_columns(f, *s[2:], 0, 6)
        assert "k_flush" in f.last_pass()
        print("case 6: pass", f.last_pass())
        before = f.state(0)
        assert np.abs(before[1][10:14, 4090:4102]).min() > 0.0
        f.fork(0, 1)
        assert same(f.state(1), before) and f.flags(1) == 0 and f.size(1) == n
        blk = f.covariance_block(10, 4090, 4, 12, b=1)             # straddles column 4096
        assert np.array_equal(blk, before[1][10:14, 4090:4102])
        assert np.array_equal(f.covariance_block(4090, 4090, 12, 12, b=1), before[1][4090:4102, 4090:4102])


# ---- 7: the device association ---------------------------------------------------------------------------------------------


def test_device_association_follows_the_state(sd):
    rng = np.random.default_rng(21)
    ids = [int(i) for i in rng.permutation(500)[:11]]
    bx = {i: float(rng.uniform(-0.5, 0.5)) for i in ids}
    bz = {i: float(rng.uniform(0.4, 1.1)) for i in ids}

    def window(k, win_ids):
        return [(k + 0.1 * fr, [tag(i, bx[i] + rng.normal(0, 0.004), bz[i] + rng.normal(0, 0.004)) for i in win_ids])
                for fr in range(2)]

    lib = sd.load_library()
    with sd.EkfSlam(3 + 2 * 30, batch=2) as f:
        for k, w in enumerate([ids[:6], ids[2:9], ids[:4]]):
            f.step_detections(0.004, 0.02, [window(k, w), window(k, w[:3])])    # slot 1 maps fewer tags, in another order
        assert f.assoc_fallbacks() == 0 and path_ran(f, "default_path")
        assert f.tag_index(0) != f.tag_index(1) and f.size(0) != f.size(1)
        before, index, tags = f.state(0), f.tag_index(0), f.tags_positions(0)
        f.fork(0, 1)
        assert same(f.state(1), before) and f.size(1) == f.size(0)
        assert f.tag_index(1) == index and f.tag_index(0) == index

        def raw_tags(b):
            m = C.c_int()
            ii, tt = np.zeros(32, np.int32), np.zeros(32, np.int32)
            arrs = [np.zeros(32) for _ in range(5)]
            assert lib.ekf_download_tags(f._h, b, C.byref(m), ii.ctypes.data_as(C.POINTER(C.c_int)),
                                         tt.ctypes.data_as(C.POINTER(C.c_int)),
                                         *[a.ctypes.data_as(C.POINTER(C.c_double)) for a in arrs]) == 0
            return [m.value, ii.tolist(), tt.tolist()] + [a.tolist() for a in arrs]

        assert raw_tags(1) == raw_tags(0) and f.tags_positions(1) == tags
        win = window(9, ids[5:11])                                 # ids[9], ids[10] are new to both
        f.step_detections(0.003, 0.01, [win, win])
        assert same(f.state(1), f.state(0)) and f.size(0) == 3 + 2 * 11
        assert f.tag_index(1) == f.tag_index(0) and f.tag_index(1)[ids[10]] == 10
        assert f.tags_positions(1) == f.tags_positions(0)
        assert f.flags(0) == 0 and f.flags(1) == 0 and f.assoc_fallbacks() == 0


# ---- 8: what belongs to the slot stays --------------------------------------------------------------------------------------
def test_slot_properties_stay(sd):
    """A noise bank, the gate and both logs on: a fork changes none of them, and twins under different noise rows then
    diverge, each as the oracle does under its own pair -- the tune_noise(start=...) contract."""
    N, B, g = 150, 3, 25.0
    s = orc.synthetic_stream(N, 60, 8, 8)
    ms, qs = np.array([0.1, 0.05, 0.2]), np.array([0.7, 0.4, 1.1])
    with sd.EkfSlam(3 + 2 * N, batch=B) as f:
        f.set_noise(ms, qs)
        f.set_nis_gate(g)
        f.log_innovations(64)
        f.log_poses(64)
        for b in range(B):
            f.set_state_diag(s[0] + 0.01 * b, s[1], b)
        run_columns(f, *s[2:], 0, 30)
        assert f.cadence_counters()[0] > 0 and path_ran(f, "general_kernels")
        before = f.state(0)
        noise, counts, innov, poses = f.noise(), f.gate_counts(), f.innovations(), f.poses()
        f.fork(0)
        assert np.array_equal(f.noise()[0], ms) and np.array_equal(f.noise()[1], qs)
        assert np.array_equal(f.noise()[0], noise[0]) and np.array_equal(f.gate_counts(), counts)
        i2, p2 = f.innovations(), f.poses()
        assert i2.steps.tolist() == innov.steps.tolist() == list(range(30)) and f.pose_steps == 30
        for a, b in zip(innov[1:], i2[1:]):
            assert np.array_equal(a, b, equal_nan=True)
        assert np.array_equal(p2.mean, poses.mean) and np.array_equal(p2.cov, poses.cov)
        for b in range(B):
            assert same(f.state(b), before)
        run_columns(f, *s[2:], 30, 60)
        got = [f.state(b) for b in range(B)]
        assert f.innovations().steps.shape[0] == 60
    assert not same(got[0], got[1]) and not same(got[0], got[2])
    for b in range(B):
        cfg = orc.EkfConfig(motion_sigma=float(ms[b]), meas_sigma=float(qs[b]))
        om, oP = before
        for k in range(30, 60):
            om, oP = gated_step(om, oP, s[2][k], s[3][k], s[4][k], s[5][k], s[6][k], cfg, g)[:2]
        assert orc.rel_fro(got[b][0], om) < TIGHT and orc.rel_fro(got[b][1], oP) < TIGHT, b


# ---- 9: a spare handle as the fallback ---------------------------------------------------------------------------------------
def test_fallback_from_a_spare_handle(sd):
    N = 150
    s = orc.synthetic_stream(N, 40, 8, 9)
    with sd.EkfSlam(3 + 2 * N) as f, sd.EkfSlam(3 + 2 * N) as spare:
        f.set_state_diag(s[0], s[1])
        for k in range(20):
            f.step(s[2][k], s[3][k], s[4][k], s[5][k], s[6][k])
        assert path_ran(f, "general_kernels")
        spare.copy_from(f)
        parked = f.state()
        assert same(spare.state(), parked)
        k = 20
        f.step(s[2][k], s[3][k], s[4][k], s[5][k] + 5.0, s[6][k])  # a window with gross outliers
        assert not same(f.state(), parked)
        f.copy_from(spare)
        assert same(f.state(), parked) and f.flags() == 0
        for k in range(20, 40):
            f.step(s[2][k], s[3][k], s[4][k], s[5][k], s[6][k])
        got = f.state()
        assert same(spare.state(), parked)
    om, oP = oracle_run(parked, *[a[20:40] for a in s[2:]])
    assert orc.rel_fro(got[0], om) < TIGHT and orc.rel_fro(got[1], oP) < TIGHT


# ---- 10: errors --------------------------------------------------------------------------------------------------------------
def test_bad_arguments_change_nothing(sd):
    N, B = 60, 4
    lib = sd.load_library()
    f, s = mapped_bank(sd, N, B, 8, 10, 10, 10)
    with f, sd.EkfSlam(3 + 2 * 10, batch=2) as small:
        before = [f.state(b) for b in range(B)]
        sbefore = [small.state(b) for b in range(2)]

        def unchanged():
            return all(same(f.state(b), before[b]) for b in range(B)) and all(same(small.state(b), sbefore[b]) for b in range(2))

        ints = lambda *v: (C.c_int * len(v))(*v)
        assert lib.ekf_copy_trajectories(f._h, None, f._h, None, -1) == EKF_ERR_ARG and unchanged()      # k < 0
        assert lib.ekf_copy_trajectories(f._h, None, f._h, ints(0, 0), 2) == EKF_ERR_ARG and unchanged()  # NULL arrays
        assert lib.ekf_copy_trajectories(f._h, ints(1, 2), f._h, None, 2) == EKF_ERR_ARG and unchanged()
        for src, dst in (([B], [0]), ([-1], [0]), ([0], [B]), ([0], [-1]),      # an index outside its bank
                         ([0, 0], [1, 1]),                                        # a destination twice
                         ([2], [2]),                                              # s == d
                         ([0, 1], [1, 2])):                                       # both a source and a destination
            with pytest.raises(sd.EkfError):
                f.copy_from(f, src, dst)
            assert unchanged(), (src, dst)
        with pytest.raises(sd.EkfError, match="n_max"):                           # a source n above the destination's n_max
            small.copy_from(f, 0, 1)
        with pytest.raises(sd.EkfError):
            small.copy_from(f, [0], [2])
        assert unchanged()
        if sd.device_count() > 1:                                                 # different devices
            with sd.EkfSlam(3 + 2 * N, device=1) as far:
                with pytest.raises(sd.EkfError, match="different devices"):
                    far.copy_from(f)
                assert unchanged()
        assert lib.ekf_copy_trajectories(f._h, None, f._h, None, 0) == 0 and unchanged()                # k = 0
        f.fork(0, [])
        f.copy_from(small, [], [])
        assert unchanged() and f.flags(0) == 0
        f.copy_from(small, 1, 3)                                   # and both handles are usable afterwards
        assert same(f.state(3), sbefore[1]) and f.size(3) == 3 and same(f.state(0), before[0])


# ---- 11: the tuning sweep from a mapped state ----------------------------------------------------------------------------------
def test_tune_noise_from_a_mapped_state(sd):
    import slam_duckietown_amd.evaluation as ev
    from tests.streams import wandering
    N, steps = 12, 200
    n = 3 + 2 * N
    means, lin, ang, idx, zr, zb, m = wandering(N, 1, steps, 6, 9400)
    diag0 = np.r_[np.full(3, 1e-3), np.full(2 * N, 0.05)]
    mgrid, qgrid = np.array([0.05, 0.1, 0.2]), np.array([0.3, 0.7, 1.2])
    with sd.EkfSlam(n) as f:
        f.set_state_diag(means[0], diag0)
        f.run_stream(lin[:100], ang[:100], idx[:100], zr[:100], zb[:100], m[:100])
        mapped = f.state()
        stream = (lin[100:, 0], ang[100:, 0], idx[100:, 0], zr[100:, 0], zb[100:, 0], m[100:, 0])
        res = ev.tune_noise(stream, mgrid, qgrid, None, None, start=(f, 0))
        assert same(f.state(), mapped)                             # the start filter is only read
        assert path_ran(f, "default_path")
    assert res.bank_sizes == (9,) and res.loglik.shape == (3, 3)
    for i, s in enumerate(mgrid):
        for j, q in enumerate(qgrid):
            with sd.EkfSlam(n, config=sd.EkfConfig(motion_sigma=float(s), meas_sigma=float(q))) as h:
                h.set_state(*mapped)
                h.log_innovations(100)
                h.run_stream(lin[100:], ang[100:], idx[100:], zr[100:], zb[100:], m[100:])
                want = ev.nis_consistency(h.innovations(0, 100)).loglik[0]
            assert abs(res.loglik[i, j] - want) <= 1e-9 * abs(want), (s, q, res.loglik[i, j], want)


# ---- a seeded soak against the model ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", range(FUZZ_RUNS))
def test_seeded_fuzz_against_the_model(sd, run):
    """step / grow / remove / fork interleaved (tests/fork_model.py: drive), on the small-state path (even runs) and on the
    general kernels (odd runs): twins stay twins bit for bit, slot properties stay, every trajectory equals the model."""
    N, cap = (8, 14) if run % 2 == 0 else (60, 66)
    B = 4
    states = fm.start_states(N, B, 700 + 10 * run)
    model = fm.ForkBank(states)
    ms, qs = [0.1, 0.1, 0.2, 0.05], [0.7, 0.7, 0.4, 1.0]
    model.set_noise(ms, qs)
    model.log_innovations(64)
    with sd.EkfSlam(3 + 2 * cap, batch=B) as f:
        f.set_noise(ms, qs)
        f.log_innovations(64)
        for b, (mu, P) in enumerate(states):
            f.set_state(mu, P, b)
        ran = fm.drive(model, 900 + run, FUZZ_OPS, cap, f, TIGHT)
        assert path_ran(f, "default_path") and all(f.flags(b) == 0 for b in range(B))
    print("fuzz run", run, ran)
    assert ran["step"] > 0
