"""GPU: landmark removal (ekf_remove_landmarks, EkfSlam.remove_landmarks; k_remove in csrc/ekf_remove.hip).

Removal is exact and moves stored values only: every case compares mean and covariance bit for bit with np.delete of the
download taken just before the call, then, where the filter goes on, with the oracle run from that deleted state.  Each case
names the path that ran (path_ran, cadence_counters / ekf_debug_chained, last_pass)."""

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from slam_duckietown_amd.evaluation import landmark_rejections
from slam_duckietown_amd.frontend import remap_tag_index
from tests.conftest import path_ran
from tests.gated_oracle import gated_step
from tests.gpu_support import raw00, same, sd, tag  # noqa: F401

pytestmark = pytest.mark.gpu

TIGHT = 1e-10


def deleted(state, lms):
    """np.delete of a downloaded (mean, covariance) on both axes: the state indices of landmarks `lms`."""
    mu, P = state
    rows = np.array([3 + 2 * l + e for l in sorted(lms) for e in (0, 1)], dtype=int)
    return np.delete(mu, rows), np.delete(np.delete(P, rows, axis=0), rows, axis=1)


def kept_stream(N, steps, m, seed, o2n):
    """synthetic_stream's observations of the landmarks that are kept, renumbered by old_to_new (m per step varies)."""
    _, _, lin, ang, idx, zr, zb = orc.synthetic_stream(N, steps, m, seed)
    I, R, Bg = np.zeros((steps, m), np.int32), np.zeros((steps, m)), np.zeros((steps, m))
    mm = np.zeros(steps, np.int32)
    for k in range(steps):
        keep = o2n[idx[k]] >= 0
        c = int(keep.sum())
        I[k, :c], R[k, :c], Bg[k, :c], mm[k] = o2n[idx[k][keep]], zr[k][keep], zb[k][keep], c
    return lin, ang, I, R, Bg, mm


def oracle_run(state, lin, ang, I, R, Bg, mm):
    cfg = orc.EkfConfig()
    om, oP = state
    for k in range(len(lin)):
        c = int(mm[k])
        om, oP = orc.ekf_step_structured(om, oP, lin[k], ang[k], I[k, :c], R[k, :c], Bg[k, :c], cfg)
    return om, oP


def run_synthetic(f, N, steps, m, seed):
    _, _, lin, ang, idx, zr, zb = orc.synthetic_stream(N, steps, m, seed)
    B = f.batch
    f.run_stream(np.repeat(lin[:, None], B, 1), np.repeat(ang[:, None], B, 1), np.repeat(idx[:, None], B, 1),
                 np.repeat(zr[:, None], B, 1), np.repeat(zb[:, None], B, 1))


# ---- 1-3: bit-exactness -----------------------------------------------------------------------------------------------------
def test_bit_exact_with_rank_terms_pending(sd):
    """N = 500 x 1, 60 stream steps of 7 landmarks (packed cadences of 40 updates: the last one's ranks stay pending), remove
    {0, 17, last}."""
    N = 500
    mean0, diag0 = orc.synthetic_stream(N, 1, 7, 3)[:2]
    with sd.EkfSlam(3 + 2 * N) as f:
        f.set_state_diag(mean0, diag0)
        run_synthetic(f, N, 60, 7, 3)
        assert f.cadence_counters()[0] > 0 and path_ran(f, "general_kernels")
        pending = raw00(sd, f)
        before = f.state()
        assert pending != before[1][0, 0]                          # the download applied ranks that were pending
        o2n = f.remove_landmarks([0, 17, N - 1])
        assert f.size() == 3 + 2 * N - 6
        assert same(f.state(), deleted(before, [0, 17, N - 1]))
        assert o2n.dtype == np.int32 and o2n.shape == (N,) and o2n[0] == -1 and o2n[17] == -1 and o2n[N - 1] == -1
        assert o2n[1] == 0 and o2n[18] == 16 and o2n[N - 2] == N - 4
        assert f.flags() == 0


def test_bit_exact_small_state(sd, both_paths):
    N = 20
    mean0, diag0 = orc.synthetic_stream(N, 1, 6, 4)[:2]
    with sd.EkfSlam(3 + 2 * N) as f:
        f.set_state_diag(mean0, diag0)
        run_synthetic(f, N, 25, 6, 4)
        assert path_ran(f, both_paths)
        before = f.state()
        f.remove_landmarks([19, 2, 11])
        assert f.size() == 3 + 2 * (N - 3)
        assert same(f.state(), deleted(before, [2, 11, 19]))
        f.remove_landmarks([0])                                    # again, and the first landmark
        assert same(f.state(), deleted(deleted(before, [2, 11, 19]), [0]))


def test_bit_exact_column_panels(sd):
    """n_max > 4096: P in column panels of 4096 doubles.  Landmark 2046 holds state indices 4095 and 4096 (it straddles the
    panel boundary); others on both sides of it."""
    N = 2100
    n = 3 + 2 * N
    rng = np.random.default_rng(5)
    A = rng.normal(size=(n, 4)) * 0.2
    P0 = A @ A.T + np.diag(rng.uniform(0.5, 2.0, n))
    mean0 = orc.synthetic_stream(N, 1, 8, 5)[0]
    with sd.EkfSlam(n) as f:
        f.set_option("active_bound", 0)
        f.set_state(mean0, P0)
        run_synthetic(f, N, 6, 8, 5)
        assert "k_flush" in f.last_pass()
        before = f.state()
        rm = [1, 1500, 2040, 2046, 2047, 2099]
        f.remove_landmarks(rm)
        assert same(f.state(), deleted(before, rm))
        assert f.flags() == 0


def test_bank_per_trajectory_and_whole_bank(sd):
    N, B = 300, 4
    mean0, diag0 = orc.synthetic_stream(N, 1, 8, 6)[:2]
    sets = [[0], [5, 299], [], [100, 101, 150]]

    def fresh(f):
        for b in range(B):
            f.set_state_diag(mean0 + 0.01 * b, diag0, b)
        run_synthetic(f, N, 30, 8, 6)

    with sd.EkfSlam(3 + 2 * N, batch=B) as f:
        fresh(f)
        assert f.cadence_counters()[0] > 0
        before = [f.state(b) for b in range(B)]
        for b, rm in enumerate(sets):
            keep_others = [f.state(t) for t in range(B)]
            f.remove_landmarks(rm, b)
            for t in range(B):
                want = deleted(before[t], rm) if t == b else keep_others[t]
                assert same(f.state(t), want), (b, t)
        assert [f.size(b) for b in range(B)] == [3 + 2 * (N - len(s)) for s in sets]
    rm = [3, 77, 200]
    with sd.EkfSlam(3 + 2 * N, batch=B) as f, sd.EkfSlam(3 + 2 * N, batch=B) as g:
        fresh(f)
        fresh(g)
        o2n = f.remove_landmarks(rm, None)
        for b in range(B):
            assert np.array_equal(g.remove_landmarks(rm, b), o2n)
        for b in range(B):
            assert same(f.state(b), g.state(b))
            assert f.flags(b) == 0


# ---- 5-6: going on after a removal ------------------------------------------------------------------------------------------
def test_continue_on_the_chained_path(sd):
    """N = 1250 x 1 (the chained solves' regime): 40 steps, remove 3 landmarks, 200 more steps of a stream that observes the
    kept ones (renumbered) -- against the oracle from np.delete of the state before the removal."""
    N = 1250
    n = 3 + 2 * N
    mean0 = orc.synthetic_stream(N, 1, 8, 7)[0]
    rng = np.random.default_rng(7)
    A = rng.normal(size=(n, 4)) * 0.2
    P0 = A @ A.T + np.diag(rng.uniform(0.5, 2.0, n))              # (dense: the whole state active, the chained regime)
    lib = sd.load_library()
    with sd.EkfSlam(n) as f:
        f.set_state(mean0, P0)
        run_synthetic(f, N, 40, 8, 7)
        before = f.state()
        rm = [2, 600, 1249]
        o2n = f.remove_landmarks(rm)
        chained0 = lib.ekf_debug_chained(f._h)
        s = kept_stream(N, 200, 8, 17, o2n)
        f.stream_upload(*s[:5], m=s[5][:, None])
        f.stream_run(0, 200)
        got = f.state()
        assert lib.ekf_debug_chained(f._h) > chained0 and f.flags() == 0
    om, oP = oracle_run(deleted(before, rm), *s)
    assert orc.rel_fro(got[0], om) < TIGHT and orc.rel_fro(got[1], oP) < TIGHT


@pytest.mark.parametrize("active_bound", [1, 0])
def test_active_bound_on_a_growing_map(sd, active_bound):
    """A diagonal start (active bound 3), steps that observe landmarks 0..39 of 150 only (the bound grows to 83); remove
    landmark 5 (below the bound) and 120 (beyond it), then steps over the whole map -- against the oracle.  Removing every
    landmark then leaves n = 3, and stepping goes on."""
    N = 150
    cfg = orc.EkfConfig()
    mean0, diag0, lin, ang, idx, zr, zb = orc.synthetic_stream(N, 30, 8, 8)
    idx = idx % 40
    with sd.EkfSlam(3 + 2 * N) as f:
        f.set_option("active_bound", active_bound)
        f.set_state_diag(mean0, diag0)
        for k in range(30):
            f.step(lin[k], ang[k], idx[k], zr[k], zb[k])
        assert path_ran(f, "general_kernels")
        before = f.state()
        o2n = f.remove_landmarks([120, 5])
        s = kept_stream(N, 40, 8, 18, o2n)
        for k in range(40):
            c = int(s[5][k])
            f.step(s[0][k], s[1][k], s[2][k, :c], s[3][k, :c], s[4][k, :c])
        got = f.state()
        om, oP = oracle_run(deleted(before, [5, 120]), *s)
        assert orc.rel_fro(got[0], om) < TIGHT and orc.rel_fro(got[1], oP) < TIGHT
        before = f.state()
        f.remove_landmarks(np.arange(N - 2))
        assert f.size() == 3 and same(f.state(), deleted(before, range(N - 2)))
        om, oP = f.state()
        f.step(0.004, 0.02, [], [], [])
        om, oP = orc.ekf_step_dense(om, oP, 0.004, 0.02, [], [], [], cfg)
        mu, P = f.state()
        assert orc.rel_fro(mu, om) < TIGHT and orc.rel_fro(P, oP) < TIGHT and f.flags() == 0


# ---- 7, 11: the device association, the gate and the log ---------------------------------------------------------------------


def test_device_association_after_removal(sd):
    rng = np.random.default_rng(11)
    cfg = orc.EkfConfig()
    ids = [int(i) for i in rng.permutation(500)[:10]]
    bx = {i: float(rng.uniform(-0.5, 0.5)) for i in ids}
    bz = {i: float(rng.uniform(0.4, 1.1)) for i in ids}
    windows = [ids[:6], ids[2:9], ids[:4]]
    gone = ids[3]

    def window(k, win_ids):
        return [(k + 0.1 * fr, [tag(i, bx[i] + rng.normal(0, 0.004), bz[i] + rng.normal(0, 0.004)) for i in win_ids])
                for fr in range(2)]

    def oracle_window(om, oP, oti, win, lin, ang):
        tags = orc.associate(win, oti, om, cfg)
        om, oP = orc.augment(om, oP, len(oti), tags, cfg)
        order = list(tags.keys())
        om, oP = orc.ekf_step_dense(om, oP, lin, ang, order, [tags[i][4] for i in order], [tags[i][5] for i in order], cfg)
        return om, oP, order

    with sd.EkfSlam(3 + 2 * 30) as f:
        om, oP, oti = np.zeros(3), np.eye(3) * 0.1, {}
        for k, w in enumerate(windows):
            win = window(k, w)
            f.step_detections(0.004, 0.02, win)
            om, oP, _ = oracle_window(om, oP, oti, win, 0.004, 0.02)
        assert f.assoc_fallbacks() == 0 and path_ran(f, "default_path")
        assert f.tag_index() == oti
        last = list(f.tags_positions().keys())
        before = f.state()
        lm = oti[gone]
        o2n = f.remove_landmarks([lm])
        oti = remap_tag_index(oti, o2n)
        assert gone not in f.tag_index() and f.tag_index() == oti
        assert sorted(oti.values()) == list(range(len(oti)))
        assert list(f.tags_positions().keys()) == [int(o2n[j]) for j in last if o2n[j] >= 0]
        om, oP = deleted(before, [lm])
        assert same(f.state(), (om, oP))
        for k, w in enumerate([ids[4:8], [gone] + ids[7:10]]):
            win = window(10 + k, w)
            n_before = len(oti)                                    # (the last window sees the removed tag again)
            f.step_detections(0.003, 0.01, win)
            om, oP, _ = oracle_window(om, oP, oti, win, 0.003, 0.01)
            mu, P = f.state()
            assert orc.rel_fro(mu, om) < TIGHT and orc.rel_fro(P, oP) < TIGHT
        assert f.tag_index() == oti and oti[gone] == n_before       # seen again: a new landmark at the end of the map
        assert P[3 + 2 * n_before, 3 + 2 * n_before] < cfg.landmark_init_var and f.flags() == 0


def test_gate_log_and_removal_end_to_end(sd):
    """A tag whose FIRST detection is displaced by ~1 m enters the map unchecked; the gate rejects its later sightings,
    landmark_rejections names it, and after remove_landmarks its next sighting re-adds it where the others are."""
    rng = np.random.default_rng(12)
    cfg = orc.EkfConfig()
    cfg.motion_sigma, cfg.meas_sigma = 0.01, 0.03                 # (the reference's 0.7 would hide a 1 m error in S)
    g = 25.0
    ids = [int(i) for i in rng.permutation(300)[:8]]
    bx = {i: float(rng.uniform(-0.4, 0.4)) for i in ids}
    bz = {i: float(rng.uniform(0.5, 0.9)) for i in ids}
    bad = ids[4]
    bx[bad] = -0.3                                                 # (displaced by 1 m it stays inside the 1.5 m range gate)
    truth = {i: np.array([bz[i], -bx[i]]) for i in ids}           # world position seen from the pose (0, 0, 0)

    def window(k, displaced=False):
        return [(k + 0.1 * fr, [tag(i, bx[i] + (1.0 if displaced and i == bad else 0.0) + rng.normal(0, 0.003),
                                    bz[i] + rng.normal(0, 0.003)) for i in ids]) for fr in range(2)]

    wins = [window(0, displaced=True)] + [window(k) for k in range(1, 6)]
    later = [window(k) for k in range(6, 10)]

    def oracle_window(om, oP, oti, win):
        tags = orc.associate(win, oti, om, cfg)
        om, oP = orc.augment(om, oP, len(oti), tags, cfg)
        order = list(tags.keys())
        om, oP, *_ = gated_step(om, oP, 0.0, 0.0, order, [tags[i][4] for i in order], [tags[i][5] for i in order], cfg, g)
        return om, oP

    scfg = sd.EkfConfig(motion_sigma=cfg.motion_sigma, meas_sigma=cfg.meas_sigma)
    with sd.EkfSlam(3 + 2 * 20, config=scfg) as f, sd.EkfSlam(3 + 2 * 20, config=scfg) as keep:
        for h in (f, keep):
            h.log_innovations(32)
            h.set_nis_gate(g)
            for win in wins:
                h.step_detections(0.0, 0.0, win)
        assert path_ran(f, "default_path")
        lm_bad = f.tag_index()[bad]
        rej = landmark_rejections(f.innovations())
        assert rej.rejected[0, lm_bad] == len(wins) - 1
        assert rej.rejected[0].sum() == rej.rejected[0, lm_bad]
        assert f.gate_counts().tolist() == [len(wins) - 1]
        before, index = f.state(), f.tag_index()
        o2n = f.remove_landmarks([lm_bad])
        oti = remap_tag_index(index, o2n)
        assert f.tag_index() == oti
        om, oP = deleted(before, [lm_bad])
        for win in later:
            f.step_detections(0.0, 0.0, win)
            keep.step_detections(0.0, 0.0, win)
            om, oP = oracle_window(om, oP, oti, win)
            mu, P = f.state()
            assert orc.rel_fro(mu, om) < TIGHT and orc.rel_fro(P, oP) < TIGHT
        assert f.tag_index()[bad] == len(ids) - 1                  # re-added at the end of the map
        mu = f.mean()
        err = {i: np.linalg.norm(mu[3 + 2 * j:5 + 2 * j] - truth[i]) for i, j in f.tag_index().items()}
        others = max(e for i, e in err.items() if i != bad)
        assert err[bad] <= max(2.0 * others, 0.02), (err[bad], others)
        # without the removal the landmark stays near the displaced first detection
        mk, jk = keep.mean(), keep.tag_index()[bad]
        assert np.linalg.norm(mk[3 + 2 * jk:5 + 2 * jk] - truth[bad]) > 0.5
        assert f.flags() == 0 and keep.flags() == 0
        # the log keeps the indices it logged
        assert (f.innovations(0, 1).idx[0, 0] == np.arange(len(ids))).all()


# ---- 8-10: stale streams, bad arguments, removal then augmentation ------------------------------------------------------------
def test_stale_stream_is_refused_until_uploaded_again(sd):
    N = 200
    mean0, diag0, lin, ang, idx, zr, zb = orc.synthetic_stream(N, 20, 8, 9)
    with sd.EkfSlam(3 + 2 * N) as f:
        f.set_state_diag(mean0, diag0)
        f.stream_upload(lin, ang, idx, zr, zb)
        f.stream_run(0, 10)
        f.remove_landmarks([7])
        with pytest.raises(sd.EkfError, match="upload the stream again"):
            f.stream_run(10, 10)
        o2n = np.arange(N, dtype=np.int32) - (np.arange(N) > 7)
        o2n[7] = -1
        s = kept_stream(N, 10, 8, 19, o2n)
        f.stream_upload(*s[:5], m=s[5][:, None])
        f.stream_run(0, 10)
        f.sync()
        assert f.flags() == 0 and f.size() == 3 + 2 * (N - 1)


def test_bad_arguments_change_nothing(sd):
    N = 60
    mean0, diag0 = orc.synthetic_stream(N, 1, 8, 10)[:2]
    with sd.EkfSlam(3 + 2 * (N + 3), batch=2) as f:
        for b in range(2):
            f.set_state_diag(mean0, diag0, b)
        f.add_landmarks(np.zeros((3, 2)), 1)                       # trajectory 1: 63 landmarks
        run_synthetic(f, N, 10, 8, 10)
        before = [f.state(b) for b in range(2)]
        for args in (([3, 3], 0), ([-1], 0), ([N], 0), ([61], None), ([2, 5, 2], None)):
            with pytest.raises(sd.EkfError):
                f.remove_landmarks(*args)
        assert f.remove_landmarks([], 0).tolist() == list(range(N))     # k = 0: nothing
        for b in range(2):
            assert same(f.state(b), before[b])
        f.remove_landmarks([61], 1)                                # valid for trajectory 1 only
        assert f.size(1) == 3 + 2 * 62 and same(f.state(0), before[0])


def test_remove_then_add(sd):
    N = 400
    cfg = orc.EkfConfig()
    mean0, diag0 = orc.synthetic_stream(N, 1, 8, 13)[:2]
    with sd.EkfSlam(3 + 2 * (N + 5)) as f:
        f.set_state_diag(mean0, diag0)
        run_synthetic(f, N, 30, 8, 13)
        before = f.state()
        f.remove_landmarks([4, 9, 399])
        om, oP = deleted(before, [4, 9, 399])
        xy = np.array([[0.1, 0.2], [0.3, -0.4], [1.0, 1.5], [-0.2, 0.0], [0.5, 0.5]])
        f.add_landmarks(xy)
        nl = (len(om) - 3) // 2
        om, oP = orc.augment(om, oP, nl + 5, {nl + i: xy[i] for i in range(5)}, cfg)
        assert same(f.state(), (om, oP))
        s = kept_stream(N, 5, 8, 20, np.where(np.arange(N) < N - 3, np.arange(N), -1).astype(np.int32))
        for k in range(5):
            c = int(s[5][k])
            f.step(s[0][k], s[1][k], s[2][k, :c], s[3][k, :c], s[4][k, :c])
            om, oP = orc.ekf_step_structured(om, oP, s[0][k], s[1][k], s[2][k, :c], s[3][k, :c], s[4][k, :c], cfg)
        mu, P = f.state()
        assert orc.rel_fro(mu, om) < TIGHT and orc.rel_fro(P, oP) < TIGHT and f.flags() == 0
