"""GPU: localisation from raw detections (ekf_localize_detections / ekf_download_unmatched; EkfSlam.localize_detections,
unmatched_tags, reset_pose; GpuBackend(localize=True)).  The maps are built with a few step_detections windows, so the tag table
is the device's own.  Three yardsticks: the same handle forked before the call and given `localize` with what ekf_download_tags
reported (bit for bit: `same`), the host route -- frontend.associate_known, then localize -- (1e-12 on the association's numbers,
`close` on the state), and the dense model tests/localize_model.py through parity_blocks.assert_state_close at the block bar of
1e-9.  Small cases run on the small-state handle (N = 6, n_max = 15) and on the general kernels (both_paths), the path asserted."""
import dataclasses

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests import loc_det_world as ldw
from tests import localize_model as lm
from tests.conftest import path_ran
from tests.gpu_support import close, same, sd  # noqa: F401
from tests.parity_blocks import assert_state_close, fmt_state

pytestmark = pytest.mark.gpu

TOL = 1e-9
INIT_VAR = 1e4
LIN, ANG = ldw.LIN, ldw.ANG
EKF_FLAG_ASSOC = 2


def built_map(sd, N=6, n_max=15, seed=5, batch=1, options=()):
    """A world of N tags and a handle that has mapped it with four step_detections windows (every slot of a bank the same)."""
    world = ldw.World(N, seed)
    f = sd.EkfSlam(n_max, batch=batch)
    for name, value in options:
        f.set_option(name, value)
    for w in ldw.mapping_windows(world):
        f.step_detections(LIN, ANG, w if batch == 1 else [w] * batch)
    f.flush()
    assert [f.size(b) for b in range(batch)] == [3 + 2 * N] * batch and f.flags() == 0 and f.assoc_fallbacks() == 0
    return world, f


def twin_of(sd, f, b=0, options=()):
    """A batch-1 handle holding trajectory b of f bit for bit (state, size, bound, tag table)."""
    g = sd.EkfSlam(f.n_max, batch=1)
    for name, value in options:
        g.set_option(name, value)
    g.copy_from(f, b, 0)
    assert same(f.state(b), g.state(0)) and f.tag_index(b) == g.tag_index(0)
    return g


def localize_with_tags(g, tags, lin=LIN, ang=ANG):
    """`localize` with idx, range and bearing exactly as tags_positions (ekf_download_tags) reported them."""
    idx = list(tags)
    g.localize(lin, ang, idx, [tags[k][4] for k in idx], [tags[k][5] for k in idx])


def check(f, model, what, b=0):
    got = (*f.state(b), f.tag_index(b), f.flags(b))
    err = assert_state_close(got, (model[0], model[1], f.tag_index(b)), INIT_VAR, tol=TOL, entry_tol=TOL, what=what + ": ")
    print(f"{what}: {fmt_state(err)}")


def same_logs(f, g):
    a, b = f.innovations(), g.innovations()
    assert np.array_equal(a.steps, b.steps) and np.array_equal(a.m, b.m)
    for k in range(len(a.steps)):
        m = int(a.m[k, 0])
        assert m > 0
        for x, y in ((a.idx, b.idx), (a.y, b.y), (a.S, b.S), (a.nis, b.nis), (a.rejected, b.rejected)):
            assert np.array_equal(x[k, 0, :m], y[k, 0, :m])
    p, q = f.poses(), g.poses()
    assert p.first == q.first and np.array_equal(p.mean, q.mean) and np.array_equal(p.cov, q.cov) and p.mean.shape[0] == len(a.steps)


# ---- 1: the same bits as localize, logs included ---------------------------------------------------------------------------------
def test_same_bits_as_localize(sd, both_paths):
    world, f = built_map(sd)
    with f, twin_of(sd, f) as g:
        for h in (f, g):
            h.log_innovations(4)
            h.log_poses(4)
        index = f.tag_index()
        for which, frames in (([3, 0, 5, 1], 3), ([2], 1), ([4, 5, 0, 1, 2, 3], 2)):
            world.move()
            f.localize_detections(LIN, ANG, world.window(which, frames))
            tags = f.tags_positions()
            assert list(tags) == [index[world.ids[j]] for j in which] and f.unmatched_tags() == []
            localize_with_tags(g, tags)
            assert same(f.state(), g.state())
        same_logs(f, g)
        assert f.tag_index() == index and f.flags() == 0 and f.assoc_fallbacks() == 0
        assert path_ran(f, both_paths)


# ---- 2: the device's association against the host's, and the device route against the host route -----------------------------------
def test_device_against_host(sd, both_paths):
    from slam_duckietown_amd import frontend
    world, f = built_map(sd)
    with f, twin_of(sd, f) as g:
        world.move()
        win = world.window([1, 4, 2, 0], 3)
        win[1][1].insert(2, ldw.det(1001, 0.2, 0.7))          # a tag the map does not hold
        want, unmatched = frontend.associate_known(win, g.tag_index(), g.mean()[:3])
        f.localize_detections(LIN, ANG, win)
        got = f.tags_positions()
        assert list(got) == list(want) and f.unmatched_tags() == unmatched == [1001]
        for j in want:
            assert got[j][3] == want[j][3]
            dev = np.array([got[j][q] for q in (0, 1, 4, 5)])
            worst = float(np.abs(dev - [want[j][q] for q in (0, 1, 4, 5)]).max())
            print(f"landmark {j}: xw, yw, range, bearing against frontend.associate_known {worst:.1e}")
            assert worst <= 1e-12
        before = g.assoc_fallbacks()
        g._host_index[0] = g.tag_index()                       # the host is in charge of this trajectory's TAG_INDEX: the host route
        g.localize_detections(LIN, ANG, win)
        assert g.assoc_fallbacks() == before + 1 and f.assoc_fallbacks() == 0 and g.unmatched_tags() == [1001]
        assert list(g.tags_positions()) == list(want)
        close(f.state()[0], g.state()[0])
        close(f.state()[1], g.state()[1])
        assert path_ran(f, both_paths)


# ---- 3: six windows against the dense model --------------------------------------------------------------------------------------
def test_against_the_model(sd, both_paths):
    world, f = built_map(sd)
    with f:
        model, index = f.state(), f.tag_index()
        frozen = (model[0][3:].copy(), model[1][3:, 3:].copy())
        for k in range(6):
            world.move(LIN, 0.005 if k == 3 else ANG)          # (the straight branch once)
            win = world.window([(2 * k + i) % world.N for i in range(1 + k % 4)], 1 + k % 3)
            if k == 2:
                win[0][1].append(ldw.det(1003, -0.3, 0.9))
            f.localize_detections(LIN, 0.005 if k == 3 else ANG, win)
            model, tags, unmatched = ldw.model_window(*model, index, win, LIN, 0.005 if k == 3 else ANG)
            assert f.unmatched_tags() == unmatched and list(f.tags_positions()) == list(tags)
        check(f, model, "six localisation windows")
        got = f.state()
        assert np.array_equal(got[0][3:], frozen[0]) and np.array_equal(got[1][3:, 3:], frozen[1]) and f.size() == 15
        assert path_ran(f, both_paths)


# ---- 4: the map is frozen ----------------------------------------------------------------------------------------------------------
def test_frozen(sd, both_paths):
    """Two unknown tags, one ignored, one beyond the gate, one seen in three frames, one id of -1.  (The window with the bad id
    goes to the device entry directly: EkfSlam.localize_detections would route it through the host, which has no such limit.)"""
    N = 4
    world, f = built_map(sd, N=N)                               # n_max = 15: room for two more landmarks
    with f, twin_of(sd, f) as g:
        for h in (f, g):
            h.set_association(1.5, [world.ids[3]])              # a tag of the map, ignored from here on
        world.move()
        a, b3, far = world.window([0], 1)[0][1][0], [world.window([1], 1)[0][1][0] for _ in range(3)], ldw.det(world.ids[2], 1.2, 1.2)
        ign, u1, u2, bad = world.window([3], 1)[0][1][0], ldw.det(1010, 0.1, 0.8), ldw.det(1005, -0.2, 0.6), ldw.det(-1, 0.0, 0.5)
        clean = [(0.0, [a, u1, ign, b3[0]]), (1.0, [b3[1], far, u2, ldw.det(1010, 0.1, 0.81)]), (2.0, [b3[2]])]
        dirty = [(0.0, clean[0][1] + [bad]), clean[1], clean[2]]
        start, index = f.state(), f.tag_index()
        for h in (f, g):
            h._per_traj(LIN, "lin", h._lin)
            h._per_traj(ANG, "ang", h._ang)
        f._localize_detections_device([dirty])
        g._localize_detections_device([clean])
        for h in (f, g):
            got = h.state()
            assert h.size() == 3 + 2 * N and h.tag_index() == index
            assert np.array_equal(got[0][3:], start[0][3:]) and np.array_equal(got[1][3:, 3:], start[1][3:, 3:])
            assert h.unmatched_tags() == [1010, 1005]
        assert f.flags() == EKF_FLAG_ASSOC and g.flags() == 0   # the bad id, and nothing else, sets the flag
        assert same(f.state(), g.state()) and not np.array_equal(f.state()[0][:3], start[0][:3])
        tags = g.tags_positions()
        la, lb = index[world.ids[0]], index[world.ids[1]]
        assert list(tags) == [la, lb] and [tags[j][3] for j in tags] == [world.ids[0], world.ids[1]]
        model, mtags, unmatched = ldw.model_window(*start, index, clean, cfg=dataclasses.replace(ldw.CFG, ignore_tags=(world.ids[3],)))
        assert unmatched == [1010, 1005] and list(mtags) == [la, lb]
        check(g, model, "the frozen window")
        # the table was not disturbed: a mapping window on the same handle appends the unknown tags at N and N + 1
        for h in (f, g):
            h.step_detections(LIN, ANG, clean)
            assert h.size() == 3 + 2 * (N + 2) and h.tag_index() == {**index, 1010: N, 1005: N + 1}
        assert path_ran(f, both_paths)


# ---- 5: the edges of the walk ------------------------------------------------------------------------------------------------------
def test_empty_window_and_unknown_tags_only(sd, both_paths):
    world, f = built_map(sd)
    with f, twin_of(sd, f) as g:
        f.localize_detections(LIN, ANG, [])                   # an empty window: localize with m = 0
        g.localize(LIN, ANG, [], [], [])
        assert same(f.state(), g.state()) and f.unmatched_tags() == [] and f.tags_positions() == {}
        world.move()
        start = f.state()
        f.localize_detections(LIN, ANG, [(0.0, [ldw.det(1001, 0.1, 0.7), ldw.det(1002, 0.2, 0.7)]), (1.0, [ldw.det(1001, 0.1, 0.7)])])
        g.localize(LIN, ANG, [], [], [])
        assert f.unmatched_tags() == [1001, 1002] and f.tags_positions() == {} and f.flags() == 0
        assert same(f.state(), g.state()) and not same(f.state(), start)
        # a prediction only: the pose `predict` gives, bit for bit
        with twin_of(sd, f) as r:
            r.set_state(*start)
            r.predict(LIN, ANG)
            assert np.array_equal(r.mean()[:3], f.mean()[:3])
        assert path_ran(f, both_paths)


def test_seventeen_known_tags_take_two_passes(sd):
    N = 20
    opts = [("small_state", 0)]
    world, f = built_map(sd, N=N, n_max=3 + 2 * N, seed=9, options=opts)
    with f, twin_of(sd, f, options=opts) as g:
        for h in (f, g):
            h.log_innovations(2)
            h.log_poses(2)
        world.move()
        which = [(3 * i + 1) % N for i in range(17)]
        assert len(set(which)) == 17
        f.localize_detections(LIN, ANG, world.window(which, 2))
        tags = f.tags_positions()
        assert len(tags) == 17 and list(tags) == [f.tag_index()[world.ids[j]] for j in which]
        localize_with_tags(g, tags)                            # 17 indices: two passes, the prediction in the first
        assert same(f.state(), g.state()) and f.flags() == 0
        same_logs(f, g)
        assert int(f.innovations().m[0, 0]) == 17
        assert path_ran(f, "general_kernels")
        # 33 distinct tags in one window: beyond the device front end, Python takes the host route
        world.move()
        win = world.window(list(range(N)), 1)
        known_only = [(win[0][0], list(win[0][1]))]
        win[0][1][5:5] = [ldw.det(990 + i, 0.05 * (i - 6), 0.9) for i in range(13)]
        before = f.assoc_fallbacks()
        f.localize_detections(LIN, ANG, win)
        g.localize_detections(LIN, ANG, known_only)            # the same matches on the device
        assert f.assoc_fallbacks() == before + 1 and g.assoc_fallbacks() == 0
        assert f.unmatched_tags() == [990 + i for i in range(13)] and list(f.tags_positions()) == list(g.tags_positions())
        close(f.state()[0], g.state()[0])
        close(f.state()[1], g.state()[1])


def test_sixty_five_detections_cross_the_chunk_edge(sd, both_paths):
    from slam_duckietown_amd import frontend
    world, f = built_map(sd)
    with f, twin_of(sd, f) as g:
        world.move()
        win = world.window([5, 2, 0, 3, 1], 13)                # 65 detections: the 65th is the second chunk
        assert sum(len(t) for _s, t in win) == 65
        win[12][1][4] = ldw.det(1001, 0.3, 0.8)                # ... and it is an unknown tag
        want, unmatched = frontend.associate_known(win, g.tag_index(), g.mean()[:3])
        f.localize_detections(LIN, ANG, win)
        tags = f.tags_positions()
        assert list(tags) == list(want) and f.unmatched_tags() == unmatched == [1001]
        for j in want:
            assert np.abs(np.array([tags[j][q] for q in (0, 1, 4, 5)]) - [want[j][q] for q in (0, 1, 4, 5)]).max() <= 1e-12
        localize_with_tags(g, tags)
        assert same(f.state(), g.state()) and f.flags() == 0
        assert path_ran(f, both_paths)


# ---- 6: an uneven bank ---------------------------------------------------------------------------------------------------------------
def test_uneven_bank(sd, both_paths):
    """Three slots of 63, 47 and 71 states with different tag tables under one launch; slot 1 gets no detection and moves by its
    prediction only; every slot equals its own batch-1 run bit for bit."""
    sizes = (30, 22, 34)
    worlds = [ldw.World(N, 60 + b) for b, N in enumerate(sizes)]
    maps = [ldw.mapping_windows(w) for w in worlds]
    with sd.EkfSlam(71, batch=3) as f:
        for k in range(4):
            f.step_detections(LIN, ANG, [maps[b][k] for b in range(3)])
        f.flush()
        assert [f.size(b) for b in range(3)] == [63, 47, 71] and f.assoc_fallbacks() == 0
        alone = [twin_of(sd, f, b) for b in range(3)]
        try:
            for w in worlds:
                w.move()
            wins = [worlds[0].window([29, 3, 11, 0, 17], 2), [], worlds[2].window(list(range(33, 12, -1)), 1)]   # 21 tags: two passes
            wins[0][0][1].append(ldw.det(1001, 0.1, 0.8))
            start1 = f.state(1)
            f.localize_detections(LIN, ANG, wins)
            for b in range(3):
                alone[b].localize_detections(LIN, ANG, wins[b])
                assert same(f.state(b), alone[b].state()), f"slot {b} differs from its batch-1 run"
                assert f.unmatched_tags(b) == alone[b].unmatched_tags() and list(f.tags_positions(b)) == list(alone[b].tags_positions())
                assert f.flags(b) == 0 and f.size(b) == (63, 47, 71)[b]
            assert len(f.tags_positions(0)) == 5 and len(f.unmatched_tags(0)) == 1 and len(f.tags_positions(2)) == 21
            want1 = lm.literal_step(*start1, LIN, ANG, [], [], [], ldw.CFG)
            check(f, want1, "slot 1: the prediction alone", b=1)
            assert np.array_equal(f.state(1)[0][3:], start1[0][3:])
            assert path_ran(f, both_paths)
        finally:
            for g in alone:
                g.close()


# ---- 7: the active bound rises on the device ---------------------------------------------------------------------------------------
def test_bound_rises_over_a_matched_landmark(sd):
    """N = 40 with the bound at 23 (ten landmarks observed); the window matches landmark 35 (state indices 73, 74: beyond the 64
    column edge).  The host learns the new bound only through its mirror: joint() over every landmark, then two SLAM steps that
    name landmark 35, agree with the model."""
    N = 40
    world = ldw.World(N, 77)
    mean0 = np.zeros(3 + 2 * N)
    mean0[3:] = (world.xy + world.rng.normal(0.0, 0.01, world.xy.shape)).ravel()
    diag0 = np.full(3 + 2 * N, 0.02)
    diag0[:3] = 0.1
    with sd.EkfSlam(3 + 2 * N, batch=1) as f:
        f.set_option("active_bound", 1)
        f.set_state_diag(mean0, diag0)
        f.set_tag_index({t: j for j, t in enumerate(world.ids)})
        for k in range(3):
            world.move()
            f.step_detections(LIN, ANG, world.window([(3 * k + i) % 10 for i in range(5)], 2))
        f.flush()
        model, index = f.state(), f.tag_index()
        assert f.size() == 3 + 2 * N and not model[1][:3, 23:].any() and model[1][:3, 3:23].all()
        world.move()
        win = world.window([2, 35], 2)
        f.localize_detections(LIN, ANG, win)
        model, tags, _ = ldw.model_window(*model, index, win)
        assert list(tags) == [2, 35]
        jm, jc = f.joint(list(range(N)), 0)
        assert lm.rel(jm, model[0]) <= TOL and lm.rel(jc, model[1]) <= TOL
        assert jc[:3, 73:75].any() and not jc[:3, 75:].any()
        check(f, model, "the bound risen over landmark 35")
        rng = np.random.default_rng(7)
        for lms in ([35, 3], [9, 35, 1]):                      # a stale mirror would leave landmark 35's correlations out of their pass
            d = model[0][3:].reshape(-1, 2)[lms] - model[0][:2]
            zr = np.hypot(d[:, 0], d[:, 1]) + rng.normal(0.0, 0.01, len(lms))
            zb = orc.wrap_pi(np.arctan2(d[:, 1], d[:, 0]) - model[0][2] + rng.normal(0.0, 0.01, len(lms)))
            f.step(LIN, ANG, lms, zr, zb)
            model = orc.ekf_step_dense(*model, LIN, ANG, np.array(lms, dtype=np.int32), zr, zb, ldw.CFG)
        f.flush()
        check(f, model, "two SLAM steps behind it")
        assert path_ran(f, "general_kernels")


# ---- 8: ranks pending at entry -----------------------------------------------------------------------------------------------------
def test_pending_ranks_at_entry(sd, both_paths):
    world, f = built_map(sd)
    with f, twin_of(sd, f) as g:
        rng = np.random.default_rng(8)
        mean = f.mean()
        for lms in ([0, 3], [5, 1, 2]):
            d = mean[3:].reshape(-1, 2)[lms] - mean[:2]
            zr, zb = np.hypot(d[:, 0], d[:, 1]) + rng.normal(0, 0.01, len(lms)), orc.wrap_pi(np.arctan2(d[:, 1], d[:, 0]) - mean[2])
            for h in (f, g):
                h.step(LIN, ANG, lms, zr, zb)                  # (no flush: what the steps appended is pending)
            world.move()
        g.flush()
        world.move()
        win = world.window([4, 0, 2], 2)
        f.localize_detections(LIN, ANG, win)
        g.localize_detections(LIN, ANG, win)
        assert same(f.state(), g.state()) and list(f.tags_positions()) == list(g.tags_positions()) == [f.tag_index()[world.ids[j]] for j in (4, 0, 2)]
        assert path_ran(f, both_paths)


# ---- 9: the NIS gate ---------------------------------------------------------------------------------------------------------------
def test_nis_gate_rejects_a_gross_outlier(sd, both_paths):
    world, f = built_map(sd)
    with f, twin_of(sd, f) as g:
        world.move()
        win = world.window([1, 4, 2], 1)
        keep = [(0.0, [win[0][1][0], win[0][1][2]])]
        t = win[0][1][1].pose_t.ravel()
        win[0][1][1] = ldw.det(world.ids[4], t[2], -t[0])       # landmark 4 a quarter turn off its bearing
        log = []
        ldw.model_window(*f.state(), f.tag_index(), win, log=log)
        bad = log[1][3]
        gate = 0.5 * bad
        assert max(log[0][3], log[2][3]) < 0.5 * gate, [r[3] for r in log]
        for h in (f, g):
            h.set_nis_gate(gate)
        start = f.state()
        f.localize_detections(LIN, ANG, win)
        g.localize_detections(LIN, ANG, keep)
        assert list(f.gate_counts()) == [1] and list(g.gate_counts()) == [0]
        assert same(f.state(), g.state()) and len(f.tags_positions()) == 3
        assert lm.rel(f.state()[0][:3], start[0][:3]) > 1e-6   # the others are applied
        assert path_ran(f, both_paths)


# ---- 10: reset_pose ------------------------------------------------------------------------------------------------------------------
def test_reset_pose(sd, both_paths):
    world, f = built_map(sd)
    with f, twin_of(sd, f) as g:
        start = f.state()
        pose, cov = np.array([0.4, -0.2, 1.1]), np.array([[0.09, 0.01, 0.0], [0.01, 0.08, -0.005], [0.0, -0.005, 0.04]])
        f.reset_pose(pose, cov)                                # nothing pending
        mean, P = f.state()
        assert np.array_equal(mean[:3], pose) and np.array_equal(P[:3, :3], cov)
        assert not P[:3, 3:].any() and not P[3:, :3].any()     # exact zeros
        assert np.array_equal(mean[3:], start[0][3:]) and np.array_equal(P[3:, 3:], start[1][3:, 3:]) and f.flags() == 0
        # with ranks pending: against the dense model
        rng = np.random.default_rng(10)
        model = g.state()
        for lms in ([0, 3], [5, 1, 2]):
            d = model[0][3:].reshape(-1, 2)[lms] - model[0][:2]
            zr, zb = np.hypot(d[:, 0], d[:, 1]) + rng.normal(0, 0.01, len(lms)), orc.wrap_pi(np.arctan2(d[:, 1], d[:, 0]) - model[0][2])
            g.step(LIN, ANG, lms, zr, zb)
            model = orc.ekf_step_dense(*model, LIN, ANG, np.array(lms, dtype=np.int32), zr, zb, ldw.CFG)
        g.reset_pose(pose, cov)
        wm, wP = model[0].copy(), 0.5 * (model[1] + model[1].T)
        wm[:3] = pose
        wP[:3, :] = 0.0
        wP[:, :3] = 0.0
        wP[:3, :3] = cov
        got = g.state()
        close(got[0], wm)
        close(got[1], wP)
        assert path_ran(g, both_paths)


def test_recovery_after_a_pose_reset(sd, both_paths):
    """The kidnapped robot: tests/test_localize_detections_cpu.py shows that the dense model meets this on the same stream."""
    world, wins, reset_truth, loc = ldw.recovery_stream()
    with sd.EkfSlam(15, batch=1) as f:
        f.set_noise(**ldw.RECOVERY_NOISE)
        f.set_state(np.zeros(3), np.eye(3) * ldw.RECOVERY_P0)
        for w in wins:
            f.step_detections(LIN, ANG, w)
        f.flush()
        assert f.size() == 15
        f.reset_pose(reset_truth + ldw.RECOVERY_OFFSET, ldw.RECOVERY_COV)
        d2 = [ldw.mahalanobis(*f.state(), reset_truth)]
        for win, truth in loc:
            f.localize_detections(LIN, ANG, win)
            assert len(f.tags_positions()) == 4 and f.unmatched_tags() == []
            d2.append(ldw.mahalanobis(*f.state(), truth))
        err = float(np.linalg.norm(f.mean()[:2] - loc[-1][1][:2]))
        print(f"recovery: Mahalanobis^2 at the reset and behind each window {[round(v, 2) for v in d2]}, final position error {err:.4f} m")
        assert d2[-1] < ldw.CHI2_3_0999 and err < 0.1 and f.flags() == 0
        assert path_ran(f, both_paths)


# ---- 11: GpuBackend(localize=True) under the replay driver -------------------------------------------------------------------------
def test_gpu_backend_in_localisation_mode(sd, both_paths):
    import slam_duckietown_amd.replay as rp
    world, f = built_map(sd)
    with f:
        mean, cov = f.state()
        index = f.tag_index()

    class Recording(rp.GpuBackend):
        def __init__(self, **kw):
            super().__init__(**kw)
            self.calls = []

        def step(self, ang, lin, detections, tag_index):
            self.calls.append((ang, lin, list(detections)))
            return super().step(ang, lin, detections, tag_index)

    lines, lt, rt = [], 100, 200
    for k in range(40):
        stamp = 20.0 + 0.1 * k
        lt, rt = lt + 1 + k % 2, rt + 2
        lines += [f"{stamp:.3f},left_wheel,{lt}", f"{stamp:.3f},right_wheel,{rt}"]
        if k % 3 == 0:
            tags = world.window([(k + i) % world.N for i in range(3)])[0][1]
            if k == 9:
                tags.append(ldw.det(1001, 0.1, 0.8))
            lines.append(f"{stamp + 0.01:.3f},detections,{[(t.tag_id, [float(v) for v in t.pose_t.ravel()], t.pose_err) for t in tags]!r}")
    be = Recording(capacity=15, localize=True)
    try:
        be.set_map(mean, cov, index)                           # (replay does the same again: the handle has its size by now)
        handle = be.filt
        mine = dict(index)
        res = rp.replay(lines, backend=be, localize=True, map_state=(mean, cov, mine))
        assert be.filt is handle and be.filt.n_max == 15 and mine == index and res.tag_index == index
        assert res.windows == len(be.calls) >= 4 and be.filt.assoc_fallbacks() == 0
        with sd.EkfSlam(15, batch=1) as g:
            g.set_state(mean, cov)
            g.set_tag_index(index)
            for k, (ang, lin, win) in enumerate(be.calls):
                g.localize_detections(lin, ang, win)
                assert np.array_equal(g.mean()[:3], res.poses[k]), k
                assert list(g.tags_positions()) == list(res.measured_tags[k])
            assert same(g.state(), (res.mean, res.covariance))
    finally:
        be.close()
