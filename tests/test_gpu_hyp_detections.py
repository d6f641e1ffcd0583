"""GPU: a hypothesis bank driven by raw detections (ekf_hypotheses_step_detections / _detections_upload / _download_tags /
_set_association, k_hyp_associate; HypothesisBank.step_detections / upload_detections / tags / unmatched_tags / set_association;
replay.relocalize).  The maps are built with a few step_detections windows (tests/loc_det_world.py), so the tag table is the
device's own; the hypotheses are spread with `bank.reset`.

Yardsticks, bit for bit (np.array_equal) unless stated: a second bank with identical resets given `step` with what `tags()`
reported; the single filter's ekf_localize_detections on the source handle (association numbers) and on forked slots (states);
the host loop step_detections + resample_if for a run.  What the device reports for a window is judged against
tests/hyp_detections_model.py (frontend.associate_known's arithmetic) at 1e-12, the project's bar for that comparison; the state
after an adopt against the dense model at the block bar of 1e-9 (tests/test_gpu_localize_detections.py's)."""
import ctypes as C

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from slam_duckietown_amd import frontend
from tests import hyp_detections_model as hdm
from tests import hyp_support as hs
from tests import hypotheses_model as hm
from tests import loc_det_world as ldw
from tests.conftest import path_ran
from tests.gpu_support import sd  # noqa: F401
from tests.parity_blocks import assert_state_close, fmt_state

pytestmark = pytest.mark.gpu

TOL = 1e-9
INIT_VAR = 1e4
LIN, ANG = ldw.LIN, ldw.ANG
EKF_FLAG_ASSOC, EKF_DMAX, EKF_AMAX = 2, 256, 32
EKF_ERR_ARG, EKF_ERR_STATE = -1, -3
SEED_COV = np.array([[0.02, 0.004, 0.0], [0.004, 0.03, 0.001], [0.0, 0.001, 0.01]])


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


def seed_poses(f, K):
    """K poses beside the map's: hypothesis k a few centimetres and hundredths of a radian off, no two alike."""
    poses = np.tile(f.mean(0)[:3], (K, 1))
    poses[:, 0] += 0.03 * (np.arange(K) % 8)
    poses[:, 1] -= 0.01 * (np.arange(K) % 5)
    poses[:, 2] += 0.01 * (np.arange(K) % 3)
    return poses


def seeded(f, K):
    bank = f.hypotheses(K)
    bank.reset(seed_poses(f, K), SEED_COV)
    return bank


def reported(bank, step=None):
    return bank.tags(step), bank.unmatched_tags(step), bank.window_flags(step)


def step_with(bank, tags, lin=LIN, ang=ANG):
    """`step` with idx, range and bearing exactly as tags() reported them (more than 16: a step and an update)."""
    idx = list(tags)
    bank.step(lin, ang, idx, [tags[k][2] for k in idx], [tags[k][3] for k in idx])


def pair_step(a, b, win, index, N, what, ignore=(), lin=LIN, ang=ANG):
    """The window through step_detections on `a`, what the device reports judged against the model, the same lists through
    `step` on `b`, and the two banks compared bit for bit; -> what the device reported."""
    a.step_detections(lin, ang, win)
    got = reported(a)
    why = hdm.judge(got, hdm.walk(win, index, N, ignore_tags=ignore))
    assert why is None, f"{what}: {why}"
    step_with(b, got[0], lin, ang)
    assert hs.same_snapshot(hs.snapshot(a), hs.snapshot(b)), f"{what}: step_detections differs from step with the reported lists"
    return got


# ---- 1: the same bits as bank.step -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 65])
def test_same_bits_as_step(sd, K):
    world, f = built_map(sd)
    with f, seeded(f, K) as a, seeded(f, K) as b:
        index = f.tag_index()
        for which, frames in (([3, 0, 5, 1], 3), ([2], 1), ([4, 5, 0, 1, 2, 3], 2)):
            world.move()
            tags, unmatched, flag = pair_step(a, b, world.window(which, frames), index, world.N, f"K = {K}, tags {which}")
            assert list(tags) == [index[world.ids[j]] for j in which] and unmatched == [] and flag == 0
        got = hs.snapshot(a)
        assert (got.n_obs == 11).all() and (got.flags == 0).all() and np.isfinite(got.pose).all() and len(np.unique(got.loglik)) > 1


# ---- 2: the same association bits as the single filter -----------------------------------------------------------------------------
def test_same_association_bits_as_localize_detections(sd, both_paths):
    world, f = built_map(sd)
    with f, seeded(f, 3) as bank:
        index, pose = f.tag_index(), f.mean()[:3].copy()
        world.move()
        win = world.window([5, 2, 0, 3], 3)
        win[1][1].insert(2, ldw.det(1001, 0.3, 0.8))           # an unknown tag, seen twice
        win[2][1].append(ldw.det(1001, 0.31, 0.79))
        win[0][1].append(ldw.det(1002, -0.2, 0.6))
        bank.step_detections(LIN, ANG, win)
        f.localize_detections(LIN, ANG, win)
        mine, single = bank.tags(), f.tags_positions()
        assert list(mine) == list(single) == [index[world.ids[j]] for j in (5, 2, 0, 3)]
        for k in mine:                                         # tag id, err, range, bearing: the same bits
            assert mine[k][0] == single[k][3]
            assert np.array_equal(np.array(mine[k][1:]), np.array([single[k][2], single[k][4], single[k][5]])), k
        assert bank.unmatched_tags() == f.unmatched_tags() == [1002, 1001] and bank.window_flags() == 0
        want, unmatched = frontend.associate_known(win, index, pose, n_landmarks=world.N)
        assert list(want) == list(mine) and unmatched == [1002, 1001]
        for k in mine:
            assert np.abs(np.array(mine[k][1:]) - [want[k][2], want[k][4], want[k][5]]).max() <= hdm.TOL, k
        assert path_ran(f, both_paths)


# ---- 3: the same bits as forked slots ------------------------------------------------------------------------------------------------
def test_same_bits_as_forked_slots(sd, both_paths):
    K = 3
    world, f = built_map(sd, batch=K + 1)
    with f, f.hypotheses(K) as bank:
        poses = seed_poses(f, K)
        bank.reset(poses, SEED_COV)
        for k in range(K):
            f.reset_pose(poses[k], SEED_COV, b=k + 1)
        for which, frames in (([3, 0, 5, 1], 3), ([], 1), ([4, 5, 0, 1, 2, 3], 2)):
            world.move()
            win = world.window(which, frames) if which else []
            bank.step_detections(LIN, ANG, win)
            f.localize_detections(LIN, ANG, [win] * (K + 1))
            for k in range(K):
                hs.assert_same_bits(bank, k, f, k + 1, f"tags {which}: hypothesis {k} against slot {k + 1}")
                assert list(bank.tags()) == list(f.tags_positions(k + 1))
        assert (bank.flags() == 0).all() and f.assoc_fallbacks() == 0
        assert path_ran(f, both_paths)


# ---- 4: the edges of the walk --------------------------------------------------------------------------------------------------------
def test_edges_of_the_walk(sd):
    K = 3
    world, f = built_map(sd)
    lib = sd.load_library()
    with f, seeded(f, K) as a, seeded(f, K) as b:
        index, N = f.tag_index(), world.N
        frozen = hs.frozen_part(sd, f, 0)
        state0 = f.state()
        # an empty window: the prediction alone, `step` with m = 0
        before = hs.snapshot(a)
        got = pair_step(a, b, [], index, N, "an empty window")
        after = hs.snapshot(a)
        assert got == ({}, [], 0) and not np.array_equal(after.pose, before.pose) and np.array_equal(after.n_obs, before.n_obs)
        # unknown tags only
        world.move()
        got = pair_step(a, b, [(0.0, [ldw.det(1001, 0.3, 0.8), ldw.det(7, -0.1, 0.5), ldw.det(1001, 0.3, 0.8)])], index, N, "unknown tags only")
        assert got == ({}, [1001, 7], 0) and np.array_equal(hs.snapshot(a).n_obs, before.n_obs)
        # an ignored tag of the map
        world.move()
        a.set_association(1.5, [world.ids[2]])
        got = pair_step(a, b, world.window([2, 4, 2], 2), index, N, "an ignored tag of the map", ignore=(world.ids[2],))
        assert list(got[0]) == [index[world.ids[4]]] and got[1] == []
        a.set_association(1.5, [])
        # a detection beyond the gate: dropped, not unmatched
        world.move()
        win = world.window([1, 3], 1)
        win[0][1].insert(1, ldw.det(world.ids[5], 0.2, 1.6))
        got = pair_step(a, b, win, index, N, "a detection beyond the gate")
        assert list(got[0]) == [index[world.ids[1]], index[world.ids[3]]] and got[1] == []
        # a tag seen in three frames, among others seen once
        world.move()
        win = world.window([0], 3)
        win[1][1].append(ldw.det(world.ids[4], *world.camera(4)))
        got = pair_step(a, b, win, index, N, "a tag seen in three frames")
        assert list(got[0]) == [index[world.ids[0]], index[world.ids[4]]]
        # id -1 through the raw C entry: the flag, and the state of the clean window
        world.move()
        clean = world.window([3, 5], 2)
        count, ids, pt, pe, _ = a._pack_detections([clean])
        ids2, pt2, pe2 = np.insert(ids[0], 1, -1).astype(np.int32), np.insert(pt[0], 1, [0.1, 0.0, 0.7], axis=0), np.insert(pe[0], 1, 1e-3)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        assert lib.ekf_hypotheses_step_detections(a._h, LIN, ANG, int(count[0]) + 1, ids2.ctypes.data_as(ip),
                                                  np.ascontiguousarray(pt2).ctypes.data_as(dp), pe2.ctypes.data_as(dp)) == 0
        b.step_detections(LIN, ANG, clean)
        assert a.window_flags() == EKF_FLAG_ASSOC and b.window_flags() == 0 and a.tags() == b.tags() and len(a.tags()) == 2
        assert hs.same_snapshot(hs.snapshot(a), hs.snapshot(b)), "id -1: the state differs from the clean window's"
        assert (a.flags() == 0).all()                          # (the window's flag is not a hypothesis's)
        # 65 detections, the 65th an unknown tag: the chunk edge
        world.move()
        win = world.window([5, 2, 0, 3, 1], 13)
        assert sum(len(t) for _s, t in win) == 65
        win[12][1][4] = ldw.det(1001, 0.3, 0.8)
        got = pair_step(a, b, win, index, N, "65 detections")
        assert len(got[0]) == 5 and got[1] == [1001] and got[2] == 0
        # nothing of the source handle has moved, and the bank's map is still the handle's (adopt compares them bit for bit)
        assert hs.frozen_same(hs.frozen_part(sd, f, 0), frozen) and np.array_equal(f.state()[0], state0[0]) and f.tag_index() == index
        a.adopt(0, f)
        assert hs.frozen_same(hs.frozen_part(sd, f, 0), frozen)
        # ... nor its tag row: every tag still matches its landmark
        got = pair_step(a, b, world.window(list(range(N)), 1), index, N, "every tag")
        assert list(got[0]) == [index[world.ids[j]] for j in range(N)]


# ---- 5: two passes -------------------------------------------------------------------------------------------------------------------
def test_two_passes(sd):
    """17 known tags: the second pass applies the 17th.  A second pass on an EMPTY record: the plan counts a window's distinct ids,
    so it takes more than 16 of them with at most 16 matched -- 20 detections of 20 distinct ids, 5 of them known -- and ends as
    the same window cut to its 5 known detections, whose plan has one pass; 20 detections of 5 distinct tags (4 frames) plan
    one pass and are checked against `step` like any window."""
    N, K = 20, 3
    world, f = built_map(sd, N=N, n_max=3 + 2 * N, seed=9, options=[("small_state", 0)])
    with f, seeded(f, K) as a, seeded(f, K) as b:
        index = f.tag_index()
        world.move()
        which = [(3 * i + 1) % N for i in range(17)]
        assert len(set(which)) == 17
        before = hs.snapshot(a).n_obs
        got = pair_step(a, b, world.window(which, 2), index, N, "17 known tags")
        assert list(got[0]) == [index[world.ids[j]] for j in which] and got[2] == 0
        assert np.array_equal(hs.snapshot(a).n_obs, before + 17)
        world.move()
        pair_step(a, b, world.window([7, 1, 12, 19, 4], 4), index, N, "20 detections of 5 distinct tags")
        world.move()
        known = world.window([2, 9, 16, 5, 11], 1)
        full = [(known[0][0], list(known[0][1]))]
        for i in range(15):
            full[0][1].insert(1 + (i * 7) % (len(full[0][1])), ldw.det(950 + i, 0.03 * (i - 7), 0.8))
        assert len(full[0][1]) == 20 and len({t.tag_id for t in full[0][1]}) == 20
        a.step_detections(LIN, ANG, full)                      # planned: two passes, the second on an empty record
        b.step_detections(LIN, ANG, known)                     # planned: one
        assert a.tags() == b.tags() and len(a.tags()) == 5 and len(a.unmatched_tags()) == 15 and b.unmatched_tags() == []
        assert hs.same_snapshot(hs.snapshot(a), hs.snapshot(b)), "an empty second pass moved a hypothesis"


def test_thirty_three_known_tags(sd):
    N, K = 40, 3
    world, f = built_map(sd, N=N, n_max=3 + 2 * N, seed=21)
    with f, seeded(f, K) as a, seeded(f, K) as b:
        index = f.tag_index()
        world.move()
        which = [(7 * i + 2) % N for i in range(33)]
        assert len(set(which)) == 33
        before = hs.snapshot(a).n_obs
        got = pair_step(a, b, world.window(which, 1), index, N, "33 known tags")
        assert list(got[0]) == [index[world.ids[j]] for j in which[:EKF_AMAX]] and got[1] == [] and got[2] == EKF_FLAG_ASSOC
        assert np.array_equal(hs.snapshot(a).n_obs, before + EKF_AMAX)


# ---- 6: the bound rises on the device ------------------------------------------------------------------------------------------------
def test_bound_rises_over_a_matched_landmark(sd):
    """N = 40 with the bank's bound at 23; the window matches landmarks 2 and 35 (state indices 73, 74).  Hypothesis 0 keeps the
    seed (the map's own pose part), the others are reset; hypothesis 0 adopted into the source slot, then two SLAM steps that
    name landmark 35, agree with the dense model."""
    N, K = 40, 3
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
        assert not model[1][:3, 23:].any() and model[1][:3, 3:23].all()
        with f.hypotheses(K) as bank:
            bank.reset(seed_poses(f, K)[1:], SEED_COV, k=(1, K - 1))
            assert not bank.rows(0)[:, 23:].any() and bank.rows(0)[:, 3:23].all() and not bank.rows(1)[:, 3:].any()
            world.move()
            win = world.window([2, 35], 2)
            bank.step_detections(LIN, ANG, win)
            model, tags, _ = ldw.model_window(*model, index, win)
            assert list(tags) == list(bank.tags()) == [2, 35]
            for k in range(K):
                rows = bank.rows(k)
                assert rows[:, 73:75].all() and not rows[:, 75:].any(), f"hypothesis {k}: the bound did not rise to 75"
            bank.adopt(0, f)
        err = assert_state_close((*f.state(), index, f.flags()), (model[0], model[1], index), INIT_VAR, tol=TOL, entry_tol=TOL,
                                 what="hypothesis 0 adopted: ")
        print(f"hypothesis 0 adopted: {fmt_state(err)}")
        rng = np.random.default_rng(7)
        for lms in ([35, 3], [9, 35, 1]):
            d = model[0][3:].reshape(-1, 2)[lms] - model[0][:2]
            zr = np.hypot(d[:, 0], d[:, 1]) + rng.normal(0.0, 0.01, len(lms))
            zb = orc.wrap_pi(np.arctan2(d[:, 1], d[:, 0]) - model[0][2] + rng.normal(0.0, 0.01, len(lms)))
            f.step(LIN, ANG, lms, zr, zb)
            model = orc.ekf_step_dense(*model, LIN, ANG, np.array(lms, dtype=np.int32), zr, zb, ldw.CFG)
        f.flush()
        err = assert_state_close((*f.state(), index, f.flags()), (model[0], model[1], index), INIT_VAR, tol=TOL, entry_tol=TOL,
                                 what="two SLAM steps behind it: ")
        print(f"two SLAM steps behind it: {fmt_state(err)}")


# ---- 7: the NIS gate -----------------------------------------------------------------------------------------------------------------
def test_nis_gate_rejects_a_gross_outlier(sd):
    """tests/test_gpu_localize_detections.py's construction for every hypothesis near the truth: landmark 4 a quarter turn off its
    bearing; the gate is put between the outlier's NIS and the others', both taken from the dense model of each hypothesis."""
    K = 5
    world, f = built_map(sd)
    with f, f.hypotheses(K) as a, f.hypotheses(K) as b:
        poses = np.tile(f.mean()[:3], (K, 1))
        poses[:, 0] += 0.002 * np.arange(K)
        poses[:, 2] -= 0.001 * np.arange(K)
        cov = np.diag([0.01 ** 2, 0.01 ** 2, 0.01 ** 2])
        world.move()
        win = world.window([1, 4, 2], 1)
        keep = [(0.0, [win[0][1][0], win[0][1][2]])]
        t = win[0][1][1].pose_t.ravel()
        win[0][1][1] = ldw.det(world.ids[4], t[2], -t[0])
        good, bad = [], []
        for k in range(K):
            log = []
            ldw.model_window(*hm.reset_state(*f.state(), poses[k], cov), f.tag_index(), win, log=log)
            good += [log[0][3], log[2][3]]
            bad.append(log[1][3])
        gate = 0.5 * min(bad)
        assert max(good) < 0.5 * gate, (good, bad)
        for bank in (a, b):
            bank.reset(poses, cov)
            bank.set_nis_gate(gate)
        start = hs.snapshot(a)
        a.step_detections(LIN, ANG, win)
        b.step_detections(LIN, ANG, keep)
        got, want = hs.snapshot(a), hs.snapshot(b)
        assert (got.n_rej == 1).all() and (want.n_rej == 0).all() and (got.n_obs == 3).all() and (want.n_obs == 2).all()
        assert len(a.tags()) == 3 and len(b.tags()) == 2
        for name in ("pose", "blk", "rows"):
            assert np.array_equal(getattr(got, name), getattr(want, name)), f"{name}: the rejected outlier moved the state"
        assert not np.array_equal(got.pose, start.pose)        # the others are applied


# ---- 8: a stream of windows ----------------------------------------------------------------------------------------------------------
def stream_windows(world, N, long_window=True):
    """12 windows on the N = 20 map: one empty, one with an unknown tag and -- unless every window is to fit one pass -- one of 17 tags."""
    wins = []
    for s in range(12):
        world.move()
        which = [(3 * s + 7 * j) % N for j in range(3 + s % 3)]
        if s == 4:
            which = []
        if s == 2 and long_window:
            which = [(3 * i + 1) % N for i in range(17)]
        win = world.window(which, 1 + s % 2) if which else []
        if s == 7:
            win[0][1].insert(1, ldw.det(1001, 0.3, 0.8))
        wins.append(win)
    return wins


def draws(K, steps=12, seed=17):
    rng = np.random.default_rng(seed)
    return rng.random(steps), rng.standard_normal((steps, K, 3))


def spread(f, K):
    """Hypotheses far enough apart for the weights to become uneven: x up to 0.7 m off."""
    bank = f.hypotheses(K)
    poses = seed_poses(f, K)
    poses[:, 0] += 0.1 * (np.arange(K) % 8)
    bank.reset(poses, SEED_COV)
    return bank


def run_kw(fraction, split, u, z, first, count):
    return dict(fraction=fraction, split=split, u=u[first:first + count] if fraction > 0.0 else None,
                z=z[first:first + count] if split > 0.0 else None)


@pytest.mark.parametrize("policy", [(0.0, 0.0), (0.9, 0.3), (2.0, 0.3)])
def test_stream_is_the_host_loop(sd, policy):
    N, K = 20, 8
    fraction, split = policy
    world, f = built_map(sd, N=N, n_max=3 + 2 * N, seed=9, options=[("small_state", 0)])
    wins = stream_windows(world, N)
    lin = [LIN * (1.0 + 0.1 * (s % 3)) for s in range(12)]
    ang = [ANG if s % 4 else 0.005 for s in range(12)]
    u, z = draws(K)
    with f, spread(f, K) as a, spread(f, K) as b, spread(f, K) as c:
        loop_tags, loop_mix, fired = [], [], []
        for s in range(12):
            a.step_detections(lin[s], ang[s], wins[s])
            loop_tags.append(reported(a))
            loop_mix.append(a.mixture())
            kw = dict(u=u[s], split=split, z=z[s]) if split > 0.0 else dict(u=u[s])
            fired.append(fraction > 0.0 and a.resample_if(fraction, **kw) is not None)
        b.upload_detections(lin, ang, wins)
        b.log(12)
        b.run(0, 12, **run_kw(fraction, split, u, z, 0, 12))
        want = hs.snapshot(a)
        assert hs.same_snapshot(hs.snapshot(b), want), f"{policy}: run differs from the host loop"
        tr = b.trace()
        print(f"{policy}: resampled at steps {np.nonzero(tr.resampled)[0].tolist()}, ess {np.array2string(tr.ess, precision=2)}")
        assert np.array_equal(tr.resampled, np.array(fired))
        if fraction > 1.0:
            assert tr.resampled.all()
        for s in range(12):
            mix = loop_mix[s]
            assert np.array_equal(tr.mean[s], mix.mean) and np.array_equal(tr.cov[s], mix.cov), f"step {s}: the trace's row"
            assert (tr.ess[s], tr.evidence[s], tr.live[s], tr.best[s]) == (mix.ess, mix.evidence, mix.live, mix.best), f"step {s}"
            assert reported(b, s) == loop_tags[s], f"step {s}: tags(step) differs from the loop's tags()"
            why = hdm.judge(loop_tags[s], hdm.walk(wins[s], f.tag_index(), N))
            assert why is None, f"step {s}: {why}"
        assert len(loop_tags[2][0]) == 17 and loop_tags[4] == ({}, [], 0) and loop_tags[7][1] == [1001]
        assert (want.n_obs > 17).all() and np.isfinite(want.pose).all()
        # in two pieces
        c.upload_detections(lin, ang, wins)
        c.run(0, 5, **run_kw(fraction, split, u, z, 0, 5))
        c.run(5, 7, **run_kw(fraction, split, u, z, 5, 7))
        assert hs.same_snapshot(hs.snapshot(c), want), f"{policy}: two pieces differ from one run"


def test_detection_stream_is_the_index_stream_of_its_lists(sd):
    N, K = 20, 8
    fraction, split = 2.0, 0.3
    world, f = built_map(sd, N=N, n_max=3 + 2 * N, seed=9, options=[("small_state", 0)])
    wins = stream_windows(world, N, long_window=False)
    lin, ang = [LIN] * 12, [ANG] * 12
    u, z = draws(K)
    with f, spread(f, K) as d, spread(f, K) as e:
        e.upload_detections(lin, ang, wins)
        lists = [e.tags(step=s) for s in range(12)]
        assert max(len(t) for t in lists) <= 16 and min(len(t) for t in lists) == 0
        idx = [list(t) for t in lists]
        rng_ = [[t[k][2] for k in t] for t in lists]
        brg = [[t[k][3] for k in t] for t in lists]
        d.upload_stream(lin, ang, idx, rng_, brg)
        for bank in (d, e):
            bank.run(0, 12, **run_kw(fraction, split, u, z, 0, 12))
        assert hs.same_snapshot(hs.snapshot(e), hs.snapshot(d)), "the detection stream differs from the index stream of its lists"
        # an index stream afterwards replaces it and runs as before
        e.upload_stream(lin, ang, idx, rng_, brg)
        with pytest.raises(sd.EkfError, match="no such step"):
            e.tags(step=0)
        for bank in (d, e):
            bank.run(3, 6, **run_kw(fraction, split, u, z, 3, 6))
        assert hs.same_snapshot(hs.snapshot(e), hs.snapshot(d)), "the index stream that replaced it"


# ---- 9: errors change nothing --------------------------------------------------------------------------------------------------------
def test_errors_change_nothing(sd):
    K = 3
    world, f = built_map(sd)
    lib = sd.load_library()
    dp, ip, up = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_uint)
    with f, seeded(f, K) as bank:
        world.move()
        wins = [world.window([1, 4], 2), world.window([0, 3, 5], 1), world.window([2], 1)]
        ids, pt, pe = np.zeros(EKF_DMAX + 1, dtype=np.int32), np.tile([0.1, 0.0, 0.7], (EKF_DMAX + 1, 1)), np.zeros(EKF_DMAX + 1)
        ids[:] = world.ids[0]
        before = hs.snapshot(bank)

        def p(a, t=dp):
            return None if a is None else a.ctypes.data_as(t)

        def refused(call, code, why):
            assert call() == code, why
            assert why.encode() in lib.ekf_hyp_last_error(bank._h), (why, lib.ekf_hyp_last_error(bank._h))
            assert hs.same_snapshot(hs.snapshot(bank), before), why

        def step_rc(lin=LIN, ang=ANG, count=2, ids=ids, pt=pt, pe=pe):
            return lambda: lib.ekf_hypotheses_step_detections(bank._h, lin, ang, count, p(ids, ip), p(pt), p(pe))

        def tags_rc(step):
            m, fl = C.c_int(), C.c_uint()
            return lambda: lib.ekf_hypotheses_download_tags(bank._h, step, C.byref(m), None, None, None, None, None, None, None, C.byref(fl))
        refused(tags_rc(-1), EKF_ERR_STATE, "no window of detections has run")
        refused(tags_rc(0), EKF_ERR_STATE, "no such step")
        refused(tags_rc(-2), EKF_ERR_ARG, "step must be")
        refused(step_rc(ids=None), EKF_ERR_ARG, "NULL detection arrays")
        refused(step_rc(pt=None), EKF_ERR_ARG, "NULL detection arrays")
        refused(step_rc(pe=None), EKF_ERR_ARG, "NULL detection arrays")
        refused(step_rc(count=-1), EKF_ERR_ARG, "count must be")
        refused(step_rc(count=EKF_DMAX + 1), EKF_ERR_ARG, "count must be")
        for value in (np.nan, np.inf, -np.inf):
            refused(step_rc(lin=value), EKF_ERR_ARG, "non-finite lin / ang")
            refused(step_rc(ang=value), EKF_ERR_ARG, "non-finite lin / ang")
        refused(tags_rc(-1), EKF_ERR_STATE, "no window of detections has run")      # (a refused window is no window)
        refused(lambda: lib.ekf_hypotheses_set_association(bank._h, 1.5, None, 2), EKF_ERR_ARG, "at most 16 ignored tags")
        refused(lambda: lib.ekf_hypotheses_set_association(bank._h, 1.5, p(ids, ip), 17), EKF_ERR_ARG, "at most 16 ignored tags")
        assert step_rc(count=EKF_DMAX)() == 0 and len(bank.tags()) == 1             # the largest window is taken
        bank.reset(seed_poses(f, K), SEED_COV)
        # the upload's refusals; a stream survives them
        bank.upload_detections([LIN] * 3, [ANG] * 3, wins)
        kept = [reported(bank, s) for s in range(3)]
        lin3, ang3, cnt = np.full(3, LIN), np.full(3, ANG), np.array([2, 1, EKF_DMAX + 1], dtype=np.int32)
        ids3, pt3, pe3 = np.tile(ids, (3, 1)), np.tile(pt, (3, 1, 1)), np.tile(pe, (3, 1))

        def up_rc(steps=3, lin=lin3, ang=ang3, cnt=cnt, ids=ids3, pt=pt3, pe=pe3, stride=EKF_DMAX + 1):
            return lambda: lib.ekf_hypotheses_detections_upload(bank._h, steps, p(lin), p(ang), p(cnt, ip), p(ids, ip), p(pt), p(pe), stride)
        ok = np.array([2, 1, 0], dtype=np.int32)
        refused(up_rc(), EKF_ERR_ARG, "count must be")
        refused(up_rc(steps=-1), EKF_ERR_ARG, "steps must be")
        refused(up_rc(cnt=ok, lin=None), EKF_ERR_ARG, "NULL array")
        refused(up_rc(cnt=None), EKF_ERR_ARG, "NULL array")
        refused(up_rc(cnt=ok, ids=None), EKF_ERR_ARG, "NULL detection arrays")
        refused(up_rc(cnt=ok, stride=1), EKF_ERR_ARG, "count must be")
        refused(up_rc(cnt=ok, ang=np.array([ANG, ANG, np.nan])), EKF_ERR_ARG, "non-finite lin / ang")
        refused(tags_rc(3), EKF_ERR_STATE, "no such step")
        assert [reported(bank, s) for s in range(3)] == kept
        with seeded(f, K) as twin:
            for s in range(3):
                twin.step_detections(LIN, ANG, wins[s])
            bank.run(0, 3, fraction=0.0)
            assert hs.same_snapshot(hs.snapshot(bank), hs.snapshot(twin)), "the stream that survived the refusals"
        # no windows: the stream is freed
        bank.upload_detections([], [], [])
        before = hs.snapshot(bank)
        refused(lambda: lib.ekf_hypotheses_run(bank._h, 0, 1, 0.0, 0.0, None, None), EKF_ERR_STATE, "no stream uploaded")
    # a bank from a handle that never had a tag table
    with sd.EkfSlam(15, batch=1) as g:
        g.set_state_diag(np.concatenate([np.zeros(3), world.xy.ravel()]), np.full(15, 0.02))
        with g.hypotheses(K) as bank:
            before = hs.snapshot(bank)
            refused(step_rc(), EKF_ERR_STATE, "no tag table")
            refused(up_rc(cnt=ok), EKF_ERR_STATE, "no tag table")


def test_windows_beyond_the_device_raise(sd):
    world, f = built_map(sd)
    with f, seeded(f, 2) as bank:
        before = hs.snapshot(bank)
        with pytest.raises(ValueError, match="EKF_DMAX"):
            bank.step_detections(LIN, ANG, world.window([0, 1, 2, 3, 4, 5], 43))
        with pytest.raises(ValueError, match="outside"):
            bank.upload_detections([LIN, LIN], [ANG, ANG], [world.window([0], 1), [(0.0, [ldw.det(1024, 0.1, 0.7)])]])
        assert hs.same_snapshot(hs.snapshot(bank), before)


# ---- 10: the kidnapped robot from a log ----------------------------------------------------------------------------------------------
def test_kidnapped_robot_from_a_log(sd):
    """ldw.recovery_stream() through replay.relocalize with hdm.RELOC_K = 32 seeds from frontend.poses_on_circle (one sighting of
    landmark 0 where the robot is put down).  tests/test_hyp_detections_cpu.py shows that the model fleet meets the thresholds
    on this stream with this seed count -- without resampling, which is the policy asserted here (fraction 0); the default
    policy (fraction 0.5, split 0.5, a seeded generator) runs too and must report the same windows."""
    import slam_duckietown_amd.replay as rp
    case = hdm.reloc_case()
    res = rp.relocalize(case.steps, case.map, case.seeds, hdm.RELOC_SEED_COV, fraction=0.0, split=0.0, noise=ldw.RECOVERY_NOISE)
    try:
        mean, cov = res.filter.state()
        d2, err = ldw.mahalanobis(mean, cov, case.truth), float(np.linalg.norm(mean[:2] - case.truth[:2]))
        print(f"relocalize: best hypothesis {res.best}, Mahalanobis^2 {d2:.3f}, position error {err:.4f} m, ess {np.array2string(res.trace.ess, precision=2)}")
        assert res.windows == ldw.RECOVERY_WINDOWS == len(res.trace.ess) and not res.trace.resampled.any()
        assert all(len(t) == 4 for t in res.tags) and all(u == [] for u in res.unmatched)
        assert res.filter.tag_index() == case.map[2] and np.array_equal(res.filter.mean()[3:], case.map[0][3:])
        assert d2 < ldw.CHI2_3_0999 and err < 0.1 and res.filter.flags() == 0
        tags = res.tags
    finally:
        res.filter.close()
    # the same lap cut from an events log by the driver's windowing, under the default policy
    lines, t0 = [], 10.0                                       # window k: the events in (t0 + 0.7 (k - 1), t0 + 0.7 k]
    lines += [f"{t0:.3f},left_wheel,100", f"{t0:.3f},right_wheel,200"]
    for k, (lin, ang, win) in enumerate(case.steps):
        dets = [(t.tag_id, [float(v) for v in t.pose_t.ravel()], t.pose_err) for _s, fr in win for t in fr]
        lines.append(f"{t0 + 0.7 * k + 0.3:.3f},detections,{dets!r}")
        lines += [f"{t0 + 0.7 * (k + 1) + 0.05:.3f},left_wheel,100", f"{t0 + 0.7 * (k + 1) + 0.05:.3f},right_wheel,200"]
    res = rp.relocalize(lines, case.map, case.seeds, hdm.RELOC_SEED_COV, rng=np.random.default_rng(3), noise=ldw.RECOVERY_NOISE)
    try:
        assert res.windows >= ldw.RECOVERY_WINDOWS and np.isfinite(res.filter.mean()).all() and res.filter.flags() == 0
        assert [t for t in res.tags if t] == tags                # the same windows, the same bits
    finally:
        res.filter.close()
