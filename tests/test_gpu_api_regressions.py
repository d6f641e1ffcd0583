"""GPU regression tests of the host-side state tracking around the HIP path (round-1 advisor findings):
the drop-in's "is this what I returned?" test, the active bound of an uploaded stream, the limits of the
device-side association, argument validation that must not leave the handle half-updated."""
from types import SimpleNamespace as NS

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests import golden_util as gu
from tests.gpu_support import close, sd, tag  # noqa: F401

pytestmark = pytest.mark.gpu

REL_TOL = 1e-6
TIGHT = 1e-9


def test_drop_in_sees_in_place_edits_of_returned_arrays(sd, both_paths):
    """The caller owns the arrays EKF_pose_estimation returned and may edit them IN PLACE (a pose reset, a wrapped
    angle, an inflated landmark-landmark entry far from the pose block): the next call must start from the edited
    values like the reference does (src/replay_no_ros.py:229-237 passes them straight back in)."""
    from slam_duckietown_amd import ekf_bindings as eb
    g = gu.load("replay_default")
    mean = np.array([0.0, 0.0, 0.0])
    cov = np.eye(3) * 0.1
    ti, oti = {}, {}
    ocfg = orc.EkfConfig()
    omean, ocov = mean.copy(), cov.copy()
    edits = 0
    for k in range(16):
        det = gu.detections_for_step(g, k)
        mean, cov, _ = eb.EKF_pose_estimation(g["ang"][k], g["lin"][k], mean, cov, 0.7, det, ti)
        omean, ocov, _ = orc.ekf_pose_estimation_dense(g["ang"][k], g["lin"][k], omean, ocov, 0.7, det, oti, ocfg)
        close(mean, omean)
        close(cov, ocov)
        n = len(mean)
        if k % 3 == 1:                               # same objects, new contents
            mean[2] = mean[2] + 0.25
            omean[2] = omean[2] + 0.25
            edits += 1
        if k % 4 == 2 and n >= 9:                    # an entry the old diag + pose-rows sample never looked at
            i, j = n - 1, n - 4
            cov[i, j] += 0.125
            cov[j, i] += 0.125
            ocov[i, j] += 0.125
            ocov[j, i] += 0.125
            edits += 1
    assert edits >= 6


def test_drop_in_beyond_the_small_records_uploads_and_recycles_buffers(sd):
    """A state beyond 131 x 131: the drop-in keeps no record of what it returned and uploads every call (in-place edits of
    the returned arrays are simply what gets uploaded), and the covariances it returns are views of recycled pinned
    buffers (`ekf_host_alloc`): an array the caller still holds must never be handed out again, one the caller dropped is."""
    import gc
    from slam_duckietown_amd import ekf_bindings as eb
    N, m, calls = 80, 6, 15                                 # (the last call is not one that is edited afterwards)
    mean0, diag0, lin, ang, idx, zr, zb = orc.synthetic_stream(N, calls, m, 5)
    ti, oti = {1000 + i: i for i in range(N)}, {1000 + i: i for i in range(N)}
    ocfg = orc.EkfConfig()
    mean, cov = mean0.copy(), np.diag(diag0)
    omean, ocov = mean0.copy(), np.diag(diag0)
    held = []
    for k in range(calls):
        xr, yr = zr[k] * np.cos(zb[k]), zr[k] * np.sin(zb[k])
        det = [(float(k), [NS(tag_id=1000 + int(i), pose_R=np.eye(3), pose_t=np.array([[-y], [0.0], [x]]), pose_err=0.0)
                           for i, x, y in zip(idx[k], xr, yr)])]
        mean, cov, _ = eb.EKF_pose_estimation(ang[k], lin[k], mean, cov, 0.7, det, ti)
        omean, ocov, _ = orc.ekf_pose_estimation_dense(ang[k], lin[k], omean, ocov, 0.7, det, oti, ocfg)
        close(mean, omean)
        close(cov, ocov)
        assert cov.flags.writeable and np.array_equal(cov, cov.T)
        if k % 4 == 1:                                      # in-place edits far from the pose block, and of the mean
            cov[40, 40] *= 1.25
            ocov[40, 40] *= 1.25
            mean[2] += 0.01
            omean[2] += 0.01
        if k < 5:
            held.append((cov, cov.copy()))                  # the caller keeps these: their buffers stay theirs
    for arr, copy in held:
        assert np.array_equal(arr, copy)
    assert eb._drop.filt.size() == 3 + 2 * N and eb._drop.mean_copy is None
    nbytes = 8 * (3 + 2 * N) ** 2
    live_before = eb._pinned.live
    assert live_before >= 6 * nbytes                        # five held + the current one, all backed by the pool
    del held, arr, copy
    gc.collect()
    assert len(eb._pinned.free.get(nbytes, [])) == eb._pinned.KEEP and eb._pinned.live < live_before
    kept = set(eb._pinned.free[nbytes])
    P2 = eb._drop.filt.covariance()                         # the next large array comes out of the pool
    assert len(eb._pinned.free[nbytes]) == eb._pinned.KEEP - 1 and P2.ctypes.data in kept
    close(P2, ocov)


def test_drop_in_trust_identity_is_opt_in_for_large_states(sd):
    """`DROP_IN_TRUST_IDENTITY`: beyond 131 x 131 the default uploads every call -- an in-place edit of
    the returned covariance is seen, like the reference (src/replay_no_ros.py:229-237 passes the arrays straight back) --; with
    the switch on, a call that gets the very objects the previous call returned skips the upload: unedited arrays give the
    oracle's results with no upload at all, an in-place edit is (documentedly) NOT seen, and FRESH arrays are still uploaded."""
    from slam_duckietown_amd import ekf_bindings as eb
    N, m, calls = 80, 6, 8
    mean0, diag0, lin, ang, idx, zr, zb = orc.synthetic_stream(N, calls, m, 9)
    ocfg = orc.EkfConfig()

    def dets(k):
        xr, yr = zr[k] * np.cos(zb[k]), zr[k] * np.sin(zb[k])
        return [(float(k), [NS(tag_id=1000 + int(i), pose_R=np.eye(3), pose_t=np.array([[-y], [0.0], [x]]), pose_err=0.0)
                            for i, x, y in zip(idx[k], xr, yr)])]

    uploads = []
    real_set_state = eb.EkfSlam.set_state

    def counting_set_state(self, *a, **kw):
        uploads.append(1)
        return real_set_state(self, *a, **kw)

    eb.EkfSlam.set_state = counting_set_state
    try:
        for trusted in (False, True):
            eb.DROP_IN_TRUST_IDENTITY = trusted
            ti, oti = {1000 + i: i for i in range(N)}, {1000 + i: i for i in range(N)}
            mean, cov = mean0.copy(), np.diag(diag0)
            omean, ocov = mean0.copy(), np.diag(diag0)
            del uploads[:]
            for k in range(calls):
                mean, cov, _ = eb.EKF_pose_estimation(ang[k], lin[k], mean, cov, 0.7, dets(k), ti)
                omean, ocov, _ = orc.ekf_pose_estimation_dense(ang[k], lin[k], omean, ocov, 0.7, dets(k), oti, ocfg)
                close(mean, omean)
                close(cov, ocov)
            assert len(uploads) == (1 if trusted else calls)        # (the first call's arrays are the caller's own)
            # an in-place edit far from the pose block, then one more call
            k = 0
            cov[-1, -1] *= 1.5
            seen_cov = ocov.copy()
            seen_cov[-1, -1] *= 1.5
            m2, c2, _ = eb.EKF_pose_estimation(ang[k], lin[k], mean, cov, 0.7, dets(k), ti)
            want_seen = orc.ekf_pose_estimation_dense(ang[k], lin[k], omean, seen_cov, 0.7, dets(k), dict(oti), ocfg)
            want_unseen = orc.ekf_pose_estimation_dense(ang[k], lin[k], omean, ocov, 0.7, dets(k), dict(oti), ocfg)
            close(c2, want_unseen[1] if trusted else want_seen[1])
            assert orc.rel_fro(c2, (want_seen if trusted else want_unseen)[1]) > 1e-6      # the two really differ
            # fresh arrays (copies) are uploaded whatever the switch says
            n_up = len(uploads)
            m3, c3, _ = eb.EKF_pose_estimation(ang[1], lin[1], np.array(m2), np.array(c2), 0.7, dets(1), ti)
            assert len(uploads) == n_up + 1
            w3 = orc.ekf_pose_estimation_dense(ang[1], lin[1], m2, c2, 0.7, dets(1), dict(oti), ocfg)
            close(c3, w3[1])
    finally:
        eb.EkfSlam.set_state = real_set_state
        eb.DROP_IN_TRUST_IDENTITY = False


def test_uploaded_stream_follows_later_state_changes(sd):
    """ekf_stream_upload bakes the active bound that follows from the stream's own observations; a dense upload, a
    second run of the same stream or a toggled option between upload and run must still give the dense reference
    result (the bound is completed at run time)."""
    N, steps, m = 120, 12, 4
    mean0, diag0, lin, ang, idx, zr, zb = orc.synthetic_stream(N, steps, m, 21)
    idx = idx % 30                                   # the stream itself only ever observes landmarks 0..29
    for k in range(steps):
        assert len(set(idx[k].tolist())) == m
    n = len(mean0)
    cfg = orc.EkfConfig()
    rng = np.random.default_rng(2)
    A = rng.normal(size=(n, 6)) * 0.4
    Pd = A @ A.T + np.diag(rng.uniform(0.5, 1.5, n))      # dense: everything correlated with everything

    def oracle_run(mu, P, k0, k1):
        for k in range(k0, k1):
            mu, P = orc.ekf_step_dense(mu, P, lin[k], ang[k], idx[k], zr[k], zb[k], cfg)
        return mu, P

    with sd.EkfSlam(n) as f:
        # 1. upload on a diagonal state, then replace the state by a dense one, then run
        f.set_state_diag(mean0, diag0)
        f.stream_upload(lin, ang, idx, zr, zb)
        f.set_state(mean0, Pd)
        f.stream_run(0, steps)
        mu, P = f.state()
        om, oP = oracle_run(mean0.copy(), Pd.copy(), 0, steps)
        close(mu, om)
        close(P, oP)
        # 2. run the first half of the same stream again on the state it left behind
        f.stream_run(0, 6)
        mu, P = f.state()
        om, oP = oracle_run(om, oP, 0, 6)
        close(mu, om)
        close(P, oP)
        # 3. the option changes after the upload
        f.set_option("active_bound", 0)
        f.stream_run(6, 6)
        f.set_option("active_bound", 1)
        f.stream_run(0, 3)
        mu, P = f.state()
        om, oP = oracle_run(om, oP, 6, 12)
        om, oP = oracle_run(om, oP, 0, 3)
        close(mu, om)
        close(P, oP)
        # 4. a state that lacks the stream's landmarks is refused, not indexed out of range
        f.set_state(mean0[:3 + 2 * 10], Pd[:23, :23])
        with pytest.raises(sd.EkfError):
            f.stream_run(0, 1)


def test_step_interleaved_with_predict_dense_keeps_the_bound(sd):
    """A general dense F correlates every state with every other: steps after ekf_predict_dense must treat the
    whole state as active, whatever the observations so far said."""
    N, steps, m = 60, 6, 4
    mean0, diag0, lin, ang, idx, zr, zb = orc.synthetic_stream(N, steps, m, 5)
    idx = idx % 10
    n = len(mean0)
    cfg = orc.EkfConfig()
    rng = np.random.default_rng(8)
    F = np.eye(n) + rng.normal(size=(n, n)) * 0.02
    Q = np.eye(n) * 0.01
    om, oP = mean0.copy(), np.diag(diag0)
    with sd.EkfSlam(n) as f:
        f.set_state_diag(mean0, diag0)
        f.stream_upload(lin, ang, idx, zr, zb)
        f.stream_run(0, 3)
        f.predict_dense(F, Q)
        f.stream_run(3, 3)
        mu, P = f.state()
    for k in range(3):
        om, oP = orc.ekf_step_dense(om, oP, lin[k], ang[k], idx[k], zr[k], zb[k], cfg)
    oP = F @ oP @ F.T + Q
    for k in range(3, 6):
        om, oP = orc.ekf_step_dense(om, oP, lin[k], ang[k], idx[k], zr[k], zb[k], cfg)
    close(mu, om)
    close(P, oP)


def test_rejected_update_leaves_the_handle_untouched(sd):
    """A duplicate index anywhere in a long list (also across the 16-landmark device passes) is refused before any
    handle state changes: the following valid steps still match the reference."""
    N = 40
    mean0, diag0, lin, ang, idx, zr, zb = orc.synthetic_stream(N, 4, 20, 13)
    cfg = orc.EkfConfig()
    om, oP = mean0.copy(), np.diag(diag0)
    with sd.EkfSlam(len(mean0), batch=2) as f:
        for b in range(2):
            f.set_state_diag(mean0, diag0, b)
        bad = idx[0].copy()
        bad[18] = bad[2]                              # the repeat sits in the second device pass
        with pytest.raises(sd.EkfError):
            f.step([lin[0]] * 2, [ang[0]] * 2, [idx[0], bad], [zr[0]] * 2, [zb[0]] * 2)
        far = idx[0].copy()
        far[19] = N                                   # outside the state, trajectory 1 only
        with pytest.raises(sd.EkfError):
            f.step([lin[0]] * 2, [ang[0]] * 2, [idx[0], far], [zr[0]] * 2, [zb[0]] * 2)
        for k in range(4):
            f.step([lin[k]] * 2, [ang[k]] * 2, [idx[k][:6]] * 2, [zr[k][:6]] * 2, [zb[k][:6]] * 2)
            om, oP = orc.ekf_step_dense(om, oP, lin[k], ang[k], idx[k][:6], zr[k][:6], zb[k][:6], cfg)
        for b in range(2):
            mu, P = f.state(b)
            close(mu, om)
            close(P, oP)


def _raw_step_detections(sd, f, lin, ang, tags):
    """The C entry point itself (one trajectory, one frame), past EkfSlam.step_detections' host-side check of the
    device front end's limits."""
    import ctypes as C
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    count = np.array([len(tags)], dtype=np.int32)
    ids = np.array([[t.tag_id for t in tags]], dtype=np.int32)
    pt = np.array([[np.asarray(t.pose_t, dtype=np.float64).ravel()[:3] for t in tags]])
    pe = np.array([[t.pose_err for t in tags]], dtype=np.float64)
    la, aa = np.array([lin]), np.array([ang])
    return sd.load_library().ekf_step_detections(f._h, la.ctypes.data_as(dp), aa.ctypes.data_as(dp), count.ctypes.data_as(ip),
                                                 ids.ctypes.data_as(ip), pt.ctypes.data_as(dp), pe.ctypes.data_as(dp), len(tags))


def test_device_association_drops_before_indexing(sd):
    """The C ABI's device front end with 33 distinct tags in one window (EKF_AMAX = 32): the 33rd is dropped BEFORE it is
    given a landmark index (no uninitialised landmark enters the state), the sticky flag is raised and tags_positions()
    reports it.  (`EkfSlam.step_detections` checks the limits on the host and never sends such a window: next test.)"""
    tags = [tag(100 + i, -0.4 + 0.025 * i, 0.6 + 0.01 * i) for i in range(33)]
    with sd.EkfSlam(3 + 2 * 40) as f:
        assert _raw_step_detections(sd, f, 0.01, 0.0, tags) == 0
        assert f.size() == 3 + 2 * 32
        assert f.tag_index() == {100 + i: i for i in range(32)}
        assert f.flags() & 2
        with pytest.raises(sd.EkfError):
            f.tags_positions()
        mu = f.mean()
        assert np.isfinite(mu).all() and (np.abs(mu[3:]) > 0).any()


def test_normal_mode_window_stays_on_the_device(sd, both_paths):
    """VERDICT r05 item 4.  The reference's NORMAL mode hands EKF_pose_estimation a 0.7 s window of every camera frame
    (src/replay_no_ros.py:17, :280-337): 21 frames x 6 tags = 126 detections of 6 distinct tags -- beyond the 64 detections the
    device front end took until round 5.  Now it stays on the device: no host fallback counted, EKF_FLAG_ASSOC clear, the
    tags_positions record, TAG_INDEX, mean and covariance of `oracle.ekf_pose_estimation_dense`; then a window with 20 distinct
    tags (two update passes of up to 16 landmarks), repeated detections, one tag beyond the gate (:289) and an ignored one
    (:286); both kernel paths."""
    from tests.conftest import path_ran
    rng = np.random.default_rng(21)
    cfg = orc.EkfConfig(ignore_tags=(55,))
    ids_a = [7, 3, 19, 11, 2, 30]
    ids_b = [40 + i for i in range(14)] + ids_a            # 20 distinct, 14 of them new
    base = {i: (float(rng.uniform(-0.5, 0.5)), float(rng.uniform(0.4, 1.1))) for i in set(ids_a + ids_b)}

    def window(ids, frames, k, extra=()):
        out = []
        for fr in range(frames):
            order = list(ids) if fr % 2 == 0 else list(ids)[::-1]              # the order within a frame wanders
            tags = [tag(int(i), base[i][0] + float(rng.normal(0, 0.004)), base[i][1] + float(rng.normal(0, 0.004))) for i in order]
            if fr == 1:
                tags += list(extra)
            out.append((k + fr / 30.0, tags))
        return out

    wins = [window(ids_a, 21, 0.0), window(ids_b, 5, 1.0, extra=(tag(777, 1.4, 1.4), tag(55, 0.1, 0.5))),
            window(ids_a[::-1], 21, 2.0)]
    assert sum(len(t) for _s, t in wins[0]) == 126
    with sd.EkfSlam(3 + 2 * 24) as f:
        f.set_association(cfg.gate_range, cfg.ignore_tags)
        om, oP, oti = np.zeros(3), np.eye(3) * 0.1, {}
        for k, w in enumerate(wins):
            lin, ang = 0.004, (0.02 if k % 2 else 0.005)
            f.step_detections(lin, ang, w)
            om, oP, otags = orc.ekf_pose_estimation_dense(ang, lin, om, oP, 0.7, w, oti, cfg)
            got = f.tags_positions()
            assert list(got.keys()) == list(otags.keys())
            for j in otags:
                assert got[j][3] == otags[j][3]
                assert np.allclose([got[j][q] for q in (0, 1, 4, 5)], [otags[j][q] for q in (0, 1, 4, 5)], rtol=0, atol=1e-12)
            assert f.tag_index() == oti and f.flags() == 0
            mu, P = f.state()
            close(mu, om)
            close(P, oP)
        assert f.assoc_fallbacks() == 0 and not f._host_tags and len(oti) == 20 and 777 not in oti and 55 not in oti
        assert path_ran(f, both_paths)


def test_step_detections_beyond_the_device_limits(sd):
    """The reference's dictionaries are unbounded (src/replay_no_ros.py:280-301).  `EkfSlam.step_detections` on windows the
    device front end cannot take -- tag ids beyond 1024 (here among 20 distinct tags and 100 detections) -- associates
    on the host instead, with the same results as the reference-shaped oracle (`associate` + augmentation + dense step);
    windows that fit go to the device again once the table can hold the map; a window mixing both kinds of id keeps the
    host in charge.  Two trajectories, so that one over-limit window takes the whole call."""
    rng = np.random.default_rng(12)
    cfg = orc.EkfConfig()

    def window(ids, frames, k):
        """`frames` frames, every tag in each (repeated detections are averaged, :315), one beyond the gate, one twice."""
        out = []
        for fr in range(frames):
            tags = [tag(int(i), float(base_x[i] + rng.normal(0, 0.004)), float(base_z[i] + rng.normal(0, 0.004))) for i in ids]
            if fr == 0:
                tags.append(tag(777, 1.4, 1.4))                   # 1.98 m away: gated (:289), never indexed
            out.append((k + 0.1 * fr, tags))
        return out

    all_ids = [3, 1500, 7, 2047, 11, 1024, 5, 9, 4000, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71]
    base_x = {i: float(rng.uniform(-0.5, 0.5)) for i in all_ids}
    base_z = {i: float(rng.uniform(0.4, 1.1)) for i in all_ids}
    small = [i for i in all_ids if i < 1024]
    plan = [
        (small[:5], 2),            # fits the device: 5 tags, 12 detections
        (all_ids[:20], 5),         # 20 distinct tags, 101 detections -- the device would take those since round 6 -- but ids >= 1024: host
        (small[2:9], 3),           # would fit the device -- but the map now holds ids the device table cannot: host
        (all_ids[4:24], 5),        # 20 tags again, four of them new
    ]
    with sd.EkfSlam(3 + 2 * 40, batch=2) as f:
        om = [np.zeros(3), np.zeros(3)]
        oP = [np.eye(3) * 0.1, np.eye(3) * 0.1]
        oti = [{}, {}]
        for k, (ids, frames) in enumerate(plan):
            wins = [window(ids, frames, k), window(ids[::-1], frames, k)]            # trajectory 1 sees them in reverse order
            lin, ang = 0.004, (0.02 if k % 2 else 0.005)
            f.step_detections(lin, ang, wins)
            for b in range(2):
                om[b], oP[b], otags = orc.ekf_pose_estimation_dense(ang, lin, om[b], oP[b], 0.7, wins[b], oti[b], cfg)
                got = f.tags_positions(b)
                assert list(got.keys()) == list(otags.keys())
                for j in otags:
                    assert got[j][3] == otags[j][3]
                    assert np.allclose([got[j][q] for q in (0, 1, 4, 5)], [otags[j][q] for q in (0, 1, 4, 5)], rtol=0, atol=1e-12)
                assert f.tag_index(b) == oti[b]
                mu, P = f.state(b)
                assert f.flags(b) == 0 and len(mu) == 3 + 2 * len(oti[b])
                close(mu, om[b])
                close(P, oP[b])
        assert len(oti[0]) == 24 and 777 not in oti[0]
        # a map the handle cannot hold is refused before anything is enqueued
        more = [tag(5000 + i, 0.01 * i, 0.5) for i in range(20)]
        before = [f.state(b) for b in range(2)]
        with pytest.raises(sd.EkfError, match="capacity"):
            f.step_detections(0.004, 0.02, [[(9.0, more)], [(9.0, more)]])
        for b in range(2):
            assert np.array_equal(f.state(b)[1], before[b][1]) and f.size(b) == len(before[b][0])
    # below the limits and with small ids the device path is the one that runs (the host overlay is dropped again)
    with sd.EkfSlam(3 + 2 * 40) as f:
        w17 = [(0.0, [tag(100 + i, -0.4 + 0.025 * i, 0.6 + 0.01 * i) for i in range(33)])]
        f.step_detections(0.004, 0.02, w17)                          # 33 tags (> EKF_AMAX): host, then the device table follows
        assert f.flags() == 0 and f.size() == 3 + 2 * 33 and not f._host_index and f.assoc_fallbacks() == 1
        w3 = [(1.0, [tag(100 + i, -0.4 + 0.025 * i, 0.61 + 0.01 * i) for i in (2, 32, 5)] + [tag(300, 0.2, 0.9)])]
        om, oP, oti = np.zeros(3), np.eye(3) * 0.1, {}
        om, oP, _ = orc.ekf_pose_estimation_dense(0.02, 0.004, om, oP, 0.7, w17, oti, cfg)
        f.step_detections(0.004, 0.02, w3)                           # device path: the table it was handed knows all 33
        assert not f._host_tags and f.assoc_fallbacks() == 1
        om, oP, ot = orc.ekf_pose_estimation_dense(0.02, 0.004, om, oP, 0.7, w3, oti, cfg)
        assert f.tag_index() == oti and list(f.tags_positions().keys()) == list(ot.keys())
        mu, P = f.state()
        close(mu, om)
        close(P, oP)


def test_gpu_backend_device_association_beyond_the_device_limits(sd, both_paths):
    """replay.GpuBackend(device_association=True) against the host-association backend on windows the device
    front end cannot take alone: more than EKF_AMAX = 32 distinct tags in a window, and a map that outgrows the capacity."""
    from slam_duckietown_amd.replay import GpuBackend
    rng = np.random.default_rng(4)
    windows = []
    for k in range(10):
        count = 36 if k in (2, 6) else 5
        ids = rng.choice(60, size=count, replace=False)
        tags = [tag(int(i), float(rng.uniform(-0.5, 0.5)), float(rng.uniform(0.4, 1.2))) for i in ids]
        windows.append([(float(k), tags)])
    res = []
    for dev in (False, True):
        be = GpuBackend(capacity=3 + 2 * 20, device_association=dev)     # 20 landmarks: regrowth needed
        be.set_state(np.zeros(3), np.eye(3) * 0.1)
        ti = {}
        for k, w in enumerate(windows):
            be.step(0.02 if k % 2 else 0.004, 0.004, w, ti)
        res.append(be.state() + (dict(ti), be.filt.flags()))
        be.close()
    assert res[0][2] == res[1][2] and res[1][3] == 0
    close(res[1][0], res[0][0])
    close(res[1][1], res[0][1])
    # and the host path itself is the reference's: the oracle's dense EKF_pose_estimation on the same windows
    om, oP, oti = np.zeros(3), np.eye(3) * 0.1, {}
    cfg = orc.EkfConfig()
    for k, w in enumerate(windows):
        om, oP, _ = orc.ekf_pose_estimation_dense(0.02 if k % 2 else 0.004, 0.004, om, oP, 0.7, w, oti, cfg)
    assert oti == res[0][2]
    close(res[0][0], om)
    close(res[0][1], oP)


def _snapshot(sd, f, b=0):
    """P_base, V, W and the mean the next step reads, raw (development hook ekf_debug_snapshot: no flush, no check)."""
    import ctypes as C
    lib = sd.load_library()
    out = []
    for which in (0, 1, 2, 3):
        count = lib.ekf_debug_snapshot(f._h, b, which, None, 0)
        assert count > 0
        a = np.empty(count)
        assert lib.ekf_debug_snapshot(f._h, b, which, a.ctypes.data_as(C.POINTER(C.c_double)), count) == count
        out.append(a)
    return out


def test_single_launch_step_wait_is_bounded(sd):
    """The panel workgroups of the single-launch step wait for their trajectory's solve on a device-scope word.  With
    the diagnostic setting `fused_step=2` the solve never publishes it: every wait must run into its bound and let the
    launch finish (no hang) WITHOUT writing anything -- P_base, V, W and the mean stay bit for bit what they were --
    and raise EKF_FLAG_INTERNAL, which every call that hands results to the host reports as an error (EKF_ERR_STATE)
    until the trajectory is uploaded again."""
    from slam_duckietown_amd import ekf_bindings as eb
    N = 40
    mean0, diag0, lin, ang, idx, zr, zb = orc.synthetic_stream(N, 4, 4, 3)
    with sd.EkfSlam(len(mean0)) as f:
        f.set_option("active_bound", 0)            # every panel workgroup takes part (none is "beyond the bound")
        f.set_state_diag(mean0, diag0)
        for k in range(2):                         # two good steps: ranks are pending, V and W hold data
            f.step(lin[k], ang[k], idx[k], zr[k], zb[k])
        f.sync()
        before = _snapshot(sd, f)
        f.set_option("fused_step", 2)
        f.step(lin[2], ang[2], idx[2], zr[2], zb[2])
        with pytest.raises(sd.EkfError, match="EKF_FLAG_INTERNAL"):
            f.sync()
        assert f.flags(0) & eb.EKF_FLAG_INTERNAL   # (reading the flags stays possible: that is how the trajectory is found)
        for name, a, b in zip(("P_base", "V", "W"), before, _snapshot(sd, f)):
            assert np.array_equal(a, b, equal_nan=True), f"{name} changed although the step timed out"
        # the mean the failed step READ is untouched (the handle has moved on to the other buffer, where the solve
        # workgroup -- which ran -- left its entries at C)
        import ctypes as C
        lib = sd.load_library()
        mu_read = np.empty(len(before[3]))
        assert lib.ekf_debug_snapshot(f._h, 0, 4, mu_read.ctypes.data_as(C.POINTER(C.c_double)), len(mu_read)) == len(mu_read)
        assert np.array_equal(mu_read, before[3])
        for call in (f.state, f.mean, f.covariance, lambda: f.covariance_block(0, 0, 3, 3)):
            with pytest.raises(sd.EkfError, match="EKF_FLAG_INTERNAL"):
                call()
        # recovery as documented: upload the trajectory again, two-launch (or healthy single-launch) steps from there
        f.set_option("fused_step", 1)
        f.set_state_diag(mean0, diag0)
        assert not f.flags(0) & eb.EKF_FLAG_INTERNAL
        om, oP = mean0.copy(), np.diag(diag0)
        cfg = orc.EkfConfig()
        for k in range(3):
            f.step(lin[k], ang[k], idx[k], zr[k], zb[k])
            om, oP = orc.ekf_step_dense(om, oP, lin[k], ang[k], idx[k], zr[k], zb[k], cfg)
        mu, P = f.state()
        assert orc.rel_fro(mu, om) < 1e-9 and orc.rel_fro(P, oP) < 1e-9
    # the same for the throughput shape (k_panels_split: the counter travels with the mailbox)
    N, B = 1200, 16
    streams = [orc.synthetic_stream(N, 2, 8, 80 + t) for t in range(B)]
    with sd.EkfSlam(3 + 2 * N, batch=B) as f:
        f.set_option("active_bound", 0)
        for b, s in enumerate(streams):
            f.set_state_diag(s[0], s[1], b)
        args = lambda k: ([s[2][k] for s in streams], [s[3][k] for s in streams], [s[4][k] for s in streams],
                          [s[5][k] for s in streams], [s[6][k] for s in streams])
        f.step(*args(0))
        f.sync()
        before = _snapshot(sd, f, 5)
        f.set_option("fused_step", 2)
        f.step(*args(1))
        with pytest.raises(sd.EkfError, match="EKF_FLAG_INTERNAL"):
            f.sync()
        assert all(f.flags(b) & eb.EKF_FLAG_INTERNAL for b in range(B))
        for name, a, b in zip(("P_base", "V", "W"), before, _snapshot(sd, f, 5)):
            assert np.array_equal(a, b, equal_nan=True), f"{name} changed although the step timed out"
        with pytest.raises(sd.EkfError, match="trajectory 5"):
            f.mean(5)

@pytest.mark.parametrize("n_lm,batch,which", [(70, 1, 0), (300, 2, 1), (2100, 1, 0)])
def test_download_into_pinned_memory_by_kernel_equals_the_copy(sd, n_lm, batch, which):
    """A whole state downloaded into pinned host memory is written by a kernel (k_pack_dense: mirrored on the way, no copy
    engine) up to 40 MB, by the mirror pass + the runtime's rectangle copy beyond and into ordinary memory: the same bytes
    either way -- with ranks pending (the download applies them first), for a trajectory that is not the first, for a size that
    is no multiple of the 64 x 64 tile and on the column-panel layout (n = 4203 > 4096)."""
    import ctypes as C
    lib = sd.load_library()
    n = 3 + 2 * n_lm
    streams = [orc.synthetic_stream(n_lm, 3, 8, 20 + t) for t in range(batch)]
    with sd.EkfSlam(n, batch=batch) as f:
        f.set_option("small_state", 0)
        for t, s in enumerate(streams):
            f.set_state_diag(s[0], s[1], t)
        for k in range(3):                                   # three steps: 48 ranks pending, no pass yet
            f.step([s[2][k] for s in streams], [s[3][k] for s in streams], [s[4][k] for s in streams],
                   [s[5][k] for s in streams], [s[6][k] for s in streams])
        out = {}
        for mode in (2, 0, 1):
            f.set_option("pack_dense", mode)
            before = lib.ekf_debug_dense_packs(f._h)
            mu, P = f.state(which)                           # (the binding's array: a recycled pinned buffer)
            assert P.base is not None
            took_kernel = lib.ekf_debug_dense_packs(f._h) - before
            assert took_kernel == (1 if mode == 2 or (mode == 1 and 8 * n * n <= 40 << 20) else 0)
            out[mode] = (mu, P)
        plain_mu, plain_P = np.empty(n), np.empty((n, n))    # ordinary memory: never the kernel
        f.set_option("pack_dense", 2)
        before = lib.ekf_debug_dense_packs(f._h)
        dp = C.POINTER(C.c_double)
        assert lib.ekf_download_state(f._h, which, plain_mu.ctypes.data_as(dp), plain_P.ctypes.data_as(dp), n) == 0
        assert lib.ekf_debug_dense_packs(f._h) == before
        for mode in (2, 1):
            assert np.array_equal(out[mode][0], out[0][0]) and np.array_equal(out[mode][1], out[0][1])
        assert np.array_equal(plain_P, out[0][1]) and np.array_equal(plain_P, plain_P.T)
        om, oP = streams[which][0].copy(), np.diag(streams[which][1])
        for k in range(3):
            s = streams[which]
            om, oP = orc.ekf_step_structured(om, oP, s[2][k], s[3][k], s[4][k], s[5][k], s[6][k], orc.EkfConfig())
        close(plain_mu, om)
        close(plain_P, oP)


@pytest.mark.parametrize("m,steps_per_pass", [(5, 7), (12, 3), (8, 5), (3, 13), (1, 40)])
def test_online_steps_are_charged_the_ranks_they_append(sd, m, steps_per_pass):
    """`EkfSlam.step` (landmark indices not known in advance: the per-step kernels) charges a step 2 ranks per landmark of its
    busiest trajectory -- not the rank slots of the kernel instantiation that ran it (1 / 2 / 4 / 8 / 16 landmarks) -- and
    flushes when the NEXT step's writes would not fit 80 ranks: m = 5: 7 steps per covariance pass (until round 4: 5),
    m = 12: 3 (2), m = 3: 13 (10).  Counted with the pass profiler; the state against the oracle."""
    N, B = 120, 2
    steps = 2 * steps_per_pass + 1
    streams = [orc.synthetic_stream(N, steps, m, 900 + t) for t in range(B)]
    cfg = orc.EkfConfig()
    with sd.EkfSlam(3 + 2 * N, batch=B) as f:
        f.set_option("active_bound", 0)
        for b, s in enumerate(streams):
            f.set_state_diag(s[0], s[1], b)
        f.profile_enable(True)
        for k in range(steps):
            f.step([s[2][k] for s in streams], [s[3][k] for s in streams], [s[4][k] for s in streams],
                   [s[5][k] for s in streams], [s[6][k] for s in streams])
        f.sync()
        _, launches = f.profile_read()
        assert launches == 2, (launches, m)                    # two full passes, the last step still pending
        for b, s in enumerate(streams):
            mu, P = f.state(b)
            om, oP = s[0].copy(), np.diag(s[1])
            for k in range(steps):
                om, oP = orc.ekf_step_dense(om, oP, s[2][k], s[3][k], s[4][k], s[5][k], s[6][k], cfg)
            close(mu, om)
            close(P, oP)
            assert f.flags(b) == 0


def test_a_bank_s_observations_as_arrays_equal_the_lists(sd):
    """`step` / `update` / `step_state` take a whole bank's observations as [batch, m] arrays (one block copy each instead of one
    per trajectory): the same state, bit for bit, as the lists of per-trajectory lists."""
    B, N = 5, 30
    streams = [orc.synthetic_stream(N, 4, 6, 90 + t) for t in range(B)]
    with sd.EkfSlam(3 + 2 * N, batch=B) as f, sd.EkfSlam(3 + 2 * N, batch=B) as g:
        for h in (f, g):
            for t, s in enumerate(streams):
                h.set_state_diag(s[0], s[1], t)
        for k in range(4):
            lin, ang = np.array([s[2][k] for s in streams]), np.array([s[3][k] for s in streams])
            idx, zr, zb = (np.stack([s[i][k] for s in streams]) for i in (4, 5, 6))
            if k == 2:
                f.update(idx, zr, zb)
                g.update(list(idx), list(zr), list(zb))
            elif k == 3:
                mu, P = f.step_state(lin, ang, idx, zr, zb, b=3)
                g.step(lin, ang, [list(r) for r in idx], [list(r) for r in zr], [list(r) for r in zb])
                mu2, P2 = g.state(3)
                assert np.array_equal(mu, mu2) and np.array_equal(P, P2)
            else:
                f.step(lin, ang, idx, zr, zb)
                g.step(lin, ang, list(idx), list(zr), list(zb))
        for t in range(B):
            a, b = f.state(t), g.state(t)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        with pytest.raises(ValueError):
            f.step(lin, ang, idx[:3], zr[:3], zb[:3])


# every name ekf_set_option accepts and its allowed range (include/ekfslam_hip.h)
OPTION_RANGES = {
    "flush_every": (0, 64), "rank_limit": (2, 80), "pass_kernel": (-1, 2), "pass_chunk": (0, 4096),
    "pass_workgroups": (0, 4096), "pass_rows_per_block": (0, 4096), "pass_streaming": (-1, 1), "active_bound": (0, 1),
    "small_state": (0, 1), "fused_step": (0, 2), "fused_cadence": (0, 1), "col_gather": (0, 1), "w_from_v": (0, 1),
    "panel_shape": (0, 3), "lookahead": (0, 1), "chain": (0, 1), "panel_tform": (0, 1), "run_end_flush": (0, 1),
    "pack_dense": (0, 2), "fetch_spin": (0, 1), "fetch_verify": (0, 1), "profile_kernels": (0, 1), "profile_stride": (1, 1024),
}


def test_handle_churn_leaves_nothing_behind(sd):
    """Twelve handles at N = 100 x 2, created and closed one after another: each takes over the stream pair its predecessor
    parked and allocates afresh what that one released when it was deleted -- every first-use buffer of the handle is switched
    on: device association (one window), both log rings (5 steps, resized to 3, then off), the NIS gate, the noise table
    (set twice in a row: the second upload waits for the first to leave the staging copy), one removal, one direct update,
    one fork, a 30-step uploaded stream.  Every handle ends in the first one's state and flags, bit for bit."""
    from slam_duckietown_amd.ekf_bindings import EKF_DIRECT_POSE
    N_cap, N, B, m, steps = 100, 96, 2, 8, 30
    streams = [orc.synthetic_stream(N, steps, m, 9100 + t) for t in range(B)]
    args = tuple(np.stack([s[i] for s in streams], axis=1) for i in (2, 3, 4, 5, 6))
    window = [(0.0, [tag(500 + i, -0.3 + 0.2 * i, 0.6 + 0.05 * i) for i in range(3)])]

    def life():
        with sd.EkfSlam(3 + 2 * N_cap, batch=B) as f:
            f.set_option("small_state", 0)
            for b in range(B):
                f.set_state_diag(streams[b][0], streams[b][1], b)
            f.log_innovations(5)
            f.log_poses(5)
            f.set_nis_gate(threshold=40.0)
            f.set_noise([0.1, 0.13], [0.7, 0.8])
            f.set_noise([0.11, 0.12], [0.75, 0.7])
            f.step_detections(0.01, 0.005, [window] * B)           # three new tags: 99 landmarks
            assert f.assoc_fallbacks() == 0 and [f.size(b) for b in range(B)] == [3 + 2 * (N + 3)] * B
            f.log_innovations(3)
            f.log_poses(3)
            f.remove_landmarks([5, N + 1], b=None)
            pose = np.stack([f.mean(b)[:3] for b in range(B)])
            got = f.update_direct([[EKF_DIRECT_POSE]] * B, [[pose[b] + [0.01, -0.02, 0.005]] for b in range(B)],
                                  [[np.diag([0.01, 0.01, 0.002])]] * B)
            assert got.applied.all()
            f.fork(0, 1)
            f.run_stream(*args)
            assert f.innovations().m.shape[0] == 3 and f.pose_steps == steps
            f.log_innovations(0)
            f.log_poses(0)
            return [f.state(b) for b in range(B)], [f.flags(b) for b in range(B)], f.gate_counts()

    first = life()
    assert [mu.shape[0] for mu, _P in first[0]] == [3 + 2 * (N + 1)] * B
    assert not np.array_equal(first[0][0][1], first[0][1][1])      # (the twins diverge again over the stream)
    for _ in range(11):
        out, flags, rejected = life()
        assert flags == first[1] and np.array_equal(rejected, first[2])
        for b in range(B):
            assert np.array_equal(out[b][0], first[0][b][0]) and np.array_equal(out[b][1], first[0][b][1])


def test_set_option_ranges_and_removed_names(sd):
    """ekf_set_option accepts both ends of every option's range and refuses the values just beyond them with an error that
    names the option; `pass_kernel` = 1 (a removed form) is refused too.  Names of options that no longer exist are unknown."""
    with sd.EkfSlam(23) as f:
        for name, (lo, hi) in OPTION_RANGES.items():
            f.set_option(name, lo)
            f.set_option(name, hi)
            for bad in (lo - 1, hi + 1) + ((1,) if name == "pass_kernel" else ()):
                with pytest.raises(sd.EkfError, match=name):
                    f.set_option(name, bad)
        for name in ("panel_own_gate", "pre_positions", "pass_share_order", "zero_copy_inputs", "lookahead_min_mb",
                     "beside_min_mb"):
            with pytest.raises(sd.EkfError, match="unknown option " + name):
                f.set_option(name, 0)


def test_update_tables_grow_with_the_calls_on_one_handle(sd):
    """ekf_update_linear's table is sized by the call (its row cap and H's columns) and shares its buffer with
    ekf_update_direct's: a handle whose FIRST call is the smallest (one row over the pose) must serve the largest ones
    (32 rows over 16 landmarks, then 33 direct rows) afterwards.  The twin sees the largest shape first -- a call under a
    gate nothing passes: rejected, so nothing of it moves -- and then the same three calls: same bits."""
    from tests import update_cases as uc
    small, large = uc.linear_case("n40", 0, 1, 0, "z"), uc.linear_case("n40", 0, 32, 16, "z")
    fix = uc.direct_case("n40", 0, 33)

    def bank():
        s = uc.stream("n40", 0)
        f = sd.EkfSlam(len(s[0]), batch=1)
        f.set_state_diag(s[0], s[1])
        f.stream_upload(*[np.stack([s[i]], 1) for i in range(2, 7)])
        f.stream_run(0, uc.steps_of("n40"))
        return f

    def calls(f):
        res = [f.update_linear(lms, H, R, z=z, b=0) for lms, H, R, z in (small, large)] + [f.update_direct(*fix)]
        return res, f.state()

    with bank() as f, bank() as twin:
        lms, H, R, z = large
        assert not twin.update_linear(lms, H, R, z=z, gate=1e-300, b=0).applied[0]
        (got, state), (want, twin_state) = calls(f), calls(twin)
    assert [r.dof[0] for r in got] == [1, 32, 33] and all(r.applied[0] for r in got)
    assert [r.nis[0] for r in got] == [r.nis[0] for r in want]
    assert np.array_equal(state[0], twin_state[0]) and np.array_equal(state[1], twin_state[1])
