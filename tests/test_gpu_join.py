"""GPU: map joining on the device (ekf_join_maps, EkfSlam.join; k_join in csrc/ekf_join.hip) against tests/join_model.py.

Tolerance against the model: entrywise |got - ref| <= 1e-13 x bound, bound = |J| |P_in| |J|^T for the covariance and
|t| + |R| |l| for the mean.  An entry is at most 13 two-factor products, so its forward error is below gamma_20 ~ 2.2e-15
of the bound, the device's sin / cos add about 1e-15: 1e-13 is roughly 25 x headroom over a derived 4e-15.  What a join
only moves, or leaves, is compared bit for bit.  Runs that go on are compared with the oracle at the project's TIGHT."""
import ctypes as C

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests import join_model as jm
from tests.conftest import path_ran
from tests.gpu_support import col, raw00, same, sd, tag, within_bounds  # noqa: F401
from tests.streams import FRAME, stream_from

pytestmark = pytest.mark.gpu

TIGHT = 1e-10          # the project's bar for a run against the oracle (tests/test_gpu_remove_landmarks.py)
TOL = 1e-13            # x the entrywise bound (see above)
EKF_ERR_ARG, EKF_ERR_STATE = -1, -3


def mapped(sd, N, n_max, steps, m, seed, general=False, batch=1, online=0):
    """A filter whose covariance is dense: `steps` steps of a synthetic stream over N landmarks (every trajectory of a bank from
    a slightly different start), then `online` single steps -- which leave their ranks pending."""
    f = sd.EkfSlam(n_max, batch=batch)
    if general:
        f.set_option("small_state", 0)
    if N == 0:                                                     # (one trajectory: predictions only)
        for _ in range(steps + online):
            f.step(0.004, 0.02, [], [], [])
        return f
    s = orc.synthetic_stream(N, steps + online, m, seed)
    for b in range(batch):
        f.set_state_diag(s[0] + 0.01 * b, s[1], b)
    rep = lambda x: np.repeat(x[:steps, None], batch, 1)
    if steps:
        f.run_stream(*[rep(a) for a in s[2:]])
    for k in range(steps, steps + online):
        obs = [s[4][k], s[5][k], s[6][k]] if batch == 1 else [[s[4][k]] * batch, [s[5][k]] * batch, [s[6][k]] * batch]
        f.step(s[2][k], s[3][k], *obs)
    return f


def check_model(got, A, B, T=None, cT=None, label=""):
    """`got` against the dense model of joining state B to state A; prints the worst ratio to the bound before it asserts."""
    xm, Pm, bound, mbound = jm.join_dense(A[0], A[1], B[0], B[1], T, cT)
    within_bounds(got, xm, Pm, bound, mbound, TOL, label)
    return xm, Pm


# ---- 1: the smallest joins, both paths ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sequential", "explicit"])
def test_smallest(sd, both_paths, mode):
    T, cT = (None, None) if mode == "sequential" else FRAME
    with mapped(sd, 0, 5, 2, 0, 0) as a, mapped(sd, 1, 5, 6, 1, 31) as b, mapped(sd, 2, 7, 6, 2, 32) as a2, \
            mapped(sd, 0, 3, 2, 0, 0) as b0:
        A, B, A2, B0 = a.state(), b.state(), a2.state(), b0.state()
        r = a.join(b, transform=T, cov=cT)                         # N_A = 0 + N_B = 1
        assert (r.first, r.count, r.twins.tolist()) == (0, 1, [-1]) and a.size() == 5 and a.flags() == 0
        check_model(a.state(), A, B, T, cT, f"0 + 1 {mode} {both_paths}")
        assert same(b.state(), B)
        r = a2.join(b0, transform=T, cov=cT)                       # N_A = 2 + N_B = 0
        assert (r.first, r.count, r.twins.tolist()) == (2, 0, []) and a2.size() == 7 and a2.flags() == 0
        if mode == "explicit":
            assert same(a2.state(), A2)                            # a no-op, bit for bit
        else:
            got = a2.state()
            check_model(got, A2, B0, label=f"2 + 0 sequential {both_paths}")
            assert np.array_equal(got[1][3:, 3:], A2[1][3:, 3:]) and not np.array_equal(got[0][:3], A2[0][:3])
        for f in (a, b, a2, b0):
            f.step(0.004, 0.02, [], [], [])
            assert path_ran(f, both_paths)


# ---- 2: tile edges on the general kernels, ranks pending on both sides ----------------------------------------------------
@pytest.mark.parametrize("NA,NB", [(30, 1), (30, 33), (31, 1), (31, 33)])
@pytest.mark.parametrize("mode", ["sequential", "explicit"])
def test_tile_edges_with_ranks_pending(sd, NA, NB, mode):
    """n_A = 63 / 65 around the 64-column edge; the source's n_max (ld = 128) differs from the destination's (ld = 256)."""
    T, cT = (None, None) if mode == "sequential" else FRAME
    mk_a = lambda: mapped(sd, NA, 3 + 2 * 70, 12, 7, 40 + NA, general=True, online=1)
    mk_b = lambda: mapped(sd, NB, 3 + 2 * 40, 12, min(7, NB), 50 + NB, general=True, online=1)
    with mk_a() as a, mk_b() as b, mk_a() as ta, mk_b() as tb:
        A, B = ta.state(), tb.state()                              # the twins' downloads: what the join must start from
        assert raw00(sd, a) != A[1][0, 0] and raw00(sd, b) != B[1][0, 0]      # ranks are pending on both sides at the call
        assert path_ran(a, "general_kernels") and path_ran(b, "general_kernels")
        r = a.join(b, transform=T, cov=cT)
        assert (r.first, r.count) == (NA, NB) and a.size() == 3 + 2 * (NA + NB) and a.flags() == 0
        got = a.state()
        check_model(got, A, B, T, cT, f"{NA} + {NB} {mode}")
        assert np.array_equal(got[1][3:3 + 2 * NA, 3:3 + 2 * NA], A[1][3:, 3:]) and np.array_equal(got[0][3:3 + 2 * NA], A[0][3:])
        assert same(b.state(), B)


# ---- 3: what is bit for bit ------------------------------------------------------------------------------------------------
def test_bit_for_bit_properties(sd):
    NA, NB = 31, 33
    nA, n_max = 3 + 2 * NA, 3 + 2 * 70

    def empty(batch=1, n=n_max):
        f = sd.EkfSlam(n, batch=batch)
        f.set_option("small_state", 0)
        return f

    with mapped(sd, NA, n_max, 12, 7, 71, general=True) as a, empty() as e, empty() as z, empty(3) as a3, empty(3) as c3, \
            mapped(sd, NB, 3 + 2 * 40, 12, 7, 72, general=True) as b, empty(3, 3 + 2 * 40) as b3:
        A, B = a.state(), b.state()
        for f, slot in ((e, 0), (z, 0), (a3, 0), (c3, 2)):         # bit-exact copies of `a` (ekf_copy_trajectories)
            f.copy_from(a, 0, slot)
            assert same(f.state(slot), A)
        a3.copy_from(a3, 0, 1)
        b3.copy_from(b, [0, 0], [0, 2])
        assert same(b3.state(2), B) and b3.size(1) == 3
        a.join(b)                                                  # sequential
        got = a.state()
        assert np.array_equal(got[1][3:nA, 3:nA], A[1][3:, 3:]) and np.array_equal(got[0][3:nA], A[0][3:])
        assert not np.array_equal(got[1][:3, :nA], A[1][:3]) and np.array_equal(got[1], got[1].T)
        e.join(b, transform=FRAME[0], cov=FRAME[1])                # explicit: A stays, the cross block is exactly zero
        ge = e.state()
        assert np.array_equal(ge[1][:nA, :nA], A[1]) and np.array_equal(ge[0][:nA], A[0])
        assert not ge[1][:nA, nA:].any() and not ge[1][nA:, :nA].any() and np.array_equal(ge[1], ge[1].T)
        assert ge[1][nA:, nA:].all()
        z.join(b, transform=np.zeros(3), cov=np.zeros((3, 3)))     # the identity frame: the source's landmarks, moved
        gz = z.state()
        assert np.array_equal(gz[1][nA:, nA:], B[1][3:, 3:]) and np.array_equal(gz[0][nA:], B[0][3:])
        assert np.array_equal(gz[1][:nA, :nA], A[1]) and not gz[1][:nA, nA:].any()
        assert same(b.state(), B)                                  # the source is not written
        # the same pair alone (above), as pair 0 of 3 (a3) and as pair 2 of 3 (c3)
        a3.join(b3, [0, 1, 2], [0, 1, 2])
        c3.join(b3, [0, 1, 2], [0, 1, 2])
        assert same(a3.state(0), got) and same(c3.state(2), got)
        assert a3.size(1) == nA and not same(a3.state(2), got) and c3.size(0) == 3 + 2 * NB


# ---- 4: banks ---------------------------------------------------------------------------------------------------------------
def test_banks_and_slots(sd):
    with mapped(sd, 20, 3 + 2 * 60, 10, 5, 81, general=True, batch=4) as d, mapped(sd, 9, 3 + 2 * 12, 8, 3, 82, batch=2) as s:
        D, S = [d.state(b) for b in range(4)], [s.state(b) for b in range(2)]
        r = d.join(s, [1, 0, 1], [0, 3, 2])                        # source 1 feeds destinations 0 and 2
        assert r.first.tolist() == [20, 20, 20] and r.count.tolist() == [9, 9, 9] and (r.twins == -1).all()
        for sb, db in ((1, 0), (0, 3), (1, 2)):
            assert d.size(db) == 3 + 2 * 29 and d.flags(db) == 0
            check_model(d.state(db), D[db], S[sb], label=f"bank {sb} -> {db}")
        assert same(d.state(1), D[1]) and d.size(1) == 43          # the untouched slot
        assert all(same(s.state(b), S[b]) for b in range(2))
        D0, D2 = d.state(0), d.state(2)
        r = d.join(d, 1, 0, transform=FRAME[0], cov=FRAME[1])      # inside one handle: slot 1 -> slot 0
        assert (r.first, r.count) == (29, 20) and d.size(0) == 3 + 2 * 49 and d.size(1) == 43
        check_model(d.state(0), D0, D[1], *FRAME, label="slots 1 -> 0")
        assert same(d.state(1), D[1]) and same(d.state(2), D2) and d.flags(0) == 0


# ---- 5: across the column-panel boundary ---------------------------------------------------------------------------------------
def test_across_the_panel_boundary(sd):
    """Destination n_max = 4203 (ld = 4224, two column panels), n_A = 4063, N_B = 40: the appended columns straddle column 4096."""
    NA, NB = 2030, 40
    nA = 3 + 2 * NA
    rng = np.random.default_rng(5)
    U = rng.normal(size=(nA, 8)) * 0.2
    PA = U @ U.T + np.diag(rng.uniform(0.5, 2.0, nA))
    xA = np.r_[0.3, -0.2, 0.9, rng.uniform(-2.0, 2.0, 2 * NA)]
    with sd.EkfSlam(4203) as a, mapped(sd, NB, 3 + 2 * NB, 12, 7, 91, general=True) as b:
        a.set_state(xA, PA)
        A, B = a.state(), b.state()
        r = a.join(b)
        assert (r.first, r.count) == (NA, NB) and a.size() == nA + 2 * NB and a.flags() == 0
        got = a.state()
    xm, Pm = jm.join_closed(A[0], A[1], B[0], B[1])
    bound = jm.join_closed(A[0], A[1], B[0], B[1], bound=True)[1]
    mbound = jm.join_mean(A[0], B[0])[1]
    new = np.r_[0:3, nA:nA + 2 * NB]                               # the pose rows and the new rows / columns
    for sl in (np.ix_(new, np.arange(nA + 2 * NB)), np.ix_(np.arange(nA + 2 * NB), new)):
        e = np.abs(got[1][sl] - Pm[sl])
        print("panel boundary: worst covariance error / bound", float(np.max(e / np.where(bound[sl] > 0, bound[sl], 1.0))))
        assert (e <= TOL * bound[sl]).all()
    assert (np.abs(got[0] - xm) <= TOL * mbound).all()
    assert np.array_equal(got[1][3:nA, 3:nA], A[1][3:, 3:]) and np.array_equal(got[0][3:nA], A[0][3:])   # the rest: bit for bit
    assert np.array_equal(got[1], got[1].T) and np.abs(got[1][4090:4100, 4090:4100]).min() > 0.0


# ---- 6: the filter goes on -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NA,NB,n_max,small", [(60, 40, 203, False), (10, 8, 39, True)])
def test_the_filter_goes_on(sd, NA, NB, n_max, small):
    """After a sequential join the stream uploaded BEFORE it (it observes the destination's own landmarks) still runs, then 40
    steps of a new stream over both parts -- against the oracle started from the joined download."""
    cfg = orc.EkfConfig()
    nA = 3 + 2 * NA

    def oracle(state, st):
        om, oP = state
        for k in range(len(st[0])):
            om, oP = orc.ekf_step_structured(om, oP, st[0][k], st[1][k], st[2][k], st[3][k], st[4][k], cfg)
        return om, oP

    with mapped(sd, NA, n_max, 20, 6, 101, general=not small) as a, mapped(sd, NB, 3 + 2 * NB, 20, 6, 102, general=not small) as b:
        A, B = a.state(), b.state()
        xm = jm.join_mean(A[0], B[0])[0]
        old = stream_from(xm[:nA], 10, 8, 103)                     # from the joined pose, over the destination's landmarks
        a.stream_upload(*[col(x) for x in old])
        with pytest.raises(sd.EkfError, match="outside the current state"):
            a.stream_upload(*[col(x) for x in stream_from(xm, (NA + NB) // 8 + 1, 8, 104)])    # (the appended landmarks do not exist yet)
        cad0 = a.cadence_counters()[0]
        a.join(b)
        joined = a.state()
        check_model(joined, A, B, label=f"{NA} + {NB} before the run")
        a.stream_run(0, 10)                                        # the stream uploaded before the join
        mid = oracle(joined, old)
        new = stream_from(mid[0], 40, 8, 105)                      # observes landmarks of both parts
        assert new[2].max() == NA + NB - 1 and new[2].min() == 0
        a.stream_upload(*[col(x) for x in new])
        a.stream_run(0, 40)
        got = a.state()
        assert a.flags() == 0 and path_ran(a, "default_path" if small else "general_kernels")
        if not small:
            print("cadences after the join:", a.cadence_counters()[0] - cad0)
            assert a.cadence_counters()[0] > cad0                  # cadences are formed
    om, oP = oracle(mid, new)
    print("after 10 + 40 steps: mean", orc.rel_fro(got[0], om), "covariance", orc.rel_fro(got[1], oP))
    assert orc.rel_fro(got[0], om) < TIGHT and orc.rel_fro(got[1], oP) < TIGHT


# ---- 7: the submapping recipe end to end ------------------------------------------------------------------------------------


def test_submapping_recipe(sd):
    """A local small-state filter maps from AprilTag detections (device association), is joined into the global filter, is
    restarted at the origin, maps again -- two tags of the first submap among its six -- and is joined again; then the
    reported twins are fused."""
    cfg, rng = orc.EkfConfig(), np.random.default_rng(17)
    ids = [int(i) for i in rng.permutation(500)[:10]]
    world = {i: np.array([rng.uniform(0.3, 1.0), rng.uniform(-0.5, 0.5)]) for i in ids}
    truth = np.zeros(3)
    origin = np.zeros(3)                                           # the local frame's origin in the world

    def window(k, win_ids):
        c, s = np.cos(truth[2]), np.sin(truth[2])
        tags = []
        for i in win_ids:
            d = world[i] - truth[:2]
            xr, yr = c * d[0] + s * d[1] + rng.normal(0, 0.004), -s * d[0] + c * d[1] + rng.normal(0, 0.004)
            tags.append(tag(i, -yr, xr))
        return [(float(k), tags)]

    with sd.EkfSlam(3 + 2 * 8) as loc, sd.EkfSlam(3 + 2 * 12) as glob:
        gm, gP, gti = glob.state() + ({},)
        for part, win_ids in enumerate((ids[:6], ids[4:10])):
            om, oP, oti = np.zeros(3), np.eye(3) * 0.1, {}
            for k in range(30):
                truth, _ = orc.motion_model(truth, 0.004, 0.02, cfg)
                win = window(k, win_ids)
                loc.step_detections(0.004, 0.02, win)
                tags = orc.associate(win, oti, om, cfg)
                om, oP = orc.augment(om, oP, len(oti), tags, cfg)
                order = list(tags.keys())
                om, oP = orc.ekf_step_dense(om, oP, 0.004, 0.02, order, [tags[i][4] for i in order], [tags[i][5] for i in order], cfg)
            assert loc.assoc_fallbacks() == 0 and path_ran(loc, "default_path") and loc.tag_index() == oti
            NA = (len(gm) - 3) // 2
            r = glob.join(loc)
            want = [gti.get(t, -1) for t, _ in sorted(oti.items(), key=lambda kv: kv[1])]
            print("submap", part, "twins", r.twins.tolist())
            assert (r.first, r.count) == (NA, 6) and r.twins.tolist() == want
            assert sorted(j for j in want if j >= 0) == ([] if part == 0 else [4, 5])
            for t, j in oti.items():
                gti.setdefault(t, NA + j)
            assert glob.tag_index() == gti
            gm, gP = jm.join_closed(gm, gP, om, oP)
            loc.set_state_diag(np.zeros(3), np.full(3, 0.1))        # restart the local filter at the origin
            loc.set_tag_index({})
            assert loc.size() == 3 and loc.tag_index() == {}
        got = glob.state()
        print("recipe: mean", orc.rel_fro(got[0], gm), "covariance", orc.rel_fro(got[1], gP))
        assert orc.rel_fro(got[0], gm) < TIGHT and orc.rel_fro(got[1], gP) < TIGHT and glob.flags() == 0
        assert glob.size() == 3 + 2 * 12
        pairs = [(int(i), r.first + j) for j, i in enumerate(r.twins) if i >= 0]
        assert len(pairs) == 2
        for i, j in pairs:                                         # a twin lies where its first copy does, to the filter's accuracy
            assert np.linalg.norm(got[0][3 + 2 * i:5 + 2 * i] - got[0][3 + 2 * j:5 + 2 * j]) < 0.5
        glob.constrain_landmarks([i for i, _ in pairs], [j for _, j in pairs], np.zeros(2), 1e-8 * np.eye(2), b=0)
        glob.remove_landmarks([j for _, j in pairs])
        assert glob.size() == 3 + 2 * 10 and glob.factor(0).info == 0 and glob.flags() == 0
        assert glob.tag_index() == {t: (j if j < 6 else j - 2) for t, j in gti.items()} and len(gti) == 10


# ---- 8: errors -------------------------------------------------------------------------------------------------------------
def test_bad_arguments_change_nothing(sd):
    lib = sd.load_library()
    with mapped(sd, 4, 3 + 2 * 14, 6, 4, 111, batch=3) as f, mapped(sd, 6, 3 + 2 * 6, 6, 3, 112, batch=2) as g, \
            mapped(sd, 10, 3 + 2 * 12, 6, 5, 113) as tight:
        F, G, Tt = [f.state(b) for b in range(3)], [g.state(b) for b in range(2)], tight.state()

        def unchanged():
            return all(same(f.state(b), F[b]) and f.size(b) == 11 for b in range(3)) and same(tight.state(), Tt) and \
                all(same(g.state(b), G[b]) and g.size(b) == 15 for b in range(2))

        ints = lambda *v: (C.c_int * len(v))(*v)
        dbl = lambda *v: (C.c_double * len(v))(*v)
        T0, C0 = dbl(0.1, 0.2, 0.3), dbl(0.01, 0, 0, 0, 0.01, 0, 0, 0, 0.01)
        call = lambda d, s, k, T=None, cT=None, twin=None, ts=0: lib.ekf_join_maps(f._h, d, g._h, s, k, T, cT, None, twin, ts)
        assert call(None, None, -1) == EKF_ERR_ARG and unchanged()                               # k < 0
        assert call(None, ints(0), 1) == EKF_ERR_ARG and call(ints(0), None, 1) == EKF_ERR_ARG and unchanged()   # NULL arrays
        for d, s in ((3, 0), (-1, 0), (0, 2), (0, -1)):                                          # an index outside its bank
            assert call(ints(d), ints(s), 1) == EKF_ERR_ARG and unchanged(), (d, s)
        assert call(ints(1, 1), ints(0, 1), 2) == EKF_ERR_ARG and unchanged()                    # a destination twice
        assert b"named twice" in lib.ekf_last_error(f._h)
        assert lib.ekf_join_maps(f._h, ints(0), f._h, ints(0), 1, None, None, None, None, 0) == EKF_ERR_ARG      # s == d
        assert lib.ekf_join_maps(f._h, ints(0, 1), f._h, ints(1, 2), 2, None, None, None, None, 0) == EKF_ERR_ARG
        assert b"both a source and a destination" in lib.ekf_last_error(f._h) and unchanged()
        with pytest.raises(sd.EkfError, match="n_max"):                                          # 10 + 6 above n_max (12 landmarks)
            tight.join(g)
        assert unchanged() and tight.size() == 23
        assert call(ints(0), ints(0), 1, T0, None) == EKF_ERR_ARG and call(ints(0), ints(0), 1, None, C0) == EKF_ERR_ARG   # one of T / covT
        assert unchanged()
        for bad_T, bad_C in ((dbl(np.nan, 0, 0), C0), (dbl(0, 0, np.inf), C0), (T0, dbl(np.nan, 0, 0, 0, 1, 0, 0, 0, 1)),
                             (T0, dbl(-1e-9, 0, 0, 0, 1, 0, 0, 0, 1)), (T0, dbl(1, 1.01, 0, 0, 1, 0, 0, 0, 1))):
            assert call(ints(0), ints(0), 1, bad_T, bad_C) == EKF_ERR_ARG and unchanged()
        twin = ints(*([7] * 8))
        assert call(ints(0), ints(0), 1, None, None, twin, 5) == EKF_ERR_ARG and unchanged()      # twin_stride below N_B
        if sd.device_count() > 1:                                                                 # different devices
            with sd.EkfSlam(3 + 2 * 6, device=1) as far:
                with pytest.raises(sd.EkfError, match="different devices"):
                    f.join(far)
                assert unchanged()
        assert call(None, None, 0) == 0 and unchanged()                                          # k = 0
        r = f.join(g, 1, 2)                                        # and both handles are usable afterwards
        assert (r.first, r.count) == (4, 6) and f.size(2) == 23 and same(g.state(1), G[1])
        check_model(f.state(2), F[2], G[1], label="after the refusals")
        assert same(f.state(0), F[0]) and same(f.state(1), F[1])


def test_a_failed_source_is_refused(sd):
    """A source, or a destination, under EKF_FLAG_INTERNAL (the diagnostic "fused_step" = 2: the bounded wait of a single-launch
    step times out) gives EKF_ERR_STATE, and the other handle's state stays bit for bit."""
    from slam_duckietown_amd import ekf_bindings as eb
    lib = sd.load_library()
    s = orc.synthetic_stream(50, 2, 8, 121)
    with sd.EkfSlam(3 + 2 * 60) as bad, mapped(sd, 4, 3 + 2 * 60, 4, 2, 122, general=True) as good:
        bad.set_option("active_bound", 0)
        bad.set_state_diag(s[0], s[1])
        bad.step(s[2][0], s[3][0], s[4][0], s[5][0], s[6][0])
        bad.sync()
        bad.set_option("fused_step", 2)
        bad.step(s[2][1], s[3][1], s[4][1], s[5][1], s[6][1])
        G = good.state()
        one = (C.c_int * 1)(0)
        assert lib.ekf_join_maps(good._h, one, bad._h, one, 1, None, None, None, None, 0) == EKF_ERR_STATE     # the source
        assert b"ekf_join_maps: source trajectory 0" in lib.ekf_last_error(good._h)
        assert same(good.state(), G) and good.size() == 11 and good.flags() == 0
        assert lib.ekf_join_maps(bad._h, one, good._h, one, 1, None, None, None, None, 0) == EKF_ERR_STATE     # the destination
        assert b"destination trajectory 0" in lib.ekf_last_error(bad._h)
        assert bad.flags(0) & eb.EKF_FLAG_INTERNAL and bad.size() == 103 and same(good.state(), G)
