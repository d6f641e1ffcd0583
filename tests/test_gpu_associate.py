"""GPU: likelihood association of unlabelled observations (ekf_associate, EkfSlam.associate / step_unlabelled,
evaluation.association_check).

The reference is NumPy (tests/assoc_world.py: ref_scores) on the flushed state() taken AFTER the query -- the query changes
nothing.  Tolerances: NIS relative 1e-9 cond_2(S_ref), ln det S absolute 2e-9 cond_2(S_ref) (1e-9 is the project's TIGHT bound
on covariance entries against the oracle; a relative perturbation eps of S moves y^T S^-1 y by at most about cond(S) eps).  The
two candidates must equal the reference's two best wherever the reference's scores at ranks 1/2 and 2/3 differ by more than
that tolerance (at most 1 % of the observations excused); entries whose unwrapped bearing residual lies within 1e-9 of an odd
multiple of pi are left out (at most 0.1 %)."""
import ctypes as C

import numpy as np
import pytest

from oracle import ekf_oracle as orc
from tests import assoc_world as aw
from tests.conftest import path_ran
from tests.gpu_support import counters, sd, tag  # noqa: F401

pytestmark = pytest.mark.gpu

EKF_ERR_ARG = -1
PATH_TOL = 1e-10
TOTALS = aw.TOTALS


def check_query(f, zr, zb, m=None, meas_sigma=None, what="", res=None):
    """aw.check_query against the state downloaded after the query."""
    return aw.check_query(f, f.state, zr, zb, m, meas_sigma, what, res)


def obs_around(rng, f, m, b_count=None):
    """Continuous random observations near the map: range / bearing of random landmarks from the current mean, perturbed."""
    B = f.batch if b_count is None else b_count
    zr, zb = np.zeros((B, m)), np.zeros((B, m))
    for b in range(B):
        mu = f.mean(b)
        N = (len(mu) - 3) // 2
        for q in range(m):
            if N:
                l = int(rng.integers(N))
                d = mu[3 + 2 * l:5 + 2 * l] - mu[:2] + rng.normal(0, 0.05, 2)
            else:
                d = rng.normal(0, 1.0, 2)
            zr[b, q] = np.hypot(*d)
            zb[b, q] = orc.wrap_pi(np.arctan2(d[1], d[0]) - mu[2] + rng.normal(0, 0.02))
    return zr, zb


def bank_streams(N, steps, B, seed):
    return [orc.synthetic_stream(N, steps, 8, seed + t) for t in range(B)]


def step_bank(f, streams, k):
    f.step(np.array([s[2][k] for s in streams]), np.array([s[3][k] for s in streams]), np.stack([s[4][k] for s in streams]),
           np.stack([s[5][k] for s in streams]), np.stack([s[6][k] for s in streams]))


def stream_args(streams):
    return tuple(np.stack([np.asarray(s[i]) for s in streams], 1) for i in (2, 3, 4, 5, 6))


def dense_start_from(rng, n):
    A = rng.normal(size=(n, 6)) * 0.3
    P = A @ A.T
    P[np.arange(n), np.arange(n)] += rng.uniform(0.5, 2.0, n)
    return P


# ---- states -----------------------------------------------------------------------------------------------------------------
def test_nothing_pending_and_bit_identical_between_two_calls(sd):
    N, B = 300, 2
    n = 3 + 2 * N
    rng = np.random.default_rng(1)
    with sd.EkfSlam(n, batch=B) as f:
        for b in range(B):
            f.set_state(rng.normal(size=n), dense_start_from(rng, n), b)
        zr, zb = obs_around(rng, f, 8)
        a, _ = check_query(f, zr, zb)
        again = f.associate(zr, zb, full=True)
        for x, y in zip(a, again):
            assert np.array_equal(x, y, equal_nan=True)
        plain = f.associate(zr, zb)
        assert plain.all_nis is None and np.array_equal(plain.cand, a.cand) and np.array_equal(plain.nis, a.nis)
        assert np.array_equal(plain.min_nis, a.min_nis) and np.array_equal(plain.logdet, a.logdet)


def test_ranks_pending_on_the_per_step_kernels(sd):
    N, B, steps = 500, 3, 3
    streams = bank_streams(N, steps + 1, B, 40)
    rng = np.random.default_rng(2)
    with sd.EkfSlam(3 + 2 * N, batch=B) as f:
        f.set_option("fused_cadence", 0)
        f.profile_enable(True)
        for b, s in enumerate(streams):
            f.set_state(s[0], np.diag(s[1]), b)
        for k in range(steps):
            step_bank(f, streams, k)
        zr, zb = obs_around(rng, f, 8)
        passes = f.profile_passes()
        a = f.associate(zr, zb, full=True)
        assert f.profile_passes() == passes                   # no covariance pass
        check_query(f, zr, zb, res=a)
        assert f.profile_passes() == passes + 1                # ranks were pending: the reference's flush ran the pass


@pytest.mark.parametrize("N,chain", [(1250, 0), (2000, 1)])
def test_stream_pieces_ending_mid_cadence_and_non_interference(sd, N, chain):
    """stream_run in pieces that end mid-cadence (look-ahead at N = 1250 x 1, chained at N = 2000 x 1) with queries between the
    pieces: each against the reference, and the run's final state bit-identical to the same pieces without queries, with
    equal cadence, chained, look-ahead and pass counts."""
    n, steps = 3 + 2 * N, 22
    s = orc.synthetic_stream(N, steps, 8, 77)
    rng = np.random.default_rng(5)
    P0 = dense_start_from(rng, n)
    args = tuple(np.asarray(a)[:, None] for a in (s[2], s[3], s[4], s[5], s[6]))
    pieces = [(0, 7), (7, 6), (13, 9)]                      # 56, 104 updates: both boundaries inside a cadence of 40
    zs = [(rng.uniform(0.2, 3.0, (1, 8)), rng.uniform(-3.0, 3.0, (1, 8))) for _ in pieces]

    def run(query):
        with sd.EkfSlam(n, batch=1) as f:
            f.set_option("chain", chain)
            f.profile_enable(True)
            f.set_state(s[0], P0)
            f.stream_upload(*args)
            got = []
            for (first, count), (zr, zb) in zip(pieces, zs):
                f.stream_run(first, count)
                if query:
                    passes = f.profile_passes()
                    got.append(f.associate(zr, zb, full=True))
                    assert f.profile_passes() == passes
            return got, f.state(0), counters(sd, f)

    q, plain = run(True), run(False)
    assert np.array_equal(q[1][0], plain[1][0]) and np.array_equal(q[1][1], plain[1][1])
    assert q[2][:5] == plain[2][:5]                         # cadences, steps covered, chained, look-aheads, passes
    assert q[2].lookaheads > 0 and (q[2].chained > 0) == bool(chain)     # the look-ahead ran, chained where asked
    # each query against the reference: replay the pieces, flushing after the query this time
    with sd.EkfSlam(n, batch=1) as f:
        f.set_option("chain", chain)
        f.set_state(s[0], P0)
        f.stream_upload(*args)
        for i, ((first, count), (zr, zb)) in enumerate(zip(pieces, zs)):
            f.stream_run(first, count)
            a, _ = check_query(f, zr, zb, what=f"piece {i}: ")
            if i == 0:                                        # (later pieces started from a flushed state here: other rounding)
                for x, y in zip(a, q[0][0]):
                    assert np.array_equal(x, y, equal_nan=True)


def test_fused_cadence_against_per_step_kernels(sd):
    """The same stream through the fused cadence and through per-step launches, ranks pending on both: within 1e-10 cond(S)."""
    N, B, steps = 500, 2, 7
    streams = bank_streams(N, steps, B, 300)
    rng = np.random.default_rng(7)
    zr, zb = rng.uniform(0.2, 3.0, (B, 8)), rng.uniform(-3.0, 3.0, (B, 8))
    res = []
    for fused in (1, 0):
        with sd.EkfSlam(3 + 2 * N, batch=B) as f:
            f.set_option("fused_cadence", fused)
            for b, s in enumerate(streams):
                f.set_state(s[0], dense_start_from(np.random.default_rng(b), 3 + 2 * N), b)
            if fused:
                f.run_stream(*stream_args(streams))
                assert f.cadence_counters()[0] > 0
            else:
                for k in range(steps):
                    step_bank(f, streams, k)
                assert f.cadence_counters()[0] == 0
            a, conds = check_query(f, zr, zb, what=f"fused={fused}: ")
            res.append(a)
    cond = np.stack(conds)[:, None, :]
    assert (np.abs(res[0].all_nis - res[1].all_nis) <= PATH_TOL * cond * np.abs(res[1].all_nis)).all()
    assert (np.abs(res[0].all_logdet - res[1].all_logdet) <= 2 * PATH_TOL * cond).all()


def test_bank_of_32_with_trajectories_of_different_sizes(sd):
    B, steps, Nmax = 32, 3, 300
    rng = np.random.default_rng(11)
    sizes = [int(x) for x in rng.integers(40, Nmax + 1, B)]
    sizes[0], sizes[5], sizes[31] = Nmax, 64, 65
    streams = bank_streams(Nmax, steps, B, 500)
    with sd.EkfSlam(3 + 2 * Nmax, batch=B) as f:
        f.set_option("fused_cadence", 0)
        for b, s in enumerate(streams):
            nb = 3 + 2 * sizes[b]
            f.set_state_diag(s[0][:nb], s[1][:nb], b)
        for k in range(steps):
            idx = [np.unique(np.asarray(s[4][k]) % sizes[b]) for b, s in enumerate(streams)]
            f.step(np.array([s[2][k] for s in streams]), np.array([s[3][k] for s in streams]), idx,
                   [s[5][k][:len(i)] for s, i in zip(streams, idx)], [s[6][k][:len(i)] for s, i in zip(streams, idx)])
        zr, zb = obs_around(rng, f, 8)
        m = rng.integers(0, 9, B).astype(np.int32)            # m = 0 rows among them
        m[3] = 0
        a, _ = check_query(f, zr, zb, m)
        assert a.all_nis.shape == (B, 8, Nmax)


def test_young_filter_with_landmarks_beyond_the_active_bound(sd):
    N, steps, m = 1000, 7, 8
    n = 3 + 2 * N
    s = orc.synthetic_stream(N, steps, m, 13)
    diag = np.full(n, 1e4)
    diag[:3] = s[1][:3]
    idx = (np.arange(steps * m, dtype=np.int32) * 3).reshape(steps, m)   # every update a landmark never seen before
    args = tuple(np.asarray(a)[:, None] for a in (s[2], s[3], idx, s[5], s[6]))
    rng = np.random.default_rng(3)
    with sd.EkfSlam(n, batch=1) as f:
        f.profile_enable(True)
        f.set_state_diag(s[0], diag)
        f.run_stream(*args)                                # 56 updates: the last 16 (new landmarks) stay pending
        zr, zb = obs_around(rng, f, 8)
        passes = f.profile_passes()
        a = f.associate(zr, zb, full=True)
        assert f.profile_passes() == passes
        check_query(f, zr, zb, res=a)
        assert f.profile_passes() == passes + 1            # ranks were pending


def test_column_panels(sd):
    """N = 2100 (n = 4203 > 4096: P_base in column panels; landmark 2046 straddles the panel boundary), ranks pending."""
    N, steps = 2100, 6
    s = orc.synthetic_stream(N, steps, 8, 91)
    idx = s[4].copy()
    idx[:, :4] = (2040 + np.arange(4))[None, :] + 4 * np.arange(steps)[:, None] % 12   # landmarks around the boundary
    idx[:, 4:] = (idx[:, :4] + 30) % N
    rng = np.random.default_rng(4)
    with sd.EkfSlam(3 + 2 * N, batch=1) as f:
        f.set_option("fused_cadence", 0)
        f.set_state_diag(s[0], s[1])
        for k in range(steps):
            f.step(s[2][k], s[3][k], idx[k], s[5][k], s[6][k])
        mu = f.mean(0)
        near = [2044, 2045, 2046, 2047, 2048, 10, 1000, 2099]
        d = np.stack([mu[3 + 2 * l:5 + 2 * l] - mu[:2] for l in near]) + rng.normal(0, 0.02, (8, 2))
        zr, zb = np.hypot(d[:, 0], d[:, 1])[None, :], orc.wrap_pi(np.arctan2(d[:, 1], d[:, 0]) - mu[2])[None, :]
        check_query(f, zr, zb)


def test_small_state_path_and_general_kernels(sd, both_paths):
    N, steps, B = 20, 12, 4
    streams = bank_streams(N, steps, B, 700)
    rng = np.random.default_rng(6)
    with sd.EkfSlam(3 + 2 * N, batch=B) as f:
        for b, st in enumerate(streams):
            f.set_state_diag(st[0], st[1], b)
        f.run_stream(*stream_args(streams))
        zr, zb = obs_around(rng, f, 16)
        a, _ = check_query(f, zr, zb)
        assert path_ran(f, both_paths)
        if both_paths == "default_path":                  # nothing is ever pending there: the same bits again
            again = f.associate(zr, zb, full=True)
            assert np.array_equal(a.all_nis, again.all_nis, equal_nan=True) and np.array_equal(a.cand, again.cand)


def test_per_trajectory_meas_sigma(sd):
    N, B, steps = 200, 3, 3
    streams = bank_streams(N, steps, B, 60)
    sig = np.array([0.7, 0.05, 2.0])
    rng = np.random.default_rng(8)
    with sd.EkfSlam(3 + 2 * N, batch=B) as f:
        f.set_option("fused_cadence", 0)
        for b, s in enumerate(streams):
            f.set_state(s[0], np.diag(s[1]), b)
        f.set_noise(meas_sigma=sig)
        for k in range(steps):
            step_bank(f, streams, k)
        zr, zb = obs_around(rng, f, 8)
        check_query(f, zr, zb, meas_sigma=sig)             # (ranks pending; the reference's download applied them)
        a = f.associate(zr, zb, full=True)
        f.set_noise()                                      # back to the handle's constants: trajectory 0 keeps its numbers
        b_, _ = check_query(f, zr, zb)
        assert np.array_equal(a.all_nis[0], b_.all_nis[0]) and not np.array_equal(a.all_nis[1], b_.all_nis[1])


def test_after_remove_landmarks(sd):
    N, B, steps = 200, 2, 3
    streams = bank_streams(N, steps, B, 80)
    rng = np.random.default_rng(9)
    with sd.EkfSlam(3 + 2 * N, batch=B) as f:
        f.set_option("fused_cadence", 0)
        for b, s in enumerate(streams):
            f.set_state(s[0], np.diag(s[1]), b)
        for k in range(steps):
            step_bank(f, streams, k)
        f.remove_landmarks([3, 64, 65, 199], 0)
        assert f.size(0) == 3 + 2 * (N - 4) and f.size(1) == 3 + 2 * N
        step_bank(f, [(s[0], s[1], s[2], s[3], np.asarray(s[4]) % (N - 4), s[5], s[6]) for s in streams], 0)
        zr, zb = obs_around(rng, f, 8)
        a, _ = check_query(f, zr, zb)
        assert np.isnan(a.all_nis[0, :, N - 4:]).all() and not np.isnan(a.all_nis[1]).any()


def test_after_step_detections_grew_the_state(sd):
    """The device-side association grew the maps (sizes refreshed by the query itself), ranks pending.  Twice: with the
    reference's constants (meas_sigma 0.7), checked against the NumPy reference; and with a sharp filter (meas_sigma 0.03), where
    each tag's own measurement must pick its own landmark.
    The sharp filter is NOT held to the NIS tolerance, by reasoning: a landmark starts at variance 1e4 and its first update
    leaves ~1e-3 -- P_base + sum W V cancels seven digits, in the query and in the covariance pass behind the reference alike,
    each in its own order (absolute error ~1e4 x 2^-53 ~ 1e-12 on an S of ~1e-3).  Measured there: NIS relative error up to
    3.4e-9 at cond(S) = 1.05 between the two, which says nothing about either."""
    rng = np.random.default_rng(21)
    ids = [int(i) for i in rng.permutation(500)[:11]]
    bx = {i: float(rng.uniform(-0.5, 0.5)) for i in ids}
    bz = {i: float(rng.uniform(0.4, 1.1)) for i in ids}

    def window(k, win_ids):
        return [(k + 0.1 * fr, [tag(i, bx[i] + rng.normal(0, 0.004), bz[i] + rng.normal(0, 0.004)) for i in win_ids])
                for fr in range(2)]

    for cfg in (sd.EkfConfig(), sd.EkfConfig(motion_sigma=0.02, meas_sigma=0.03)):
        with sd.EkfSlam(3 + 2 * 100, batch=2, config=cfg) as f:  # (beyond the small-state limit: the sizes grow on the device)
            for k, w in enumerate([ids[:6], ids[2:9], ids[:4]]):
                f.step_detections(0.004, 0.02, [window(k, w), window(k, w[:3])])
            # the query comes first: it has to refresh the sizes the device-side association grew
            zr, zb = rng.uniform(0.3, 1.2, (2, 6)), rng.uniform(-1.0, 1.0, (2, 6))
            a = f.associate(zr, zb, full=True)
            assert f.assoc_fallbacks() == 0 and f.size(0) == 3 + 2 * 9 and f.size(1) == 3 + 2 * 5
            assert a.all_nis.shape == (2, 6, 9) and np.isnan(a.all_nis[1, :, 5:]).all() and not np.isnan(a.all_nis[0]).any()
            if cfg.meas_sigma == 0.7:
                check_query(f, zr, zb, res=a)
                continue
            # the tags' own positions, unlabelled: each observation's best candidate is its tag's landmark
            tp = f.tags_positions(0)
            own = f.associate([[tp[j][4] for j in tp], []], [[tp[j][5] for j in tp], []])
            assert list(own.cand[0, :len(tp), 0]) == list(tp.keys()) and len(f.tag_index(0)) == 9
            assert (own.cand[1] == -1).all()


def test_no_observations_and_no_landmarks(sd):
    with sd.EkfSlam(3 + 2 * 50, batch=3) as f:
        mu = np.concatenate([[0.0, 0.0, 0.1], np.random.default_rng(0).uniform(-2, 2, 100)])
        f.set_state_diag(mu, np.full(103, 0.5), 0)
        f.set_state_diag(mu[:5], np.full(5, 0.5), 2)        # trajectory 1 keeps the start: no landmarks; 2 has one
        zr, zb = np.full((3, 4), 1.0), np.full((3, 4), 0.3)
        a, _ = check_query(f, zr, zb, np.array([4, 4, 2], dtype=np.int32))
        assert (a.cand[1] == -1).all() and np.isnan(a.nis[1]).all() and np.isnan(a.min_nis[1]).all()
        assert (a.cand[2, :2, 0] == 0).all() and (a.cand[2, :2, 1] == -1).all()
        z = f.associate(zr, zb, np.zeros(3, dtype=np.int32))
        assert (z.cand == -1).all() and np.isnan(z.nis).all() and np.isnan(z.min_nis).all()
        empty = f.associate([[], [], []], [[], [], []])
        assert empty.cand.shape == (3, 1, 2) and (empty.cand == -1).all()


# ---- errors -----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_leave_the_handle_usable(sd):
    lib = sd.load_library()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    N, B = 100, 2
    rng = np.random.default_rng(12)
    with sd.EkfSlam(3 + 2 * N, batch=B) as f:
        for b in range(B):
            f.set_state(rng.normal(size=3 + 2 * N), dense_start_from(rng, 3 + 2 * N), b)
        zr, zb = obs_around(rng, f, 4)
        m = np.full(B, 4, dtype=np.int32)
        cand = np.empty((B, 4, 2), dtype=np.int32)
        nis, ld, mn = np.empty((B, 4, 2)), np.empty((B, 4, 2)), np.empty((B, 4))
        an, al = np.empty((B, 4, N)), np.empty((B, 4, N))
        P = lambda x, t=dp: x.ctypes.data_as(t)

        def call(b0=0, count=B, zr_=zr, zb_=zb, m_=m, stride=4, cand_=cand, an_=an, al_=al, cap=N):
            return lib.ekf_associate(f._h, b0, count, P(zr_), P(zb_), P(m_, ip), stride, None if cand_ is None else P(cand_, ip),
                                     P(nis), P(ld), P(mn), None if an_ is None else P(an_), None if al_ is None else P(al_), cap)

        bad_z = zr.copy()
        bad_z[1, 2] = np.inf
        bad_b = zb.copy()
        bad_b[0, 0] = np.nan
        cases = [dict(b0=-1), dict(count=0), dict(b0=1, count=2), dict(stride=0), dict(stride=17),
                 dict(m_=np.array([4, 5], dtype=np.int32)), dict(m_=np.array([-1, 4], dtype=np.int32)), dict(zr_=bad_z),
                 dict(zb_=bad_b), dict(cand_=None), dict(cap=N - 1)]
        want, _ = check_query(f, zr, zb)
        for kw in cases:
            assert call(**kw) == EKF_ERR_ARG, kw
            assert lib.ekf_last_error(f._h).decode().startswith("ekf_associate"), kw
            assert call() == 0
            assert np.array_equal(cand, want.cand) and np.array_equal(an, want.all_nis) and np.array_equal(mn, want.min_nis)
        # a non-finite entry beyond m[b] is not an observation
        assert call(zr_=bad_z, m_=np.array([4, 2], dtype=np.int32)) == 0
        assert call(an_=None, al_=None, cap=0) == 0 and np.array_equal(cand, want.cand)
        assert f.flags(0) == 0 and f.flags(1) == 0


# ---- end to end -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["5x5", "6x6"])
def test_step_unlabelled_recovers_the_labels_bit_identical_to_the_labelled_run(sd, name):
    """Bank of 3 (seeds 0 - 2): step_unlabelled against the truth, and mean / covariance bit-identical to the labelled run made
    from predict, add_landmarks in the same order, and update.  5 x 5 runs on the small-state path (n_max = 53); the 6 x 6
    handle is given room for 40 landmarks (n_max = 83, beyond the small-state limit of 79), so that it runs the general kernels
    with ranks pending at every query."""
    B = 3
    runs = [aw.make_run(name, seed)[1] for seed in aw.SEEDS]
    side = aw.WORLDS[name][0]
    N = side * side
    cfg = sd.EkfConfig(motion_sigma=0.02, meas_sigma=0.03)
    n_max = 3 + 2 * (N if name == "5x5" else 40)
    with sd.EkfSlam(n_max, batch=B, config=cfg) as f, sd.EkfSlam(n_max, batch=B, config=cfg) as g:
        for k in range(len(runs[0])):
            lin, ang = runs[0][k][0], runs[0][k][1]
            zr, zb = np.stack([r[k][3] for r in runs]), np.stack([r[k][4] for r in runs])
            before = [(g.size(b) - 3) // 2 for b in range(B)]
            assign = f.step_unlabelled(lin, ang, zr, zb)
            # the labelled run: world landmark w is filter landmark w here (first sights come in ascending order)
            g.predict(lin, ang)
            for b in range(B):
                vis = runs[b][k][2]
                assert list(assign[b]) == list(vis), (k, b)
                new = [q for q, w in enumerate(vis) if w >= before[b]]
                if new:
                    assert [vis[q] for q in new] == list(range(before[b], before[b] + len(new)))
                    x0, y0, th = g.mean(b)[:3]
                    g.add_landmarks(np.array([(x0 + zr[b, q] * np.cos(zb[b, q] + th), y0 + zr[b, q] * np.sin(zb[b, q] + th))
                                              for q in new]), b)
            g.update([r[k][2] for r in runs], list(zr), list(zb))
        for b in range(B):
            (mf, Pf), (mg, Pg) = f.state(b), g.state(b)
            assert len(mf) == 3 + 2 * N and np.array_equal(mf, mg) and np.array_equal(Pf, Pg)
        assert path_ran(f, "default_path") and path_ran(g, "default_path")
        assert (sd.load_library().ekf_debug_small_launches(f._h) > 0) == (name == "5x5")


def test_association_check_flags_exactly_the_swapped_labels(sd):
    from slam_duckietown_amd import evaluation as ev
    B, name = 3, "5x5"
    runs = [aw.make_run(name, seed)[1] for seed in aw.SEEDS]
    N = 25
    cfg = sd.EkfConfig(motion_sigma=0.02, meas_sigma=0.03)
    with sd.EkfSlam(3 + 2 * N, batch=B, config=cfg) as f:
        for k in range(40):
            f.step_unlabelled(runs[0][k][0], runs[0][k][1], np.stack([r[k][3] for r in runs]), np.stack([r[k][4] for r in runs]))
        k = 40
        f.predict(runs[0][k][0], runs[0][k][1])
        idx = [np.array(r[k][2]) for r in runs]
        zr, zb = [r[k][3] for r in runs], [r[k][4] for r in runs]
        before = f.state(1)
        assert ev.association_check(f, idx, zr, zb) == []
        assert ev.association_check(f, idx, zr, zb, margin=32.0) == []      # the worlds' runner-up margin
        idx[0][[1, 3]] = idx[0][[3, 1]]                       # two tags of trajectory 0 read as each other
        idx[2][4] = (idx[2][4] + 7) % N                       # one tag of trajectory 2 misread
        flags = ev.association_check(f, idx, zr, zb)
        assert [(x.b, x.q) for x in flags] == [(0, 1), (0, 3), (2, 4)]
        assert [x.best for x in flags] == [runs[0][k][2][1], runs[0][k][2][3], runs[2][k][2][4]]
        assert all(x.d_labelled > x.d_other + 32.0 for x in flags)
        after = f.state(1)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_zz_caps_on_what_was_left_out_or_excused():
    """Over everything the tests above compared: at most 0.1 % of the entries left out, at most 1 % of the observations excused."""
    print(TOTALS)
    assert TOTALS["entries"] > 0 and TOTALS["obs"] > 0
    assert TOTALS["left_out"] <= 1e-3 * TOTALS["entries"]
    assert TOTALS["excused"] <= 1e-2 * TOTALS["obs"]
